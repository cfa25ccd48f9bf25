"""Cash-flow schedules (smmc_engine_simulate_cashflow) on the GPU against the numpy float32 restatement of
include/smmc.h's arithmetic over the CPU oracle's returns (tests/cashflow_reference.py).

final, paid and ruin_period are compared on their bits, depleted_at exactly; of the statistics record the integer
fields, min, max and bucket counts with ==, the two double sums to the relative 1e-12 of tests/test_gpu_parity.py
(the device adds in another order).  Capital 1000, floor 0.01, first_path 3 throughout; on 2000 paths the
restatement depletes 0.55 (Gaussian) / 0.63 (table) with 6.0 per period over 360 periods, 0.375 / 0.66 with
3.0 + 0.2 % over 1000, none with 0.4 % alone.  The 7-period shapes take 145 per period (about capital / 7),
which depletes 0.36 / 0.49 / 0.43 of 8199 paths; the tests assert 0 < depleted < n on the restatement's answer."""
import functools

import numpy as np
import pytest

import cashflow_reference as ref

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("cashflow")

N_MAX = 2 * 4099 + 1
PATHS = [1, 255, 4099, N_MAX]   # one path; a partial wave; a ragged last chunk past one workgroup walk; more of it
PERIODS = [7, 360, 1000]        # below one Philox block; a multiple of 8 and of 4; neither
MODES = ["gaussian", "table", "table3001"]
SCHEDULES = ["amount", "fraction", "both", "arrays"]
BINS, LO, HI, BELOW = 64, 0.0, 4000.0, 500.0


def _mode(name):
    from stock_market_monte_carlo_amd import MODE_GAUSSIAN, MODE_TABLE
    return (MODE_GAUSSIAN, "none") if name == "gaussian" else (MODE_TABLE, "bundled" if name == "table" else "big")


@pytest.fixture(scope="module")
def engines(table):
    import stock_market_monte_carlo_amd as S
    e, big = S.Engine(0), S.Engine(0)
    e.set_table(table)
    big.set_table(ref.big_table())
    yield {"gaussian": e, "table": e, "table3001": big}
    e.close()
    big.close()


def schedule(name, P):
    """(amount, fraction, amounts, fractions) of a named schedule for P periods."""
    base = 145.0 if P == 7 else 6.0
    if name == "amount":
        return base, 0.0, None, None
    if name == "fraction":
        return 0.0, 0.004, None, None
    if name == "both":
        return (base if P == 7 else 3.0), 0.002, None, None
    if name == "zero":
        return 0.0, 0.0, None, None
    assert name == "arrays"  # the amount grows 0.2 % per period (indexed to inflation), the fraction alternates
    am = (np.float64(base) * 1.002 ** np.arange(P)).astype(np.float32)
    fr = np.where(np.arange(P) % 2 == 0, 0.0, 0.002).astype(np.float32)
    return 0.0, 0.0, am, fr


@functools.lru_cache(maxsize=None)
def _reference(oracle, mode_name, P, sched, floor=ref.FLOOR):
    """The restatement's (final, paid, ruin) of paths 3 .. 3 + N_MAX; computed once, shared, never modified."""
    mode, key = _mode(mode_name)
    R = ref.cached_returns(oracle, mode, key, N_MAX, P)
    amount, fraction, am, fr = schedule(sched, P)
    v, paid, ruin, _ = ref.simulate(R, amount if am is None else am, fraction if fr is None else fr, floor)
    for a in (v, paid, ruin):
        a.setflags(write=False)
    return v, paid, ruin


def _sim(mode_name, n, P, first=ref.FIRST_PATH, exact_div=False, n_bins=BINS):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(n, P, _mode(mode_name)[0], ref.SEED, first_path=first, initial_capital=ref.CAPITAL, n_bins=n_bins,
                             hist_lo=LO, hist_hi=HI, below_threshold=BELOW, exact_div=exact_div)


def _run(eng, sim, sched, floor=ref.FLOOR, to_host=False, **want):
    """All outputs (or those named in want) as host arrays: final, paid (float32), ruin_period (uint32), stats_raw
    (bytes), depleted_at (uint64)."""
    amount, fraction, am, fr = schedule(sched, int(sim.n_periods))
    if not want:
        want = dict(want_final=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
    full = dict(want_final=False, want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=False)
    full.update(want)
    if to_host:
        return eng.simulate_cashflow_to_host(sim, amount, fraction, am, fr, floor, **full)
    raw = eng.simulate_cashflow_raw(sim, amount, fraction, am, fr, floor, **full)
    eng.sync()
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in raw.items()}
    if out["ruin_period"] is not None:
        out["ruin_period"] = out["ruin_period"].view(np.uint32)
    if out["depleted_at"] is not None:
        out["depleted_at"] = out["depleted_at"].view(np.uint64)
    if out["stats_raw"] is not None:
        out["stats_raw"] = out["stats_raw"].tobytes()
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against(oracle, out, v, paid, ruin, P, tag):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    n = v.size
    assert np.array_equal(_bits(out["final"]), _bits(v)), tag
    assert np.array_equal(_bits(out["paid"]), _bits(paid)), tag
    assert np.array_equal(out["ruin_period"], ruin), tag
    dep = out["depleted_at"]
    assert dep.size == P + 1 and int(dep.sum()) == n, tag
    assert np.array_equal(dep, np.bincount(ruin, minlength=P + 1).astype(np.uint64)), tag
    st = stats_from_bytes(out["stats_raw"])
    ost, ohist = oracle.values_stats(v, BELOW, BINS, LO, HI)
    assert st.count == ost.count == n, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert st.min == ost.min and st.max == ost.max, tag
    assert np.array_equal(st.hist, ohist) and int(st.hist.sum()) + st.underflow + st.overflow == n, tag
    assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("n", PATHS)
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("mode_name", MODES)
def test_parity_with_the_restatement(engines, oracle, mode_name, P, n, sched):
    v, paid, ruin = _reference(oracle, mode_name, P, sched)
    depleted = int((ruin > 0).sum())
    print(f"{mode_name} P={P} {sched}: the restatement depletes {depleted} of {N_MAX}")
    if P == 7 and sched != "fraction":
        assert 0 < depleted < N_MAX  # a degenerate input must not hide a kernel bug
    out = _run(engines[mode_name], _sim(mode_name, n, P), sched)
    _check_against(oracle, out, v[:n], paid[:n], ruin[:n], P, (mode_name, P, n, sched))


def test_the_restatement_depletes_the_stated_shares(oracle):
    """The shares the inputs were chosen by, on the first 2000 paths (floor 0.01, from first_path 3)."""
    share = lambda m, P, s: float((_reference(oracle, m, P, s)[2][:2000] > 0).mean())  # noqa: E731
    assert share("gaussian", 360, "amount") == pytest.approx(0.55, abs=0.005)
    assert share("table", 360, "amount") == pytest.approx(0.63, abs=0.005)
    assert share("gaussian", 1000, "both") == pytest.approx(0.375, abs=0.005)
    assert share("table", 1000, "both") == pytest.approx(0.66, abs=0.005)
    assert share("gaussian", 360, "fraction") == share("table", 1000, "fraction") == 0.0


@pytest.mark.parametrize("mode_name", MODES)
def test_zero_flow_is_the_plain_simulation(engines, mode_name):
    """amount = fraction = 0, floor 0: final values bit-identical to Engine.simulate for the same sim."""
    eng, n, P = engines[mode_name], N_MAX, 360
    sim = _sim(mode_name, n, P)
    plain = eng.simulate(sim).final.cpu().numpy()
    out = _run(eng, sim, "zero", floor=0.0)
    assert np.array_equal(_bits(out["final"]), _bits(plain))
    assert not out["ruin_period"].any() and not _bits(out["paid"]).any()
    assert int(out["depleted_at"][0]) == n and int(out["depleted_at"].sum()) == n


def _same_outputs(a, b, tag=None):
    for k in ("final", "paid", "ruin_period", "depleted_at"):
        assert (a[k] is None) == (b[k] is None), (tag, k)
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
    assert a["stats_raw"] == b["stats_raw"], tag


@pytest.mark.parametrize("mode_name", MODES)
def test_divide_variants_give_the_same_bytes(engines, oracle, mode_name):
    from stock_market_monte_carlo_amd import _lib
    # 360 periods; the 3001-entry table's +25 % entries leave the fast form's proof only 120 (1.25^360 > 2^115)
    eng, n, P = engines[mode_name], 4099, (120 if mode_name == "table3001" else 360)
    amount, fraction, _, _ = schedule("amount", P)
    assert eng.cashflow_divide_kind(_sim(mode_name, n, P), amount, fraction, floor=ref.FLOOR) == _lib.DIV_FAST
    assert eng.cashflow_divide_kind(_sim(mode_name, n, P, exact_div=True), amount, fraction, floor=ref.FLOOR) == _lib.DIV_EXACT
    for sched in ("amount", "arrays"):
        _same_outputs(_run(eng, _sim(mode_name, n, P), sched), _run(eng, _sim(mode_name, n, P, exact_div=True), sched), sched)
    # half of the value goes every period: values collapse towards the floor and every path is depleted early
    assert eng.cashflow_divide_kind(_sim(mode_name, n, P), 0.0, 0.5, floor=ref.FLOOR) == _lib.DIV_FAST
    collapse = lambda exact: eng.simulate_cashflow_to_host(  # noqa: E731
        _sim(mode_name, n, P, exact_div=exact), 0.0, 0.5, floor=ref.FLOOR, want_paid=True, want_ruin_period=True, want_stats=True)
    fast, exact = collapse(False), collapse(True)
    _same_outputs(fast, exact, "collapse")
    assert fast["ruin_period"].min() > 0 and fast["ruin_period"].max() < 40 and int(fast["depleted_at"][0]) == 0  # 1000 / 2^17 < 0.01
    mode, key = _mode(mode_name)
    v, paid, ruin, dep = ref.simulate(ref.cached_returns(oracle, mode, key, N_MAX, P)[:n], 0.0, 0.5, ref.FLOOR)
    assert np.array_equal(_bits(fast["paid"]), _bits(paid)) and np.array_equal(fast["ruin_period"], ruin)
    assert np.array_equal(fast["depleted_at"], dep) and not fast["final"].any()


@pytest.mark.parametrize("mode_name,sched", [("gaussian", "amount"), ("table", "arrays"), ("table3001", "both")])
def test_shards_of_one_request_merge(engines, mode_name, sched):
    """Split at an odd boundary into two calls with shifted first_path: the per-path outputs concatenate, the
    records merge by smmc_stats_merge, the depletion counts add.  (The schedule's index is the period, so both
    shards get the same arrays.)"""
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes, stats_from_bytes
    eng, n, P, cut = engines[mode_name], 4099, 360, 1531
    whole = _run(eng, _sim(mode_name, n, P), sched)
    a = _run(eng, _sim(mode_name, cut, P), sched)
    b = _run(eng, _sim(mode_name, n - cut, P, first=ref.FIRST_PATH + cut), sched)
    for k in ("final", "paid", "ruin_period"):
        assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes(), k
    assert np.array_equal(a["depleted_at"] + b["depleted_at"], whole["depleted_at"])
    m, w = stats_from_bytes(merge_stats_bytes([a["stats_raw"], b["stats_raw"]])), stats_from_bytes(whole["stats_raw"])
    assert (m.count, m.below, m.underflow, m.overflow, m.min, m.max) == (w.count, w.below, w.underflow, w.overflow, w.min, w.max)
    assert np.array_equal(m.hist, w.hist)
    assert m.sum == pytest.approx(w.sum, rel=1e-12) and m.sumsq == pytest.approx(w.sumsq, rel=1e-12)


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_identical_calls_give_identical_bytes(engines, mode_name):
    """... also with a different call in between: the engine's accumulators are left zero, its staged schedule is
    the call's own."""
    eng = engines[mode_name]
    first = _run(eng, _sim(mode_name, 4099, 360), "arrays")
    _same_outputs(first, _run(eng, _sim(mode_name, 4099, 360), "arrays"), "again")
    other = _run(eng, _sim(mode_name, 2 * 4099 + 1, 1000), "both")
    eng.simulate(_sim(mode_name, 1000, 360), want_stats=True)  # another user of the engine's bucket accumulator
    _same_outputs(first, _run(eng, _sim(mode_name, 4099, 360), "arrays"), "after other calls")
    _same_outputs(other, _run(eng, _sim(mode_name, 2 * 4099 + 1, 1000), "both"), "the other call again")
    # calls back to back without a wait in between: each uploads its own schedule behind the kernel before it
    raws = [eng.simulate_cashflow_raw(_sim(mode_name, 4099, 360), *schedule(s, 360), ref.FLOOR, want_paid=True) for s in
            ("arrays", "amount", "arrays", "both", "arrays", "arrays")]
    eng.sync()
    for i in (0, 2, 4, 5):
        assert raws[i]["paid"].cpu().numpy().tobytes() == first["paid"].tobytes(), i
        assert raws[i]["depleted_at"].cpu().numpy().view(np.uint64).tobytes() == first["depleted_at"].tobytes(), i


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_each_output_alone_and_the_host_entry(engines, mode_name):
    eng, sim = engines[mode_name], _sim(mode_name, 4099, 360)
    everything = _run(eng, sim, "arrays")
    _same_outputs(everything, _run(eng, sim, "arrays", to_host=True), "to_host")
    for want, key in (("want_final", "final"), ("want_paid", "paid"), ("want_ruin_period", "ruin_period"),
                      ("want_stats", "stats_raw"), ("want_depleted_at", "depleted_at")):
        for to_host in (False, True):
            alone = _run(eng, sim, "arrays", to_host=to_host, **{want: True})
            assert [k for k, x in alone.items() if x is not None] == [key], (want, to_host)
            got, all_ = alone[key], everything[key]
            assert (got == all_) if key == "stats_raw" else (got.tobytes() == all_.tobytes()), (want, to_host)


def test_result_object_and_survival(engines, oracle):
    eng = engines["gaussian"]
    res = eng.simulate_cashflow(_sim("gaussian", 4099, 360), amount=6.0, floor=ref.FLOOR, want_stats=True)
    v, paid, ruin = _reference(oracle, "gaussian", 360, "amount")
    assert res.paid is None and res.ruin_period is None and res.stats.count == 4099
    assert np.array_equal(_bits(res.final.cpu().numpy()), _bits(v[:4099]))
    assert res.depleted_at.dtype == np.uint64 and res.depleted_at.size == 361
    s = res.survival()
    assert s.size == 361 and s[0] == 1.0 and np.all(np.diff(s) <= 0)
    assert s[-1] == pytest.approx(float((ruin[:4099] == 0).mean())) and s[-1] == pytest.approx(int(res.depleted_at[0]) / 4099)


def test_period_limits(engines):
    from stock_market_monte_carlo_amd import MAX_CASHFLOW_PERIODS, SmmcError
    eng = engines["table"]
    out = _run(eng, _sim("table", 64, MAX_CASHFLOW_PERIODS), "both")
    assert out["depleted_at"].size == MAX_CASHFLOW_PERIODS + 1 and int(out["depleted_at"].sum()) == 64
    assert out["ruin_period"].max() <= MAX_CASHFLOW_PERIODS
    assert np.array_equal(np.bincount(out["ruin_period"], minlength=MAX_CASHFLOW_PERIODS + 1), out["depleted_at"].astype(np.int64))
    with pytest.raises(SmmcError, match="SMMC_MAX_CASHFLOW_PERIODS"):
        _run(eng, _sim("table", 64, MAX_CASHFLOW_PERIODS + 1), "both")
