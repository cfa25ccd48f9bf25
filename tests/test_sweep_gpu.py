"""Cash-flow sweeps (smmc_engine_simulate_cashflow_sweep) on the GPU against the numpy float32 restatement of
include/smmc.h's arithmetic over the CPU oracle's returns (tests/cashflow_reference.py): scenario s of a sweep is the
restatement's simulate(R, amount[s], fraction[s], floor[s]).

Per scenario final, paid and ruin_period are compared on their bits, depleted_at exactly; of the statistics record the
integer fields, min, max and bucket counts with ==, the two double sums to the relative 1e-12 of tests/test_gpu_parity.py
against oracle.values_stats.  Capital 1000, floor 0.01, first_path 3, 64 buckets on [0, 4000), below-threshold 500, as
tests/test_cashflow_gpu.py.  The amount sets are those of tests/test_sweep_cpu.py, which states the shares they deplete;
smaller sweeps take a spread of them.

Evidence that the tests see a kernel that confuses its scenarios: a build made wrong on purpose -- `c.floor[0]` in the
place of `c.floor[sc]` in cashflow_sweep_kernel's step, every scenario depleted at scenario 0's floor -- was run once against
this file: test_mixed_scenarios_in_one_sweep and test_a_sweep_is_its_single_calls failed in all three modes (the scenario
with floor 50), the other 41 cases, whose scenarios share one floor, passed."""
import ctypes as C
import functools

import numpy as np
import pytest

import cashflow_reference as ref
from test_sweep_cpu import AMOUNTS, SHARES

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("cashflow_sweep")

N_MAX = 2 * 4099 + 1
PATHS = [1, 255, 4099, N_MAX]   # one path; a partial wave; a ragged last chunk past one workgroup walk; more of it
MODES = ["gaussian", "table", "table3001"]
# S = 3 and S = 5 run the instantiations for 4 and 8 with padding; P = 7 is below one Philox block, P = 1000 ends in a partial one
SHAPES = [(7, 8), (360, 8), (360, 3), (1000, 5), (360, 1)]
PICK = {8: range(8), 5: (0, 2, 4, 5, 7), 3: (0, 5, 7), 1: (5,)}  # which of a set's eight amounts a smaller sweep takes
BINS, LO, HI, BELOW = 64, 0.0, 4000.0, 500.0
# every mode meets every (P, S); the n walk round PATHS so that the six S = 8 cases meet all four
CASES = [(m, P, S, PATHS[(5 * i + j) % 4]) for i, m in enumerate(MODES) for j, (P, S) in enumerate(SHAPES)]
assert {n for _, _, S, n in CASES if S == 8} == set(PATHS)
# amount-only, fraction-only, both, a contribution, another floor, nothing, a floor of 0 (the IEEE divide for the sweep), 5.0
MIXED = [(6.0, 0.0, 0.01), (0.0, 0.004, 0.01), (3.0, 0.002, 0.01), (-2.0, 0.0, 0.01), (6.0, 0.0, 50.0), (0.0, 0.0, 0.0),
         (12.0, 0.0, 0.0), (5.0, 0.0, 0.01)]
SENTINEL = 0x7FC0BEEF  # a NaN pattern as float32


def _mode(name):
    from stock_market_monte_carlo_amd import MODE_GAUSSIAN, MODE_TABLE
    return (MODE_GAUSSIAN, "none") if name == "gaussian" else (MODE_TABLE, "bundled" if name == "table" else "big")


def _amounts(P, S):
    full = AMOUNTS[7 if P == 7 else 360]
    return [full[i] for i in PICK[S]]


@pytest.fixture(scope="module")
def engines(table):
    import stock_market_monte_carlo_amd as S
    e, big = S.Engine(0), S.Engine(0)
    e.set_table(table)
    big.set_table(ref.big_table())
    yield {"gaussian": e, "table": e, "table3001": big}
    e.close()
    big.close()


@functools.lru_cache(maxsize=None)
def _reference(oracle, mode_name, P, amount, fraction, floor):
    """The restatement's (final, paid, ruin) of paths 3 .. 3 + N_MAX for one scenario; computed once, shared, never modified."""
    mode, key = _mode(mode_name)
    v, paid, ruin, _ = ref.simulate(ref.cached_returns(oracle, mode, key, N_MAX, P), amount, fraction, floor)
    for a in (v, paid, ruin):
        a.setflags(write=False)
    return v, paid, ruin


def _sim(mode_name, n, P, first=ref.FIRST_PATH, exact_div=False, n_bins=BINS):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(n, P, _mode(mode_name)[0], ref.SEED, first_path=first, initial_capital=ref.CAPITAL, n_bins=n_bins,
                             hist_lo=LO, hist_hi=HI, below_threshold=BELOW, exact_div=exact_div)


ALL = dict(want_final=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
NONE = dict(want_final=False, want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=False)


def _run(eng, sim, scenarios, to_host=False, **want):
    """The outputs (all, or those named in want) as host arrays, scenario-major: final, paid (float32 [S, n]),
    ruin_period (uint32), stats_raw (S x bytes), depleted_at (uint64 [S, P + 1])."""
    am, fr, fl = ([s[i] for s in scenarios] for i in range(3))
    full = dict(NONE, **want) if want else ALL
    rec = int(eng._L.smmc_stats_bytes(sim.n_bins))
    if to_host:
        out = eng.simulate_cashflow_sweep_to_host(sim, am, fr, fl, **full)
    else:
        raw = eng.simulate_cashflow_sweep_raw(sim, am, fr, fl, **full)
        eng.sync()
        out = {k: (None if t is None else t.cpu().numpy()) for k, t in raw.items()}
        if out["ruin_period"] is not None:
            out["ruin_period"] = out["ruin_period"].view(np.uint32)
        if out["depleted_at"] is not None:
            out["depleted_at"] = out["depleted_at"].view(np.uint64)
        if out["stats_raw"] is not None:
            out["stats_raw"] = out["stats_raw"].tobytes()
    if out["stats_raw"] is not None:
        assert len(out["stats_raw"]) == rec * len(scenarios)
        out["stats_raw"] = [out["stats_raw"][s * rec:(s + 1) * rec] for s in range(len(scenarios))]
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_scenario(oracle, out, s, v, paid, ruin, P, tag, sums=None):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    n = v.size
    assert out["final"].shape[1] == n
    assert np.array_equal(_bits(out["final"][s]), _bits(v)), tag
    assert np.array_equal(_bits(out["paid"][s]), _bits(paid)), tag
    assert np.array_equal(out["ruin_period"][s], ruin), tag
    dep = out["depleted_at"][s]
    assert dep.size == P + 1 and int(dep.sum()) == n, tag
    assert np.array_equal(dep, np.bincount(ruin, minlength=P + 1).astype(np.uint64)), tag
    st = stats_from_bytes(out["stats_raw"][s])
    ost, ohist = oracle.values_stats(v, BELOW, BINS, LO, HI)
    assert st.count == ost.count == n, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert st.min == ost.min and st.max == ost.max, tag
    assert np.array_equal(st.hist, ohist) and int(st.hist.sum()) + st.underflow + st.overflow == n, tag
    want_sum, want_sumsq = sums if sums is not None else (ost.sum, ost.sumsq)
    assert st.sum == pytest.approx(want_sum, rel=1e-12) and st.sumsq == pytest.approx(want_sumsq, rel=1e-12), tag


def _check_sweep(oracle, out, mode_name, scenarios, n, P, tag):
    assert out["final"].shape == out["paid"].shape == out["ruin_period"].shape == (len(scenarios), n)
    assert out["depleted_at"].shape == (len(scenarios), P + 1)
    for s, sc in enumerate(scenarios):
        v, paid, ruin = _reference(oracle, mode_name, P, *sc)
        _check_scenario(oracle, out, s, v[:n], paid[:n], ruin[:n], P, tag + (s, sc))


@pytest.mark.parametrize("mode_name,P,S,n", CASES)
def test_parity_with_the_restatement(engines, oracle, mode_name, P, S, n):
    scenarios = [(a, 0.0, ref.FLOOR) for a in _amounts(P, S)]
    if S == 8 and P in (7, 360):  # a degenerate input must not hide a kernel bug: asserted on the restatement's answer
        shares = [float((_reference(oracle, mode_name, P, *sc)[2][:2000] > 0).mean()) for sc in scenarios]
        print(f"{mode_name} P={P}: the restatement depletes {shares} of the first 2000 paths")
        assert any(x == 0.0 for x in shares) and any(0.0 < x < 1.0 for x in shares)
        assert all(x == 1.0 for x, stated in zip(shares, SHARES[(mode_name, P)]) if stated == 1)
    _check_sweep(oracle, _run(engines[mode_name], _sim(mode_name, n, P), scenarios), mode_name, scenarios, n, P, (mode_name, P, S, n))


@pytest.mark.parametrize("mode_name", MODES)
def test_mixed_scenarios_in_one_sweep(engines, oracle, mode_name):
    """Amount-only, fraction-only, both, a contribution, differing floors: a kernel that reads a neighbour's parameter
    or shares an `alive` mask fails here (the module's docstring names the wrong build that did)."""
    n, P = 4099, 360
    ruins = [_reference(oracle, mode_name, P, *sc)[2][:n] for sc in MIXED]
    assert (ruins[0] != ruins[4]).any()  # floor 0.01 and floor 50 part ways
    assert not ruins[1].any() and not ruins[3].any() and not ruins[5].any() and 0 < (ruins[0] > 0).sum() < n and 0 < (ruins[7] > 0).sum() < n
    _check_sweep(oracle, _run(engines[mode_name], _sim(mode_name, n, P), MIXED), mode_name, MIXED, n, P, (mode_name, "mixed"))


def _single(eng, sim, sc):
    raw = eng.simulate_cashflow_raw(sim, sc[0], sc[1], None, None, sc[2], **ALL)
    eng.sync()
    return {k: t.cpu().numpy() for k, t in raw.items()}


@pytest.mark.parametrize("mode_name", MODES)
def test_a_sweep_is_its_single_calls(engines, mode_name):
    """Scenario s of a sweep against smmc_engine_simulate_cashflow of that scenario from the same engine, on the bits
    the contract lists."""
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng, n, P = engines[mode_name], N_MAX, 360
    sim = _sim(mode_name, n, P)
    out = _run(eng, sim, MIXED)
    for s, sc in enumerate(MIXED):
        one = _single(eng, sim, sc)
        assert np.array_equal(_bits(out["final"][s]), _bits(one["final"])), (s, sc)
        assert np.array_equal(_bits(out["paid"][s]), _bits(one["paid"])), (s, sc)
        assert np.array_equal(out["ruin_period"][s], one["ruin_period"].view(np.uint32)), (s, sc)
        assert np.array_equal(out["depleted_at"][s], one["depleted_at"].view(np.uint64)), (s, sc)
        a, b = stats_from_bytes(out["stats_raw"][s]), stats_from_bytes(one["stats_raw"].tobytes())
        assert (a.count, a.below, a.underflow, a.overflow, a.min, a.max) == (b.count, b.below, b.underflow, b.overflow, b.min, b.max)
        assert np.array_equal(a.hist, b.hist)
        assert a.sum == pytest.approx(b.sum, rel=1e-12) and a.sumsq == pytest.approx(b.sumsq, rel=1e-12)


def _same_outputs(a, b, tag=None):
    for k in ("final", "paid", "ruin_period", "depleted_at"):
        assert (a[k] is None) == (b[k] is None), (tag, k)
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
    assert a["stats_raw"] == b["stats_raw"], tag


@pytest.mark.parametrize("mode_name", MODES)
@pytest.mark.parametrize("S", [3, 5])
def test_padding_leaks_nothing(engines, mode_name, S):
    """The padded instantiations: buffers one scenario larger than the request keep their sentinel beyond S, every
    depleted_at row sums to n, and a scenario's outputs do not depend on how many others the sweep holds."""
    import torch
    eng, n, P = engines[mode_name], 4099, 360
    sim = _sim(mode_name, n, P)
    scenarios = MIXED[:S]
    rec = int(eng._L.smmc_stats_bytes(BINS))
    cfs, _, _, _ = eng.make_sweep(*[[s[i] for s in scenarios] for i in range(3)])
    fill = lambda count, dtype: torch.full((S + 1, count), SENTINEL, dtype=dtype, device=eng.tdevice)  # noqa: E731
    final, paid, ruin = fill(n, torch.int32), fill(n, torch.int32), fill(n, torch.int32)
    stats, dep = fill(rec // 4, torch.int32), fill(P + 1, torch.int64)
    cur = eng._enter()
    rc = eng._L.smmc_engine_simulate_cashflow_sweep(eng._h, C.byref(sim), cfs, S, *[C.c_void_p(t.data_ptr()) for t in (final, paid, ruin, stats, dep)])
    assert rc == 0, eng._L.smmc_last_error()
    eng._leave(cur, final, paid, ruin, stats, dep)
    eng.sync()
    for t in (final, paid, ruin, stats, dep):
        assert (t[S].cpu().numpy() == SENTINEL).all()
    assert (dep[:S].cpu().numpy().sum(axis=1) == n).all()
    got = {"final": final[:S].cpu().numpy().view(np.float32), "paid": paid[:S].cpu().numpy().view(np.float32),
           "ruin_period": ruin[:S].cpu().numpy().view(np.uint32), "depleted_at": dep[:S].cpu().numpy().view(np.uint64)}
    whole = _run(eng, sim, MIXED)  # the same scenarios as the first S of eight
    alone = _run(eng, sim, scenarios)
    for k, a in got.items():
        assert a.tobytes() == whole[k][:S].tobytes() == alone[k].tobytes(), k
    host = stats[:S].cpu().numpy().tobytes()
    assert [host[s * rec:(s + 1) * rec] for s in range(S)] == alone["stats_raw"]
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    for s in range(S):  # another launch geometry: the integer fields and the buckets, not the order of the double sums
        a, b = stats_from_bytes(alone["stats_raw"][s]), stats_from_bytes(whole["stats_raw"][s])
        assert (a.count, a.below, a.underflow, a.overflow, a.min, a.max) == (b.count, b.below, b.underflow, b.overflow, b.min, b.max)
        assert np.array_equal(a.hist, b.hist) and a.sum == pytest.approx(b.sum, rel=1e-12) and a.sumsq == pytest.approx(b.sumsq, rel=1e-12)


@pytest.mark.parametrize("mode_name", MODES)
def test_divide_variants_give_the_same_bytes(engines, mode_name):
    from stock_market_monte_carlo_amd import _lib
    # 360 periods; the 3001-entry table's +25 % entries leave the fast form's proof only 120 (as tests/test_cashflow_gpu.py)
    eng, n, P = engines[mode_name], 4099, (120 if mode_name == "table3001" else 360)
    fast = [sc for sc in MIXED if sc[2] > 0.0 or sc[0] == 0.0]  # without the amount on floor 0
    am, fr, fl = ([s[i] for s in fast] for i in range(3))
    assert len(fast) == 7 and eng.cashflow_sweep_divide_kind(_sim(mode_name, n, P), am, fr, fl) == _lib.DIV_FAST
    assert eng.cashflow_sweep_divide_kind(_sim(mode_name, n, P, exact_div=True), am, fr, fl) == _lib.DIV_EXACT
    assert eng.cashflow_sweep_divide_kind(_sim(mode_name, n, P), *([s[i] for s in MIXED] for i in range(3))) == _lib.DIV_EXACT
    _same_outputs(_run(eng, _sim(mode_name, n, P), fast), _run(eng, _sim(mode_name, n, P, exact_div=True), fast), "seven")
    amounts = [(a, 0.0, ref.FLOOR) for a in AMOUNTS[360]]
    _same_outputs(_run(eng, _sim(mode_name, n, P), amounts), _run(eng, _sim(mode_name, n, P, exact_div=True), amounts), "eight")


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_each_output_alone_and_the_host_entry(engines, mode_name):
    eng, sim = engines[mode_name], _sim(mode_name, 4099, 360)
    everything = _run(eng, sim, MIXED)
    _same_outputs(everything, _run(eng, sim, MIXED, to_host=True), "to_host")
    for want, key in (("want_final", "final"), ("want_paid", "paid"), ("want_ruin_period", "ruin_period"),
                      ("want_stats", "stats_raw"), ("want_depleted_at", "depleted_at")):
        for to_host in (False, True):
            alone = _run(eng, sim, MIXED, to_host=to_host, **{want: True})
            assert [k for k, x in alone.items() if x is not None] == [key], (want, to_host)
            got, all_ = alone[key], everything[key]
            assert (got == all_) if key == "stats_raw" else (got.tobytes() == all_.tobytes()), (want, to_host)
    pair = _run(eng, sim, MIXED, want_stats=True, want_depleted_at=True)  # what a survival curve needs: no per-path output
    assert pair["stats_raw"] == everything["stats_raw"] and pair["depleted_at"].tobytes() == everything["depleted_at"].tobytes()
    # without the record its buckets do not count towards SMMC_MAX_SWEEP_COUNTERS: 8 x (1000 + 1) fits, with 64 buckets it does not
    from stock_market_monte_carlo_amd import SmmcError
    counts = _run(eng, _sim(mode_name, 255, 1000), MIXED, want_depleted_at=True)
    assert (counts["depleted_at"].sum(axis=1) == 255).all()
    with pytest.raises(SmmcError, match="SMMC_MAX_SWEEP_COUNTERS"):
        _run(eng, _sim(mode_name, 255, 1000), MIXED, want_stats=True, want_depleted_at=True)


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_identical_calls_give_identical_bytes(engines, mode_name):
    """... records included, also with other users of the engine's accumulator in between: it is left zero."""
    eng = engines[mode_name]
    first = _run(eng, _sim(mode_name, 4099, 360), MIXED)
    _same_outputs(first, _run(eng, _sim(mode_name, 4099, 360), MIXED), "again")
    other = _run(eng, _sim(mode_name, N_MAX, 1000), MIXED[:5])
    eng.simulate(_sim(mode_name, 1000, 360), want_stats=True)
    eng.simulate_cashflow(_sim(mode_name, 1000, 360), amount=6.0, floor=ref.FLOOR, want_stats=True)
    _same_outputs(first, _run(eng, _sim(mode_name, 4099, 360), MIXED), "after other calls")
    _same_outputs(other, _run(eng, _sim(mode_name, N_MAX, 1000), MIXED[:5]), "the other call again")


@pytest.mark.parametrize("mode_name,S", [("gaussian", 8), ("table", 5), ("table3001", 3)])
def test_shards_of_one_request_merge(engines, mode_name, S):
    """Split at an odd boundary into two sweeps with shifted first_path: the per-path outputs concatenate, the records
    merge by smmc_stats_merge, the depletion counts add, scenario by scenario."""
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes, stats_from_bytes
    eng, n, P, cut, scenarios = engines[mode_name], 4099, 360, 1531, MIXED[:S]
    whole = _run(eng, _sim(mode_name, n, P), scenarios)
    a = _run(eng, _sim(mode_name, cut, P), scenarios)
    b = _run(eng, _sim(mode_name, n - cut, P, first=ref.FIRST_PATH + cut), scenarios)
    for k in ("final", "paid", "ruin_period"):
        assert np.concatenate([a[k], b[k]], axis=1).tobytes() == whole[k].tobytes(), k
    assert np.array_equal(a["depleted_at"] + b["depleted_at"], whole["depleted_at"])
    for s in range(S):
        m, w = stats_from_bytes(merge_stats_bytes([a["stats_raw"][s], b["stats_raw"][s]])), stats_from_bytes(whole["stats_raw"][s])
        assert (m.count, m.below, m.underflow, m.overflow, m.min, m.max) == (w.count, w.below, w.underflow, w.overflow, w.min, w.max)
        assert np.array_equal(m.hist, w.hist)
        assert m.sum == pytest.approx(w.sum, rel=1e-12) and m.sumsq == pytest.approx(w.sumsq, rel=1e-12)


# amounts for the 38 and 41 periods of tests/test_walk_trips_gpu.py (its own flows are 23 .. 29 per period)
TRIP_AMOUNTS = (0.0, 20.0, 24.0, 27.0, 29.0, 32.0, 40.0, 1001.0)


@pytest.mark.parametrize("mode_name", ["gaussian", "table", "table2500"])
def test_outputs_when_waves_make_several_trips(oracle, table, monkeypatch, mode_name):
    """The size and the means of tests/test_walk_trips_gpu.py (its docstring has the sizes): an engine with one workgroup
    per compute unit and 64 (2 W + 1) - 51 paths, W = cus x kW, at which every wave of cashflow_kernel's grid makes a
    second trip and one a third; the sweep's grid is an eighth of that one, so its waves make sixteen and more.  S = 8,
    ids that cross 2^32, against the restatement; the double sums against exact sums of the restatement's values."""
    import test_walk_trips_gpu as wt
    from stock_market_monte_carlo_amd import Engine
    mode, tab = wt._mode_table(mode_name, table)
    P = wt.PERIODS[mode_name]
    with wt._one_block_per_cu(monkeypatch, tab) as (eng, cus):
        n = wt._walk_sizes(cus, mode_name)[0]
        R = ref.returns(oracle, mode, tab, n, P, first_path=wt.FIRST, seed=wt.SEED)
        want = [ref.simulate(R, a, 0.0, wt.FLOOR) for a in TRIP_AMOUNTS]
        shares = [float((ruin > 0).mean()) for _, _, ruin, _ in want]
        print(f"{mode_name}: the restatement depletes {shares} of {n} paths")
        assert any(x == 0.0 for x in shares) and any(0.05 < x < 0.95 for x in shares) and shares[-1] == 1.0
        sim = Engine.make_sim(n, P, mode, wt.SEED, first_path=wt.FIRST, initial_capital=ref.CAPITAL, n_bins=BINS, hist_lo=LO,
                              hist_hi=HI, below_threshold=BELOW)
        out = _run(eng, sim, [(a, 0.0, wt.FLOOR) for a in TRIP_AMOUNTS])
        for s, (v, paid, ruin, _) in enumerate(want):
            _check_scenario(oracle, out, s, v, paid, ruin, P, (mode_name, n, s), sums=wt._exact_sums(v))


@pytest.mark.parametrize("P", [360, 7])
@pytest.mark.parametrize("mode_name", MODES)
def test_monotone_in_the_amount_on_the_device(engines, mode_name, P):
    """include/smmc.h's property on the device's own outputs: equal floor, fraction 0, amounts ascending."""
    eng, n = engines[mode_name], 4099
    out = _run(eng, _sim(mode_name, n, P), [(a, 0.0, ref.FLOOR) for a in AMOUNTS[P]])
    latest = np.where(out["ruin_period"] == 0, P + 1, out["ruin_period"]).astype(np.int64)
    assert (np.diff(out["final"], axis=0) <= 0).all() and (np.diff(latest, axis=0) <= 0).all()
    never = out["depleted_at"][:, 0].astype(np.int64)
    assert (np.diff(never) <= 0).all() and never[0] == n and never[-1] < n


def test_result_object(engines, oracle):
    from stock_market_monte_carlo_amd import SweepResult
    eng, n, P = engines["gaussian"], 4099, 360
    res = eng.simulate_cashflow_sweep(_sim("gaussian", n, P), AMOUNTS[360], floors=ref.FLOOR, want_final=True, want_stats=True)
    assert isinstance(res, SweepResult) and res.paid is None and res.ruin_period is None and tuple(res.final.shape) == (8, n)
    assert len(res.stats) == 8 and all(st.count == n for st in res.stats) and res.depleted_at.shape == (8, P + 1)
    ruins = [_reference(oracle, "gaussian", P, a, 0.0, ref.FLOOR)[2][:n] for a in AMOUNTS[360]]
    s = res.survival()
    assert s.shape == (8, P + 1) and (s[:, 0] == 1.0).all() and (np.diff(s, axis=1) <= 0).all()
    assert np.allclose(s[:, -1], [float((r == 0).mean()) for r in ruins]) and np.allclose(res.depleted_share(), 1.0 - s[:, -1])
    one = eng.simulate_cashflow(_sim("gaussian", n, P), amount=6.0, floor=ref.FLOOR)
    assert np.array_equal(s[5], one.survival())
    alive = [float((r == 0).mean()) for r in ruins]
    assert res.highest_surviving(0.95) == max(i for i, a in enumerate(alive) if a >= 0.95) == 4  # 5.0 survives with 0.99, 6.0 with 0.45
    assert res.highest_surviving(0.3) == 5 and res.highest_surviving(0.0) == 7
