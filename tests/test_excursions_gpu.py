"""Excursion statistics (smmc_engine_simulate_excursions) on the GPU against the numpy float32 restatement of
include/smmc.h's arithmetic over the CPU oracle's trajectories (tests/excursions_reference.py).

The eight per-path outputs are compared on their bits, the two count arrays exactly; of both records the integer
fields, min, max and bucket counts with ==, the two double sums to the relative 1e-12 of tests/test_gpu_parity.py
(the device adds in another order).  Capital 1000, Gaussian 0.6 +- 4.3 %, first_path 3 throughout; levels
(950, 1050) at 7 periods and (800, 2000) at 360 and 1000.  On 8199 paths the restatement has 0.39 / 0.64 (Gaussian)
and 0.41 / 0.61 (bundled table) ever below / reached at 7 periods, 0.26 / 0.96 and 0.30 / 0.93 at 360, 0.26 / 1.00 and
0.30 / 0.999 at 1000 (tests/test_excursions_cpu.py asserts these); for the 3001-entry table the fractions are printed
and only parity is asserted."""
import numpy as np
import pytest

import excursions_reference as ref

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("excursions")

N_MAX = ref.N_MAX
PATHS = [1, 255, 4099, N_MAX]   # one path; a partial wave; a ragged last chunk; past one workgroup walk
PERIODS = [7, 360, 1000]        # below one Philox block; a multiple of 8 and of 4; neither
MODES = ["gaussian", "table", "table3001"]
BINS, LO, HI, BELOW = 64, 0.0, 4000.0, 500.0
PER_PATH = ref.FIELDS
COUNTS = ("first_below_at", "first_reach_at")
RECORDS = ("stats", "drawdown_stats")
ALL = PER_PATH + RECORDS + COUNTS


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


def _sim(mode_name, n, P, first=ref.FIRST_PATH, exact_div=False, n_bins=BINS):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(n, P, _mode(mode_name)[0], ref.SEED, first_path=first, initial_capital=ref.CAPITAL,
                             gauss_mean=ref.GAUSS_MEAN, gauss_std=ref.GAUSS_STD, n_bins=n_bins, hist_lo=LO, hist_hi=HI,
                             below_threshold=BELOW, exact_div=exact_div)


def _run(eng, sim, levels=None, to_host=False, only=None):
    """All outputs (or those named in only) as host arrays: float32 / uint32 per path, bytes for the two records,
    uint64 count arrays; None for the others."""
    lower, target = levels if levels is not None else ref.levels(int(sim.n_periods))
    wants = {"want_" + k: (only is None or k in only) for k in ALL}
    if to_host:
        return eng.simulate_excursions_to_host(sim, lower, target, ref.DD_THRESHOLD, **wants)
    raw = eng.simulate_excursions_raw(sim, lower, target, ref.DD_THRESHOLD, **wants)
    eng.sync()
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in raw.items()}
    for k in ("drawdown_period", "underwater", "first_below", "first_reach"):
        if out[k] is not None:
            out[k] = out[k].view(np.uint32)
    for k in COUNTS:
        if out[k] is not None:
            out[k] = out[k].view(np.uint64)
    for k in RECORDS:
        if out[k] is not None:
            out[k] = out[k].tobytes()
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_record(oracle, raw, values, below, lo, hi, n_bins, tag):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    st = stats_from_bytes(raw)
    ost, ohist = oracle.values_stats(values, below, n_bins, lo, hi)
    n = values.size
    assert st.count == ost.count == n, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert st.min == ost.min and st.max == ost.max, tag
    assert np.array_equal(st.hist, ohist), tag
    if n_bins:
        assert int(st.hist.sum()) + st.underflow + st.overflow == n, tag
    assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag


def _check_against(oracle, out, want, n, P, tag, n_bins=BINS):
    for k in PER_PATH:
        assert np.array_equal(_bits(out[k]), _bits(want[k][:n])), (tag, k)
    for k, per_path in zip(COUNTS, ("first_below", "first_reach")):
        assert out[k].size == P + 1 and int(out[k].sum()) == n, (tag, k)
        assert np.array_equal(out[k], np.bincount(want[per_path][:n], minlength=P + 1).astype(np.uint64)), (tag, k)
    _check_record(oracle, out["stats"], want["final"][:n], BELOW, LO, HI, n_bins, (tag, "stats"))
    _check_record(oracle, out["drawdown_stats"], want["drawdown"][:n], ref.DD_THRESHOLD, 0.0, 1.0, n_bins, (tag, "drawdown_stats"))


@pytest.mark.parametrize("n", PATHS)
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("mode_name", MODES)
def test_parity_with_the_restatement(engines, oracle, mode_name, P, n):
    mode, key = _mode(mode_name)
    want = ref.cached_excursions(oracle, mode, key, P)
    below, reach = int((want["first_below"] > 0).sum()), int((want["first_reach"] > 0).sum())
    print(f"{mode_name} P={P}: the restatement has {below} ever below, {reach} reached, of {N_MAX}; "
          f"median drawdown {float(np.median(want['drawdown'])):.3f}")
    if mode_name != "table3001":  # a degenerate input must not hide a kernel bug
        assert 0 < below < N_MAX and 0 < reach
        if not (mode_name == "gaussian" and P == 1000):
            assert reach < N_MAX
    out = _run(engines[mode_name], _sim(mode_name, n, P))
    _check_against(oracle, out, want, n, P, (mode_name, P, n))


@pytest.mark.parametrize("mode_name", MODES)
def test_final_values_are_the_plain_simulation(engines, mode_name):
    """final is bit-identical to Engine.simulate for the same sim, and the stats record's integer fields equal its."""
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng, sim = engines[mode_name], _sim(mode_name, N_MAX, 360)
    plain = eng.simulate(sim, want_stats=True)
    pst = eng.read_stats(plain.stats_raw)
    out = _run(eng, sim, only=("final", "stats"))
    assert np.array_equal(_bits(out["final"]), _bits(plain.final.cpu().numpy()))
    st = stats_from_bytes(out["stats"])
    assert (st.count, st.below, st.underflow, st.overflow, st.min, st.max) == (pst.count, pst.below, pst.underflow, pst.overflow,
                                                                              pst.min, pst.max)
    assert np.array_equal(st.hist, pst.hist)


def _same_outputs(a, b, tag=None):
    for k in ALL:
        assert (a[k] is None) == (b[k] is None), (tag, k)
        if a[k] is None:
            continue
        if k in RECORDS:
            assert a[k] == b[k], (tag, k)
        else:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)


@pytest.mark.parametrize("mode_name, P", [("gaussian", 120), ("table", 360)])
def test_exact_div_gives_the_same_bytes(engines, mode_name, P):
    """Shapes for which the fast divide is proven, so that the two calls run the two variants.  The bundled table
    (-15.1 .. +14.3 %) is at 360 periods.  Gaussian 0.6 +- 4.3 % is bounded by 100.6 +- 7 * 4.3: 1.307^360 * 1000 is
    beyond 2^127, so the default is already the IEEE divide there (the parity grid covers it), and the proof holds up to
    194 periods (0.705^P * 1000 > 2^-88); 120 is a multiple of 8 well inside."""
    from stock_market_monte_carlo_amd import _lib
    eng = engines[mode_name]
    assert eng.divide_kind(_sim(mode_name, 4099, P), keepdata=True) == _lib.DIV_FAST
    assert eng.divide_kind(_sim(mode_name, 4099, P, exact_div=True), keepdata=True) == _lib.DIV_EXACT
    _same_outputs(_run(eng, _sim(mode_name, 4099, P)), _run(eng, _sim(mode_name, 4099, P, exact_div=True)))


def test_a_table_the_fast_divide_is_not_proven_for(oracle, table):
    """+42.2 % and -29.7 % planted (the values tests/test_gpu_parity.py plants): the keepdata rule says EXACT, and
    parity with the oracle's trajectories holds."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import _lib
    real = table.copy()
    real[7], real[100] = 42.2, -29.7
    eng = S.Engine(0)
    try:
        eng.set_table(real)
        n, P = 4099, 360
        sim = _sim("table", n, P)
        assert eng.divide_kind(sim, keepdata=True) == _lib.DIV_EXACT
        want = ref.excursions(ref.trajectories(oracle, S.MODE_TABLE, real, n, P), *ref.levels(P))
        assert 0 < int((want["first_below"] > 0).sum()) < n
        _check_against(oracle, _run(eng, sim), want, n, P, "planted")
    finally:
        eng.close()


def test_a_table_with_a_nan_entry(oracle, table):
    """Every comparison is false for NaN: a path that draws the entry keeps its extremes, drawdown and first
    passages from before, and its final value is NaN.  NaN payloads are not part of any contract: the float outputs
    are compared on their bits where they are numbers and on being NaN where they are not."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    bad = table.copy()
    bad[11] = np.nan
    eng = S.Engine(0)
    try:
        eng.set_table(bad)
        n, P = 4099, 7
        sim = _sim("table", n, P)
        want = ref.excursions(ref.trajectories(oracle, S.MODE_TABLE, bad, n, P), *ref.levels(P))
        hit = np.isnan(want["final"])
        print(f"{int(hit.sum())} of {n} paths draw the NaN entry")
        assert 0 < int(hit.sum()) < n
        out = _run(eng, sim)
        for k in ("final", "peak", "low", "drawdown"):
            nan = np.isnan(want[k])
            assert np.array_equal(np.isnan(out[k]), nan), k
            assert np.array_equal(_bits(out[k])[~nan], _bits(want[k])[~nan]), k
        assert not np.isnan(want["peak"]).any() and not np.isnan(want["drawdown"]).any()
        for k in ("drawdown_period", "underwater", "first_below", "first_reach"):
            assert np.array_equal(out[k], want[k]), k
        for k in COUNTS:
            assert np.array_equal(out[k], want[k]), k
        _check_record(oracle, out["drawdown_stats"], want["drawdown"], ref.DD_THRESHOLD, 0.0, 1.0, BINS, "drawdown_stats")
        st = stats_from_bytes(out["stats"])  # the NaN finals: counted, beyond the buckets, not in min / max
        ost, ohist = oracle.values_stats(want["final"], BELOW, BINS, LO, HI)
        assert (st.count, st.below, st.underflow, st.overflow) == (ost.count, ost.below, ost.underflow, ost.overflow)
        assert st.overflow >= int(hit.sum()) and np.array_equal(st.hist, ohist) and np.isnan(st.sum)
        assert st.min == ost.min and st.max == ost.max
    finally:
        eng.close()


@pytest.mark.parametrize("mode_name", MODES)
def test_shards_of_one_request_merge(engines, mode_name):
    """8199 paths from a global id just below 2^32, as 3 unequal shards, the last of which starts above 2^32: the
    per-path outputs are the unsharded run's slices, the count arrays add, the records merge by smmc_stats_merge."""
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes, stats_from_bytes
    eng, n, P = engines[mode_name], N_MAX, 360
    first = (1 << 32) - 5000
    cuts = [0, 1531, 5000 + 77, n]
    assert first + cuts[2] > (1 << 32) > first + cuts[1]
    whole = _run(eng, _sim(mode_name, n, P, first=first))
    parts = [_run(eng, _sim(mode_name, cuts[i + 1] - cuts[i], P, first=first + cuts[i])) for i in range(3)]
    for k in PER_PATH:
        assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes(), k
    for k in COUNTS:
        assert np.array_equal(parts[0][k] + parts[1][k] + parts[2][k], whole[k]), k
    for k in RECORDS:
        m, w = stats_from_bytes(merge_stats_bytes([p[k] for p in parts])), stats_from_bytes(whole[k])
        assert (m.count, m.below, m.underflow, m.overflow, m.min, m.max) == (w.count, w.below, w.underflow, w.overflow, w.min, w.max), k
        assert np.array_equal(m.hist, w.hist), k
        assert m.sum == pytest.approx(w.sum, rel=1e-12) and m.sumsq == pytest.approx(w.sumsq, rel=1e-12), k


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_identical_calls_give_identical_bytes(engines, mode_name):
    """... double sums included, also with other users of the engine's accumulator in between: it is left zero."""
    eng = engines[mode_name]
    first = _run(eng, _sim(mode_name, N_MAX, 360))
    _same_outputs(first, _run(eng, _sim(mode_name, N_MAX, 360)), "again")
    other = _run(eng, _sim(mode_name, 4099, 1000))
    eng.simulate(_sim(mode_name, 1000, 360), want_stats=True)
    eng.simulate_cashflow(_sim(mode_name, 1000, 360), amount=6.0, floor=0.01, want_stats=True)
    _same_outputs(first, _run(eng, _sim(mode_name, N_MAX, 360)), "after other calls")
    _same_outputs(other, _run(eng, _sim(mode_name, 4099, 1000)), "the other call again")


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_each_output_alone_and_the_host_entry(engines, mode_name):
    eng, sim = engines[mode_name], _sim(mode_name, 4099, 360)
    everything = _run(eng, sim)
    _same_outputs(everything, _run(eng, sim, to_host=True), "to_host")
    for key in ALL:
        alone = _run(eng, sim, only=(key,))
        assert [k for k, x in alone.items() if x is not None] == [key], key
        got, all_ = alone[key], everything[key]
        assert (got == all_) if key in RECORDS else (got.tobytes() == all_.tobytes()), key


def test_without_buckets(engines, oracle):
    """n_bins = 0: both records are their headers, everything else as with buckets."""
    eng = engines["gaussian"]
    want = ref.cached_excursions(oracle, 1, "none", 360)
    out = _run(eng, _sim("gaussian", 4099, 360, n_bins=0))
    assert len(out["stats"]) == len(out["drawdown_stats"]) == 64
    _check_against(oracle, out, want, 4099, 360, "n_bins = 0", n_bins=0)


def test_result_object(engines, oracle):
    eng = engines["gaussian"]
    want = ref.cached_excursions(oracle, 1, "none", 360)
    res = eng.simulate_excursions(_sim("gaussian", 4099, 360), 800.0, 2000.0, want_drawdown=True, want_stats=True)
    assert res.peak is None and res.first_below is None and res.stats.count == 4099 == res.drawdown_stats.count
    assert np.array_equal(_bits(res.final.cpu().numpy()), _bits(want["final"][:4099]))
    assert np.array_equal(_bits(res.drawdown.cpu().numpy()), _bits(want["drawdown"][:4099]))
    assert res.drawdown_stats.below == int((want["drawdown"][:4099] < np.float32(0.2)).sum())
    assert (res.drawdown_stats.hist_lo, res.drawdown_stats.hist_hi) == (0.0, 1.0)
    eb, rb = res.ever_below(), res.reached_by()
    assert eb.size == rb.size == 361 and eb[0] == rb[0] == 0.0 and np.all(np.diff(eb) >= 0) and np.all(np.diff(rb) >= 0)
    assert eb[-1] == pytest.approx(float((want["first_below"][:4099] > 0).mean()))
    assert rb[120] == pytest.approx(float(((want["first_reach"][:4099] > 0) & (want["first_reach"][:4099] <= 120)).mean()))
    with pytest.raises(TypeError):
        eng.simulate_excursions(_sim("gaussian", 64, 7), 800.0, 2000.0, want_nothing=True)


def test_infinite_levels(engines):
    eng, sim = engines["table"], _sim("table", 255, 360)
    never = _run(eng, sim, levels=(-np.inf, np.inf))
    assert not never["first_below"].any() and not never["first_reach"].any()
    assert int(never["first_below_at"][0]) == 255 == int(never["first_reach_at"][0])
    always = _run(eng, sim, levels=(np.inf, -np.inf))
    assert (always["first_below"] == 1).all() and (always["first_reach"] == 1).all()
    assert int(always["first_below_at"][1]) == 255 == int(always["first_reach_at"][1])


def test_period_limits(engines, oracle, table):
    from stock_market_monte_carlo_amd import MAX_EXCURSION_PERIODS, MODE_TABLE, SmmcError
    eng = engines["table"]
    for P in (1, MAX_EXCURSION_PERIODS):
        want = ref.excursions(ref.trajectories(oracle, MODE_TABLE, table, 255, P), *ref.levels(P))
        _check_against(oracle, _run(eng, _sim("table", 255, P)), want, 255, P, ("limits", P))
    with pytest.raises(SmmcError, match="SMMC_MAX_EXCURSION_PERIODS"):
        _run(eng, _sim("table", 255, MAX_EXCURSION_PERIODS + 1))
