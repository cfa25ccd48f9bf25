"""Allocation sweeps (smmc_engine_simulate_allocation_sweep) on the GPU against the restatement of the contract
(tests/allocation_sweep_reference.py): scenario s of a sweep is tests/portfolio_cashflow_reference.py's simulate with
(weights, R, amount, fraction, floor)[s] on the multipliers of tests/portfolio_reference.py.

Per scenario final, holdings, paid and ruin_period are compared on their bits, depleted_at exactly; of the statistics
record the integer fields, min, max and bucket counts with ==, the two double sums to the relative 1e-12 of
tests/test_gpu_parity.py against oracle.values_stats.  Capital 1000, first_path 2^32 - 100, 64 buckets on [0, 4000),
below-threshold 1000; n in 1, 255, 4099 and 2 * 4099 + 1; a dense table of 37 rows, a wide one of 2500, Gaussian mode; K = 1
.. 4.  The scenario sets are sized in the reference module and checked on the restatement alone in
tests/test_allocation_sweep_cpu.py.

On the commit before this feature every test here fails: the symbols do not exist.  The commit that added this file
could not run it on a device; the cases, bounds and references stand as the feature's issue states them.

Evidence that the tests see a kernel that confuses its scenarios: NOT MEASURED.  The build made wrong on purpose that
the feature's issue asks for (tools/variant_build.py, scenario 0's weights in the place of scenario sc's in
allocation_sweep_kernel's step) was not run against this file."""
import ctypes as C

import numpy as np
import pytest

import allocation_sweep_reference as ref
from test_allocation_sweep_cpu import LEDGER

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("allocation_sweep")

BINS, LO, HI, BELOW = ref.BINS, ref.LO, ref.HI, ref.BELOW
STATS = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
ALL = dict(want_final=True, want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
NONE = {k: False for k in ALL}
PER_PATH = ("final", "holdings", "paid", "ruin_period")
SENTINEL = 0x7FC0BEEF  # a NaN pattern as float32


def _gauss_args(shape, K):
    if shape != "gauss":
        return {}
    means, stds, corr = ref.gauss_setup(K)
    return {"means": means, "factor": ref.factor_of(stds, corr)}


@pytest.fixture(scope="module")
def engines():
    """One engine per shape, made on first use; table-mode engines have no single-series table unless a test sets one."""
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(shape, K):
        key = (shape, K if shape != "gauss" else 0)
        if key not in made:
            made[key] = S.Engine(0)
            if shape != "gauss":
                made[key].set_asset_table(ref.asset_table(int(shape[1:]), K))
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _sim(shape, n, P, first=0, exact_div=False, stats=True):
    import stock_market_monte_carlo_amd as S
    mode = S.MODE_GAUSSIAN if shape == "gauss" else S.MODE_TABLE
    return S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH + first, initial_capital=ref.CAPITAL, exact_div=exact_div,
                             **(STATS if stats else {}))


def _args(scenarios):
    return dict(weights=[sc[0] for sc in scenarios], rebalance_every=[sc[1] for sc in scenarios], amounts=[sc[2] for sc in scenarios],
                fractions=[sc[3] for sc in scenarios], floors=[sc[4] for sc in scenarios])


def _run(eng, sim, shape, K, scenarios, to_host=False, **want):
    """The outputs (all, or those named in want) as host arrays, scenario-major: final, paid (float32 [S, n]), holdings
    ([S, K, n]), ruin_period (uint32), stats_raw (S x bytes), depleted_at (uint64 [S, P + 1])."""
    full = dict(NONE, **want) if want else ALL
    rec = int(eng._L.smmc_stats_bytes(sim.n_bins))
    kw = dict(_args(scenarios), **_gauss_args(shape, K), **full)
    if to_host:
        out = eng.simulate_allocation_sweep_to_host(sim, **kw)
    else:
        raw = eng.simulate_allocation_sweep_raw(sim, **kw)
        eng.sync()
        out = {k: (t if t is None or isinstance(t, int) else t.cpu().numpy()) for k, t in raw.items()}
        if out["ruin_period"] is not None:
            out["ruin_period"] = out["ruin_period"].view(np.uint32)
        if out["depleted_at"] is not None:
            out["depleted_at"] = out["depleted_at"].view(np.uint64)
        if out["stats_raw"] is not None:
            out["stats_raw"] = out["stats_raw"].tobytes()
    assert out.pop("n_assets") == K
    if out["stats_raw"] is not None:
        assert len(out["stats_raw"]) == rec * len(scenarios)
        out["stats_raw"] = [out["stats_raw"][s * rec:(s + 1) * rec] for s in range(len(scenarios))]
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _record_fields(st):
    return (st.count, st.below, st.underflow, st.overflow, st.min, st.max)


def _check_scenario(oracle, out, s, want, P, tag, stats=True):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    n = want["final"].size
    assert out["final"].shape[1] == n and out["holdings"].shape[1:] == want["holdings"].shape, tag
    for key in ("final", "holdings", "paid"):
        assert np.array_equal(_bits(out[key][s]), _bits(want[key])), (tag, key)
    assert np.array_equal(out["ruin_period"][s], want["ruin_period"]), tag
    dep = out["depleted_at"][s]
    assert dep.size == P + 1 and int(dep.sum()) == n and np.array_equal(dep, want["depleted_at"]), tag
    if not stats:
        return
    st = stats_from_bytes(out["stats_raw"][s])
    ost, ohist = oracle.values_stats(want["final"], BELOW, BINS, LO, HI)
    assert st.count == ost.count == n, tag
    assert _record_fields(st)[1:] == (ost.below, ost.underflow, ost.overflow, ost.min, ost.max), tag
    assert np.array_equal(st.hist, ohist) and int(st.hist.sum()) + st.underflow + st.overflow == n, tag
    assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag


def _check_sweep(oracle, out, shape, K, scenarios, n, P, tag, stats=True):
    S = len(scenarios)
    assert out["final"].shape == out["paid"].shape == out["ruin_period"].shape == (S, n) and out["holdings"].shape == (S, K, n)
    assert out["depleted_at"].shape == (S, P + 1)
    for s, sc in enumerate(scenarios):
        _check_scenario(oracle, out, s, ref.cut(ref.reference(oracle, shape, K, P, sc), n), P, tag + (s,), stats)


# ---- parity with the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(LEDGER))
def test_every_instantiation_runs_once(engines, oracle, key):
    """The ledger of tests/test_allocation_sweep_cpu.py: 64 kW 2 + 37 paths, P = 9 (dense table) or 5."""
    from stock_market_monte_carlo_amd import _lib
    shape, K, P, S, exact = LEDGER[key]
    eng, n = engines(shape, K), 64 * (8 if shape == "gauss" else 4) * 2 + 37
    scenarios = ref.uniform_set(oracle, shape, K, P, S)
    sim = _sim(shape, n, P, exact_div=exact)
    kind = eng.allocation_sweep_divide_kind(sim, **_args(scenarios), **_gauss_args(shape, K))
    assert kind == (_lib.DIV_EXACT if exact else _lib.DIV_FAST), key  # the row reaches the instantiation it names
    _check_sweep(oracle, _run(eng, sim, shape, K, scenarios), shape, K, scenarios, n, P, key)


@pytest.mark.parametrize("shape,K,P,S,n", ref.PARITY_CASES)
def test_parity_with_the_restatement(engines, oracle, shape, K, P, S, n):
    scenarios = ref.uniform_set(oracle, shape, K, P, S)
    _check_sweep(oracle, _run(engines(shape, K), _sim(shape, n, P), shape, K, scenarios), shape, K, scenarios, n, P, (shape, K, P, S, n))


@pytest.mark.parametrize("shape,K,P,S,n", ref.LONG_CASES)
def test_a_thousand_periods_without_the_records(engines, oracle, shape, K, P, S, n):
    """5 x 1001 depletion counters fit SMMC_MAX_SWEEP_COUNTERS; with 64 buckets each they would still, with eight scenarios
    they would not."""
    from stock_market_monte_carlo_amd import SmmcError
    eng, scenarios = engines(shape, K), ref.uniform_set(oracle, shape, K, P, S)
    want = dict(ALL, want_stats=False)
    out = _run(eng, _sim(shape, n, P), shape, K, scenarios, **want)
    assert out["stats_raw"] is None
    _check_sweep(oracle, out, shape, K, scenarios, n, P, (shape, K, P), stats=False)
    eight = ref.uniform_set(oracle, shape, K, P, 8)
    counts = _run(eng, _sim(shape, n, P), shape, K, eight, want_depleted_at=True)
    assert (counts["depleted_at"].sum(axis=1) == n).all()
    with pytest.raises(SmmcError, match="SMMC_MAX_SWEEP_COUNTERS"):
        _run(eng, _sim(shape, n, P), shape, K, eight, want_stats=True, want_depleted_at=True)


@pytest.mark.parametrize("shape,K", ref.MIXED_CASES)
def test_mixed_scenarios_in_one_sweep(engines, oracle, shape, K):
    """Eight scenarios that differ in weights, R, amount, fraction and floor, one with a zero weight: a kernel that reads a
    neighbour's parameter, shares a countdown or an `alive` mask fails here."""
    n, P = 4099, 360
    mixed = ref.mixed_set(oracle, shape, K, P)
    _check_sweep(oracle, _run(engines(shape, K), _sim(shape, n, P), shape, K, mixed), shape, K, mixed, n, P, (shape, K, "mixed"))


# ---- a sweep is its single calls --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,K", ref.MIXED_CASES)
def test_a_sweep_is_its_single_calls(engines, oracle, shape, K):
    """Scenario s of a sweep against smmc_engine_simulate_portfolio_cashflow of that scenario from the same engine, on the
    bits the contract lists."""
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng, n, P = engines(shape, K), ref.N_MAX, 360
    sim, mixed = _sim(shape, n, P), ref.mixed_set(oracle, shape, K, P)
    out = _run(eng, sim, shape, K, mixed)
    for s, (w, R, am, fr, fl) in enumerate(mixed):
        raw = eng.simulate_portfolio_cashflow_raw(sim, w, R, am, fr, fl, want_final=True, want_holdings=True, want_paid=True,
                                                  want_ruin_period=True, want_stats=True, want_depleted_at=True, **_gauss_args(shape, K))
        eng.sync()
        one = {k: t.cpu().numpy() for k, t in raw.items() if k != "n_assets"}
        for key in PER_PATH:
            assert out[key][s].tobytes() == one[key].tobytes(), (s, key)
        assert np.array_equal(out["depleted_at"][s], one["depleted_at"].view(np.uint64)), s
        a, b = stats_from_bytes(out["stats_raw"][s]), stats_from_bytes(one["stats_raw"].tobytes())
        assert _record_fields(a) == _record_fields(b) and np.array_equal(a.hist, b.hist), s
        assert a.sum == pytest.approx(b.sum, rel=1e-12) and a.sumsq == pytest.approx(b.sumsq, rel=1e-12), s


@pytest.mark.parametrize("T", [37, 2500])
def test_a_sweep_with_one_asset_is_the_cash_flow_sweep_on_that_column(oracle, T):
    import stock_market_monte_carlo_amd as S
    shape, column, n, P = "t%d" % T, ref.asset_table(T, 1), 4099, 360
    scenarios = ref.mixed_set(oracle, shape, 1, P)
    eng = S.Engine(0)
    try:
        eng.set_table(column[:, 0])
        eng.set_asset_table(column)
        sim = _sim(shape, n, P)
        got = _run(eng, sim, shape, 1, scenarios)
        raw = eng.simulate_cashflow_sweep_raw(sim, [sc[2] for sc in scenarios], [sc[3] for sc in scenarios], [sc[4] for sc in scenarios],
                                              want_final=True, want_paid=True, want_ruin_period=True, want_depleted_at=True)
        eng.sync()
        for key in ("final", "paid", "ruin_period", "depleted_at"):
            assert got[key].tobytes() == raw[key].cpu().numpy().tobytes(), key
        assert got["holdings"][:, 0].tobytes() == got["final"].tobytes()
        assert 0 < int(got["depleted_at"][0, 0]) < n
    finally:
        eng.close()


# ---- padding ----------------------------------------------------------------------------------------------------------

def _same_outputs(a, b, tag=None):
    for k in PER_PATH + ("depleted_at",):
        assert (a[k] is None) == (b[k] is None), (tag, k)
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
    assert a["stats_raw"] == b["stats_raw"], tag


@pytest.mark.parametrize("shape,K", ref.MIXED_CASES)
@pytest.mark.parametrize("S", [3, 5])
def test_padding_leaks_nothing(engines, oracle, shape, K, S):
    """The padded widths: buffers one scenario larger than the request keep their sentinel beyond S, every depleted_at row
    sums to n, and a scenario's outputs depend neither on how many others the sweep holds nor on their order."""
    import torch
    from stock_market_monte_carlo_amd import _lib
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng, n, P = engines(shape, K), 4099, 360
    sim, mixed = _sim(shape, n, P), ref.mixed_set(oracle, shape, K, P)
    scenarios = mixed[:S]
    rec = int(eng._L.smmc_stats_bytes(BINS))
    pfs, cfs = eng.make_allocation_sweep(**_args(scenarios), **_gauss_args(shape, K))[:2]
    fill = lambda count, dtype: torch.full((S + 1, count), SENTINEL, dtype=dtype, device=eng.tdevice)  # noqa: E731
    bufs = {"final": fill(n, torch.int32), "holdings": fill(K * n, torch.int32), "paid": fill(n, torch.int32),
            "ruin_period": fill(n, torch.int32), "stats": fill(rec // 4, torch.int32), "depleted_at": fill(P + 1, torch.int64)}
    o = _lib.AllocationSweepOutputs()
    o.struct_size = C.sizeof(_lib.AllocationSweepOutputs)
    for name, t in bufs.items():
        setattr(o, name, t.data_ptr())
    cur = eng._enter()
    rc = eng._L.smmc_engine_simulate_allocation_sweep(eng._h, C.byref(sim), pfs, cfs, S, C.byref(o))
    assert rc == 0, eng._L.smmc_last_error()
    eng._leave(cur, *bufs.values())
    eng.sync()
    for t in bufs.values():
        assert (t[S].cpu().numpy() == SENTINEL).all()
    assert (bufs["depleted_at"][:S].cpu().numpy().sum(axis=1) == n).all()
    alone, whole = _run(eng, sim, shape, K, scenarios), _run(eng, sim, shape, K, mixed)
    back = _run(eng, sim, shape, K, mixed[::-1])  # the eight in reverse order: scenario s sits at 7 - s
    for key, name in (("final", "final"), ("holdings", "holdings"), ("paid", "paid"), ("ruin_period", "ruin_period"),
                      ("depleted_at", "depleted_at")):
        direct = bufs[name][:S].cpu().numpy().tobytes()
        assert direct == alone[key].tobytes() == whole[key][:S].tobytes() == back[key][::-1][:S].tobytes(), key
    host = bufs["stats"][:S].cpu().numpy().tobytes()
    assert [host[s * rec:(s + 1) * rec] for s in range(S)] == alone["stats_raw"]
    for s in range(S):  # another launch geometry: the integer fields and the buckets, not the order of the double sums
        a = stats_from_bytes(alone["stats_raw"][s])
        for b in (stats_from_bytes(whole["stats_raw"][s]), stats_from_bytes(back["stats_raw"][7 - s])):
            assert _record_fields(a) == _record_fields(b) and np.array_equal(a.hist, b.hist)
            assert a.sum == pytest.approx(b.sum, rel=1e-12) and a.sumsq == pytest.approx(b.sumsq, rel=1e-12)


# ---- other properties ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,K", ref.MIXED_CASES)
def test_divide_variants_give_the_same_bytes(engines, oracle, shape, K):
    """36 periods, at which the single call's rule proves the fast form for the seven scenarios that take an amount out."""
    from stock_market_monte_carlo_amd import _lib
    eng, n, P = engines(shape, K), 4099, 36
    seven = ref.uniform_set(oracle, shape, K, P, 8)[1:]
    g = _gauss_args(shape, K)
    assert eng.allocation_sweep_divide_kind(_sim(shape, n, P), **_args(seven), **g) == _lib.DIV_FAST
    assert eng.allocation_sweep_divide_kind(_sim(shape, n, P, exact_div=True), **_args(seven), **g) == _lib.DIV_EXACT
    with_fraction = seven[:3] + [(seven[3][0], 5, 0.0, 0.004, ref.FLOOR)]
    assert eng.allocation_sweep_divide_kind(_sim(shape, n, P), **_args(with_fraction), **g) == _lib.DIV_EXACT
    fast, exact = _run(eng, _sim(shape, n, P), shape, K, seven), _run(eng, _sim(shape, n, P, exact_div=True), shape, K, seven)
    _same_outputs(fast, exact, "seven")


@pytest.mark.parametrize("shape,K", [("t37", 3), ("gauss", 4)])
def test_each_output_alone_and_the_host_entry(engines, oracle, shape, K):
    eng, sim = engines(shape, K), _sim(shape, 4099, 360)
    mixed = ref.mixed_set(oracle, shape, K, 360)
    everything = _run(eng, sim, shape, K, mixed)
    _same_outputs(everything, _run(eng, sim, shape, K, mixed, to_host=True), "to_host")
    for want, key in (("want_final", "final"), ("want_holdings", "holdings"), ("want_paid", "paid"), ("want_ruin_period", "ruin_period"),
                      ("want_stats", "stats_raw"), ("want_depleted_at", "depleted_at")):
        for to_host in (False, True):
            alone = _run(eng, sim, shape, K, mixed, to_host=to_host, **{want: True})
            assert [k for k, x in alone.items() if x is not None] == [key], (want, to_host)
            got, all_ = alone[key], everything[key]
            assert (got == all_) if key == "stats_raw" else (got.tobytes() == all_.tobytes()), (want, to_host)


@pytest.mark.parametrize("shape,K", [("t2500", 2), ("gauss", 4)])
def test_identical_calls_give_identical_bytes(engines, oracle, shape, K):
    """... records included, also with other users of the engine's accumulator in between: it is left zero."""
    eng, mixed = engines(shape, K), ref.mixed_set(oracle, shape, K, 360)
    g = _gauss_args(shape, K)
    first = _run(eng, _sim(shape, 4099, 360), shape, K, mixed)
    _same_outputs(first, _run(eng, _sim(shape, 4099, 360), shape, K, mixed), "again")
    other = _run(eng, _sim(shape, ref.N_MAX, 36), shape, K, mixed[:5])
    eng.simulate_portfolio(_sim(shape, 1000, 360), mixed[0][0], 12, want_stats=True, **g)
    eng.simulate_portfolio_cashflow(_sim(shape, 1000, 360), mixed[0][0], 12, amount=6.0, floor=ref.FLOOR, want_stats=True, **g)
    _same_outputs(first, _run(eng, _sim(shape, 4099, 360), shape, K, mixed), "after other calls")
    _same_outputs(other, _run(eng, _sim(shape, ref.N_MAX, 36), shape, K, mixed[:5]), "the other call again")


@pytest.mark.parametrize("shape,K,S", [("gauss", 4, 8), ("t37", 3, 5), ("t2500", 2, 3)])
def test_shards_of_one_request_merge(engines, oracle, shape, K, S):
    """Split at an odd boundary into two sweeps with shifted first_path: the per-path outputs concatenate, the records
    merge by smmc_stats_merge, the depletion counts add, scenario by scenario."""
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes, stats_from_bytes
    eng, n, P, cut = engines(shape, K), 4099, 360, 1531
    scenarios = ref.mixed_set(oracle, shape, K, P)[:S]
    whole = _run(eng, _sim(shape, n, P), shape, K, scenarios)
    a = _run(eng, _sim(shape, cut, P), shape, K, scenarios)
    b = _run(eng, _sim(shape, n - cut, P, first=cut), shape, K, scenarios)
    for k in PER_PATH:
        assert np.concatenate([a[k], b[k]], axis=-1).tobytes() == whole[k].tobytes(), k
    assert np.array_equal(a["depleted_at"] + b["depleted_at"], whole["depleted_at"])
    for s in range(S):
        m, w = stats_from_bytes(merge_stats_bytes([a["stats_raw"][s], b["stats_raw"][s]])), stats_from_bytes(whole["stats_raw"][s])
        assert _record_fields(m) == _record_fields(w) and np.array_equal(m.hist, w.hist)
        assert m.sum == pytest.approx(w.sum, rel=1e-12) and m.sumsq == pytest.approx(w.sumsq, rel=1e-12)


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_outputs_when_waves_make_several_trips(oracle, table, monkeypatch, mode_name):
    """The helpers of tests/test_walk_trips_gpu.py as tests/test_sweep_gpu.py uses them: an engine with one workgroup per
    compute unit and 64 (2 W + 1) - 51 paths, W = cus x kW; the sweep's grid is an eighth of the single call's, so every
    wave makes sixteen trips and more.  S = 8, K = 2, ids that cross 2^32, against the restatement on those paths."""
    import portfolio_cashflow_reference as pcref
    import portfolio_reference as pref
    import test_walk_trips_gpu as wt
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN, MODE_TABLE
    shape, K = ("gauss", 2) if mode_name == "gaussian" else ("t37", 2)
    P = wt.PERIODS[mode_name]
    with wt._one_block_per_cu(monkeypatch) as (eng, cus):
        n = wt._walk_sizes(cus, mode_name)[0]
        if shape == "gauss":
            means, stds, corr = ref.gauss_setup(K)
            a = pref.gauss_multipliers(oracle, means, ref.factor_of(stds, corr), wt.SEED, wt.FIRST, n, P)
        else:
            eng.set_asset_table(ref.asset_table(37, K))
            a = pref.table_multipliers(oracle, ref.asset_table(37, K), wt.SEED, wt.FIRST, n, P)
        m = float(np.median(pcref.simulate(a[:2000], ref.WEIGHT_SETS[K][0], 0)["final"])) / ref.CAPITAL
        lv = ref.CAPITAL * m * (m ** (1.0 / P) - 1.0) / (m - 1.0)
        scenarios = [(ref.WEIGHT_SETS[K][i], ref.REBALANCE[i], float(np.float32(ref.MULTIPLES[i] * lv)), 0.0, ref.FLOOR) for i in range(8)]
        want = ref.simulate(a, scenarios)
        shares = [float((w["ruin_period"] > 0).mean()) for w in want]
        print(f"{mode_name}: the restatement depletes {shares} of {n} paths")
        assert any(x == 0.0 for x in shares) and any(0.05 < x < 0.95 for x in shares)
        sim = Engine.make_sim(n, P, MODE_GAUSSIAN if shape == "gauss" else MODE_TABLE, wt.SEED, first_path=wt.FIRST,
                              initial_capital=ref.CAPITAL, **STATS)
        out = _run(eng, sim, shape, K, scenarios)
        for s, w in enumerate(want):
            _check_scenario(oracle, out, s, w, P, (mode_name, n, s))


def test_result_object(engines, oracle):
    from stock_market_monte_carlo_amd import AllocationSweepResult, SweepResult
    shape, K, n, P = "gauss", 4, 4099, 360
    eng, mixed = engines(shape, K), ref.mixed_set(oracle, shape, K, P)
    res = eng.simulate_allocation_sweep(_sim(shape, n, P), **_args(mixed), **_gauss_args(shape, K), want_holdings=True, want_stats=True)
    assert isinstance(res, AllocationSweepResult) and isinstance(res, SweepResult) and res.final is None and res.paid is None
    assert tuple(res.holdings.shape) == (8, K, n) and res.n_assets == K and res.weights.shape == (8, K)
    assert len(res.stats) == 8 and all(st.count == n for st in res.stats) and res.depleted_at.shape == (8, P + 1)
    alive = [float((ref.reference(oracle, shape, K, P, sc)["ruin_period"][:n] == 0).mean()) for sc in mixed]
    s = res.survival()
    assert s.shape == (8, P + 1) and (s[:, 0] == 1.0).all() and (np.diff(s, axis=1) <= 0).all()
    assert np.allclose(s[:, -1], alive) and np.allclose(res.depleted_share(), 1.0 - s[:, -1])
    assert res.surviving(0.95) == [i for i, x in enumerate(alive) if x >= 0.95] and 1 in res.surviving(0.95)
    assert len(res.surviving(0.95)) < 8 and res.surviving(0.0) == list(range(8))
