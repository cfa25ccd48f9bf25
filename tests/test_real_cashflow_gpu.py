"""smmc_engine_simulate_real_cashflow on the device against the numpy restatement of its contract
(tests/real_cashflow_reference.py): nominal final values, real final values, price indices, holdings, totals paid,
periods of depletion and the depletion counts on their bits; of the record (of the REAL final values) the integer
counters, buckets, min and max on their bits, the two double sums to the relative 1e-12 of tests/test_gpu_parity.py.

Shapes: a joint table of 37 rows with K = 1 .. 3 invested assets and the inflation column, one of 2500 rows x (2 + 1)
and Gaussian mode with K = 1 .. 3; path ids from 2^32 - 100 on; 64 kW 2 + 37 paths with kW = 4 (table) or 8 (Gaussian);
P in 1, 7, 8, 9 and 41 (table) or 38 (Gaussian); R in 0, 1, 5, 12; the parent's four schedules in money of period 0
(tests/test_real_cashflow_cpu.py checks that each depletes between 10 % and 90 % of the paths at the longest P).

The three identities of include/smmc.h are checked against smmc_engine_simulate_portfolio_cashflow ON THE DEVICE.  The
ledger of tests/real_cashflow_matrix.py is run row by row with the host's divide kind asserted.  The later walk trips run
in a fresh child process with SMMC_BLOCKS_PER_CU=1, sized as in tests/test_portfolio_cashflow_gpu.py.

On the commit before this feature every test here fails: the symbols do not exist."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import real_cashflow_matrix as RM
import real_cashflow_reference as ref

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("real_cashflow")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, LO, HI, BELOW = ref.BINS, ref.LO, ref.HI, ref.BELOW
STATS = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
ALL = dict(want_final=True, want_final_real=True, want_index=True, want_holdings=True, want_paid=True, want_ruin_period=True,
           want_stats=True, want_depleted_at=True)
PARENT_ALL = dict(want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
KEYS = ("final", "final_real", "index", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at")
NOMINAL = ("final", "holdings", "paid", "ruin_period", "depleted_at")
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gauss_args(shape, K):
    if shape != "gauss":
        return {}
    means, factor = ref.gauss_law(K)
    return {"means": means, "factor": factor}


@pytest.fixture(scope="module")
def engines():
    """One engine per shape, made on first use."""
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(shape, K):
        key = (shape, K if shape != "gauss" else 0)
        if key not in made:
            made[key] = S.Engine(0)
            if shape != "gauss":
                made[key].set_asset_table(ref.joint_table(int(shape[1:]), K))
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _sim(shape, n, P, first=0, **kw):
    import stock_market_monte_carlo_amd as S
    mode = S.MODE_GAUSSIAN if shape == "gauss" else S.MODE_TABLE
    return S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH + first, initial_capital=ref.CAPITAL, **kw)


def _same_floats(got, want, tag):
    """On the bits, NaN matching NaN (the payload of an invalid operation is the machine's own)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), tag
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), tag


def _fsum(values):
    try:
        return math.fsum(values)
    except (ValueError, OverflowError):  # inf - inf; a sum beyond binary64
        return float(np.sum(np.asarray(values, dtype=np.float64)))


def _same_sum(got, want, tag):
    if math.isfinite(want):
        assert got == pytest.approx(want, rel=1e-12), tag
    else:
        assert (math.isnan(got) and math.isnan(want)) or got == want, (tag, got, want)


def _check_record(oracle, st, values, tag, stats_range=(BINS, LO, HI, BELOW)):
    bins, lo, hi, below = stats_range
    values = np.ascontiguousarray(values, dtype=np.float32)
    ost, ohist = oracle.values_stats(values, below, bins, lo, hi)
    assert st.count == ost.count == values.size, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    _same_floats([st.min, st.max], [ost.min, ost.max], tag)
    assert np.array_equal(st.hist, ohist) and (not bins or int(st.hist.sum()) + st.underflow + st.overflow == values.size), tag
    d = values.astype(np.float64)
    with np.errstate(all="ignore"):
        _same_sum(st.sum, _fsum(d.tolist()), tag)
        _same_sum(st.sumsq, _fsum((d * d).tolist()), tag)


def _check_outputs(out, want, tag):
    """out: numpy arrays by key (ruin_period and depleted_at as the engine's signed tensors or as unsigned arrays)."""
    for key in ("final", "final_real", "index", "paid"):
        _same_floats(out[key], want[key], (tag, key))
    assert out["holdings"].shape == want["holdings"].shape, tag
    _same_floats(out["holdings"], want["holdings"], (tag, "holdings"))
    assert np.array_equal(out["ruin_period"].view(np.uint32), want["ruin_period"]), tag
    dep = out["depleted_at"].view(np.uint64)
    assert np.array_equal(dep, want["depleted_at"]) and int(dep.sum()) == want["final"].size, tag


def _numpy(raw):
    return {k: t.cpu().numpy() for k, t in raw.items() if k != "n_assets" and t is not None}


# 1
@pytest.mark.parametrize("shape,K", ref.SHAPES)
def test_outputs_bit_for_bit(oracle, engines, shape, K):
    """Every schedule, R and P, block boundaries and the partial block included."""
    eng, n, weights = engines(shape, K), ref.n_paths(shape), ref.WEIGHTS[K]
    sched = ref.schedules(oracle, shape, K, weights)
    wants = {k: v for k, v in ALL.items() if k != "want_stats"}
    for name in ref.SCHEDULES:
        for R in ref.REBALANCE:
            for P in ref.periods(shape):
                want = ref.reference(oracle, shape, K, weights, R, name, P)
                raw = eng.simulate_real_cashflow_raw(_sim(shape, n, P), weights, R, **ref.cut(sched[name], P), **wants, **_gauss_args(shape, K))
                eng.sync()
                _check_outputs(_numpy(raw), want, (shape, K, name, R, P))


# 2
@pytest.mark.parametrize("shape,K,name", [("t37", 3, "amount"), ("t2500", 2, "varying"), ("gauss", 3, "floor")])
def test_the_record_is_of_the_real_final_values(oracle, engines, shape, K, name):
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    want = ref.reference(oracle, shape, K, ref.WEIGHTS[K], 12, name, P)
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)
    r = eng.simulate_real_cashflow(_sim(shape, n, P, **STATS), ref.WEIGHTS[K], 12, want_final=False, want_final_real=False,
                                   want_stats=True, **kw, **_gauss_args(shape, K))
    assert r.final is None and r.final_real is None and r.index is None and r.holdings is None and r.paid is None
    assert not np.array_equal(_bits(want["final_real"]), _bits(want["final"]))
    _check_record(oracle, r.stats, want["final_real"], (shape, K, name))
    assert np.array_equal(r.depleted_at, want["depleted_at"])
    assert r.survival()[-1] == pytest.approx(want["depleted_at"][0] / n)


def _parent_equal(got, parent, tag, record=True):
    for key in NOMINAL:
        assert got[key].tobytes() == parent[key].tobytes(), (tag, key)
    if record:
        assert got["stats_raw"].tobytes() == parent["stats_raw"].tobytes(), (tag, "stats_raw")


# 3
@pytest.mark.parametrize("T,K", [(37, 1), (37, 3), (2500, 2)])
@pytest.mark.parametrize("name", ["amount", "varying"])
def test_identity_1_a_zero_inflation_column_is_the_parent_call(oracle, T, K, name):
    import stock_market_monte_carlo_amd as S
    shape = "t%d" % T
    n, P, w = ref.n_paths(shape), ref.longest(shape), ref.WEIGHTS[K]
    table = ref.joint_table(T, K).copy()
    table[:, K] = 0.0
    kw = ref.schedules(oracle, shape, K, w)[name]
    eng = S.Engine(0)
    try:
        for R in (0, 5):
            eng.set_asset_table(table)
            got = _numpy(eng.simulate_real_cashflow_raw(_sim(shape, n, P, **STATS), w, R, **ALL, **kw))
            eng.set_asset_table(np.ascontiguousarray(table[:, :K]))
            parent = _numpy(eng.simulate_portfolio_cashflow_raw(_sim(shape, n, P, **STATS), w, R, **PARENT_ALL, **kw))
            assert 0 < int(parent["depleted_at"][0]) < n
            _parent_equal(got, parent, (shape, K, name, R))
            assert got["final_real"].tobytes() == got["final"].tobytes() and (got["index"] == 1.0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("K", [1, 2, 3])
def test_identity_1_a_zero_gaussian_row_is_the_parent_call(oracle, engines, K):
    eng, n, P, w = engines("gauss", K), ref.n_paths("gauss"), ref.longest("gauss"), ref.WEIGHTS[K]
    means, factor = ref.gauss_law(K)
    means, factor = list(means), factor.copy()
    means[K] = 0.0
    factor[K, :] = 0.0
    kw = ref.schedules(oracle, "gauss", K, w)["floor"]
    for R in (0, 12):
        got = _numpy(eng.simulate_real_cashflow_raw(_sim("gauss", n, P, **STATS), w, R, **ALL, **kw, means=means, factor=factor))
        parent = _numpy(eng.simulate_portfolio_cashflow_raw(_sim("gauss", n, P, **STATS), w, R, **PARENT_ALL, **kw, means=means[:K],
                                                            factor=np.ascontiguousarray(factor[:K, :K])))
        assert 0 < int(parent["depleted_at"][0]) < n
        _parent_equal(got, parent, (K, R))
        assert got["final_real"].tobytes() == got["final"].tobytes() and (got["index"] == 1.0).all()


# 4
@pytest.mark.parametrize("shape,K", [("t37", 2), ("t2500", 2), ("gauss", 3)])
def test_identity_2_without_amount_and_floor_the_nominal_outputs_are_the_parents(oracle, shape, K):
    import stock_market_monte_carlo_amd as S
    n, P, w = ref.n_paths(shape), ref.longest(shape), ref.WEIGHTS[K]
    frac = np.where(np.arange(P) % 3 == 0, 0.0, 0.02).astype(f32)
    g = _gauss_args(shape, K)
    gp = {"means": g["means"][:K], "factor": np.ascontiguousarray(g["factor"][:K, :K])} if g else {}
    eng = S.Engine(0)
    try:
        for R, kw in ((0, dict(fraction=0.03)), (5, dict(fractions=frac))):
            if shape != "gauss":
                eng.set_asset_table(ref.joint_table(int(shape[1:]), K))
            got = _numpy(eng.simulate_real_cashflow_raw(_sim(shape, n, P), w, R, **{**ALL, "want_stats": False}, **kw, **g))
            if shape != "gauss":
                eng.set_asset_table(np.ascontiguousarray(ref.joint_table(int(shape[1:]), K)[:, :K]))
            parent = _numpy(eng.simulate_portfolio_cashflow_raw(_sim(shape, n, P), w, R, **{**PARENT_ALL, "want_stats": False}, **kw, **gp))
            _parent_equal(got, parent, (shape, K, R), record=False)
            assert np.unique(got["index"]).size > n // 2 and got["final_real"].tobytes() != got["final"].tobytes()
    finally:
        eng.close()


# 5
@pytest.mark.parametrize("T,K", [(37, 1), (37, 3), (2500, 2)])
def test_identity_3_a_constant_inflation_column_is_the_parents_amounts_array(oracle, T, K):
    """0.3 % every month and floor 0: the parent call with amounts[t - 1] = fl(amount * I_t)."""
    import stock_market_monte_carlo_amd as S
    shape = "t%d" % T
    n, P, w = ref.n_paths(shape), ref.longest(shape), ref.WEIGHTS[K]
    table = ref.joint_table(T, K).copy()
    table[:, K] = f32(0.3)
    index = np.ones(P + 1, f32)
    for t in range(1, P + 1):
        index[t] = (index[t - 1] * (f32(100.0) + f32(0.3))) / f32(100.0)
    amount = f32(ref.schedules(oracle, shape, K, w)["amount"]["amount"])
    eng = S.Engine(0)
    try:
        for R in (0, 5):
            eng.set_asset_table(table)
            got = _numpy(eng.simulate_real_cashflow_raw(_sim(shape, n, P), w, R, **{**ALL, "want_stats": False}, amount=float(amount), fraction=0.001))
            eng.set_asset_table(np.ascontiguousarray(table[:, :K]))
            parent = _numpy(eng.simulate_portfolio_cashflow_raw(_sim(shape, n, P), w, R, **{**PARENT_ALL, "want_stats": False},
                                                                amounts=(amount * index[1:]).astype(f32), fraction=0.001))
            assert 0 < int(parent["depleted_at"][0]) < n
            _parent_equal(got, parent, (shape, K, R), record=False)
            assert (_bits(got["index"]) == _bits(index[P:])).all()
    finally:
        eng.close()


# 6
@pytest.mark.parametrize("shape,K,name", [("t37", 2, "varying"), ("gauss", 2, "amount")])
def test_determinism_and_the_accumulators_are_left_zero(oracle, engines, shape, K, name):
    import stock_market_monte_carlo_amd as S
    eng, n, P = engines(shape, K), ref.n_paths(shape), 24
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)
    runs = []
    for _ in range(2):
        raw = eng.simulate_real_cashflow_raw(_sim(shape, n, P, **STATS), ref.WEIGHTS[K], 5, **ALL, **kw, **_gauss_args(shape, K))
        eng.sync()
        runs.append({k: raw[k].cpu().numpy().tobytes() for k in KEYS})
    assert runs[0] == runs[1]
    assert int(np.frombuffer(runs[0]["depleted_at"], dtype=np.uint64).sum()) == n
    # a plain simulate with buckets straight afterwards: its record is its own
    plain = S.Engine.make_sim(1000, 36, S.MODE_GAUSSIAN, 99, **STATS)
    st = eng.read_stats(eng.simulate(plain, want_final=False, want_stats=True).stats_raw)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 36, 1000, 99, **STATS))
    assert np.array_equal(st.hist, o["hist"]) and st.below == o["stats"].below and st.count == 1000
    # and a real cash flow of fewer periods straight after that: its depletion counts are its own
    short = eng.simulate_real_cashflow(_sim(shape, n, 7), ref.WEIGHTS[K], 5, **ref.cut(kw, 7), **_gauss_args(shape, K))
    assert np.array_equal(short.depleted_at, ref.reference(oracle, shape, K, ref.WEIGHTS[K], 5, name, 7)["depleted_at"])


# 7
@pytest.mark.parametrize("shape,K,name", [("t37", 3, "varying"), ("gauss", 3, "floor")])
def test_two_shards_split_at_an_odd_path_are_the_whole_request(oracle, engines, shape, K, name):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes
    eng, n, P, cut = engines(shape, K), ref.n_paths(shape), 24, 333
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)

    def run(first, count):
        raw = eng.simulate_real_cashflow_raw(_sim(shape, count, P, first=first, **STATS), ref.WEIGHTS[K], 5, **ALL, **kw,
                                             **_gauss_args(shape, K))
        eng.sync()
        return {k: raw[k].cpu().numpy() for k in KEYS}

    whole, lo, hi = run(0, n), run(0, cut), run(cut, n - cut)
    for key in ("final", "final_real", "index", "paid", "ruin_period"):
        assert np.concatenate([lo[key], hi[key]]).tobytes() == whole[key].tobytes(), key
    assert np.concatenate([lo["holdings"], hi["holdings"]], axis=1).tobytes() == whole["holdings"].tobytes()
    assert np.array_equal(lo["depleted_at"] + hi["depleted_at"], whole["depleted_at"])
    merged = S.engine.stats_from_bytes(merge_stats_bytes([lo["stats_raw"].tobytes(), hi["stats_raw"].tobytes()]))
    want = S.engine.stats_from_bytes(whole["stats_raw"].tobytes())
    assert (merged.count, merged.below, merged.underflow, merged.overflow) == (want.count, want.below, want.underflow, want.overflow)
    assert merged.min == want.min and merged.max == want.max and np.array_equal(merged.hist, want.hist)
    assert merged.sum == pytest.approx(want.sum, rel=1e-12) and merged.sumsq == pytest.approx(want.sumsq, rel=1e-12)


# 8
@pytest.mark.parametrize("shape,K,name", [("t37", 3, "varying"), ("gauss", 2, "fraction")])
def test_the_host_form_is_the_device_form(oracle, engines, shape, K, name):
    eng, n, P = engines(shape, K), ref.n_paths(shape), 24
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)
    g = _gauss_args(shape, K)
    sim = _sim(shape, n, P, **STATS)
    raw = eng.simulate_real_cashflow_raw(sim, ref.WEIGHTS[K], 12, **ALL, **kw, **g)
    eng.sync()
    host = eng.simulate_real_cashflow_to_host(sim, ref.WEIGHTS[K], 12, **ALL, **kw, **g)
    for key in KEYS:
        h = host[key] if isinstance(host[key], bytes) else host[key].tobytes()
        assert h == raw[key].cpu().numpy().tobytes(), key
    empty = eng.simulate_real_cashflow_to_host(_sim(shape, 0, P, **STATS), ref.WEIGHTS[K], 12, **ALL, **kw, **g)
    assert not empty["depleted_at"].any() and empty["final_real"].size == 0 and empty["holdings"].shape == (K, 0)
    assert not np.frombuffer(empty["stats_raw"], dtype=np.uint64)[:4].any()  # count, below, underflow, overflow


# 9
@pytest.mark.parametrize("shape,K", [("t37", 2), ("gauss", 2)])
def test_the_divide_form(oracle, engines, shape, K):
    """A request for which the rule says FAST (contributions, depleted by a floor) and one for which it says EXACT (the
    constant withdrawal the parent's rule proves and this one cannot): both the reference's bits; the FAST request forced
    with SMMC_FLAG_EXACT_DIV gives equal bytes."""
    from stock_market_monte_carlo_amd import _lib
    eng, n, P, w, R = engines(shape, K), ref.n_paths(shape), ref.longest(shape), ref.WEIGHTS[K], 5
    g = _gauss_args(shape, K)
    a = ref.multipliers(oracle, shape, K, n, P)
    paying_in = dict(amount=-15.0, floor=float(f32(1.02 * ref.CAPITAL)))  # 1.5 % in every period, depleted under 102 % in real terms
    taking_out = dict(amount=27.0, floor=0.01)
    fast, exact = _sim(shape, n, P), _sim(shape, n, P, exact_div=True)
    assert eng.real_cashflow_divide_kind(fast, w, R, **paying_in, **g) == _lib.DIV_FAST
    assert eng.real_cashflow_divide_kind(exact, w, R, **paying_in, **g) == _lib.DIV_EXACT
    assert eng.real_cashflow_divide_kind(fast, w, R, **taking_out, **g) == _lib.DIV_EXACT  # FAST in the parent
    wants = {k: v for k, v in ALL.items() if k != "want_stats"}
    for kw in (paying_in, taking_out):
        want = ref.simulate(a, w, R, **kw)
        assert 0 < int(want["depleted_at"][0]) < n
        got = _numpy(eng.simulate_real_cashflow_raw(fast, w, R, **kw, **wants, **g))
        _check_outputs(got, want, (shape, K, kw["amount"]))
        forced = _numpy(eng.simulate_real_cashflow_raw(exact, w, R, **kw, **wants, **g))
        for key in got:
            assert got[key].tobytes() == forced[key].tobytes(), key


# 10
def _case_engine(made, c):
    import stock_market_monte_carlo_amd as S
    key = ("gauss",) if c["mode"] == "gauss" else (c["T"], c["K"], c["extreme"])
    if key not in made:
        made[key] = S.Engine(0)
        if c["mode"] == "table":
            made[key].set_asset_table(RM.joint_table(c))
    return made[key]


@pytest.fixture(scope="module")
def case_engines():
    made = {}
    yield lambda c: _case_engine(made, c)
    for e in made.values():
        e.close()


def check_case(oracle, eng, c):
    """A case of tests/real_cashflow_matrix.py (or of tests/real_cashflow_fuzz.py) against its restatement."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    bins, lo, hi, below = RM.hist_range(c)
    sim = S.Engine.make_sim(c["n"], c["P"], S.MODE_GAUSSIAN if c["mode"] == "gauss" else S.MODE_TABLE, c.get("seed", RM.M.SEED),
                            first_path=c.get("first", RM.M.FIRST_PATH), initial_capital=c["capital"], n_bins=bins, hist_lo=lo, hist_hi=hi,
                            below_threshold=below, exact_div=c["exact"] == "flag")
    want = RM.reference(oracle, c)
    R, sched = want["args"]
    g = dict(zip(("means", "factor"), RM.gauss_law(c))) if c["mode"] == "gauss" else {}
    kind = eng.real_cashflow_divide_kind(sim, RM.weights(c), R, **sched, **g)
    if c["kind"] is not None:  # a fuzz case claims none
        assert kind == c["kind"], f"{c['id']}: the host chose divide kind {kind}, the ledger claims {c['kind']}"
    out = _numpy(eng.simulate_real_cashflow_raw(sim, RM.weights(c), R, **sched, **g, **ALL))
    _check_outputs(out, want, c["id"])
    _check_record(oracle, stats_from_bytes(out["stats_raw"].tobytes()), want["final_real"], c["id"], (bins, lo, hi, below))


@pytest.mark.parametrize("c", RM.CASES, ids=[c["id"] for c in RM.CASES])
def test_every_row_of_the_ledger(oracle, case_engines, c):
    check_case(oracle, case_engines(c), c)


# 11
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import real_cashflow_reference as ref
import stock_market_monte_carlo_amd as S
out, K, R = sys.argv[3], 2, 5
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
eng.set_asset_table(ref.joint_table(37, K))
means, factor = ref.gauss_law(K)
res = {"grid": grid}
for shape, mode, kW, extra in (("t37", S.MODE_TABLE, 4, {}), ("gauss", S.MODE_GAUSSIAN, 8, {"means": means, "factor": factor})):
    P = ref.longest(shape)
    kw = ref.schedules(O, shape, K, ref.WEIGHTS[K])["varying"]
    for n in (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1):
        sim = S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL, n_bins=ref.BINS,
                                hist_lo=ref.LO, hist_hi=ref.HI, below_threshold=ref.BELOW)
        raw = eng.simulate_real_cashflow_raw(sim, ref.WEIGHTS[K], R, want_index=True, want_holdings=True, want_paid=True,
                                             want_ruin_period=True, want_stats=True, **kw, **extra)
        eng.sync()
        for key in ("final", "final_real", "index", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at"):
            res[f"{shape}:{n}:{key}"] = raw[key].cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 2, R = 5, the varying schedule, both modes: every wave makes a second and a third trip, the index starts again
    at 1 for every path and the schedule is read again from its start."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid, K, R = int(got["grid"]), 2, 5
    for shape, kW in (("t37", 4), ("gauss", 8)):
        P = ref.longest(shape)
        sizes = (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1)
        a = ref.multipliers(oracle, shape, K, max(sizes), P)
        want = ref.simulate(a, ref.WEIGHTS[K], R, **ref.schedules(oracle, shape, K, ref.WEIGHTS[K])["varying"])
        for n in sizes:
            tag = (shape, n)
            cutn = {k: (v[:, :n] if k == "holdings" else v[:n]) for k, v in want.items() if k != "depleted_at"}
            cutn["depleted_at"] = np.bincount(want["ruin_period"][:n], minlength=P + 1).astype(np.uint64)
            _check_outputs({k: got[f"{shape}:{n}:{k}"] for k in KEYS if k != "stats_raw"}, cutn, tag)
            _check_record(oracle, S.engine.stats_from_bytes(got[f"{shape}:{n}:stats_raw"].tobytes()), want["final_real"][:n], tag)
