"""smmc_engine_simulate_portfolio_cashflow_checkpoints on the device against the numpy restatement of the parent's
contract with every column kept (tests/portfolio_cashflow_reference.py: simulate(..., columns=True)["values"]): record k
is the record of column periods[k] -- integer counters, buckets, min and max on their bits, the two double sums to the
relative 1e-12 of tests/test_checkpoints_gpu.py against math.fsum of the restated binary32 values and of their squares --
and every parent output is the restatement's on its bits.

Shapes are the reference module's: a joint table of 37 rows (eight draws per Philox block) with K = 1 .. 4, one of 2500
rows x 2 assets (four per block), Gaussian mode with K = 1 .. 4 (four per block); path ids from 2^32 - 100 on;
64 kW 2 + 37 paths: whole chunks, a ragged one, inactive lanes; P = 41 (tables) or 38 (Gaussian).  The schedules are the
module's, sized to deplete between 10 % and 90 % of the paths (tests/test_portfolio_cashflow_checkpoints_cpu.py asserts
that on the reference alone), so every late record holds depleted paths, as the value 0, beside live ones.

The later walk trips run in a fresh child process with SMMC_BLOCKS_PER_CU=1 (the knob is read when an engine is made);
their sizes rest on host_wave_walk_grid capping the launch at min(chunks, grid) workgroups, as in
tests/test_portfolio_cashflow_gpu.py.

On the commit before this feature every test here fails: the module imports a name that does not exist there."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import portfolio_cashflow_checkpoints_fuzz as fuzz
import portfolio_cashflow_checkpoints_matrix as CM
import portfolio_cashflow_reference as ref
from stock_market_monte_carlo_amd.engine import PortfolioCashflowCheckpointsResult  # noqa: F401  this feature's

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("portfolio_cashflow_checkpoints")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, LO, HI, BELOW = ref.BINS, ref.LO, ref.HI, ref.BELOW
STATS = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
ALL = dict(want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
KEYS = ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at")
SCHEDULES = ("amount", "varying", "floor")


def checkpoint_sets(P):
    """One period at either end, three across the boundary of an eight-draw block, pairs across the boundaries of both
    draw widths with the partial last block, and every period."""
    return [(1,), (P,), (7, 8, 9), (4, 5, 8, 9, 16, 17, P - 1, P), tuple(range(1, P + 1))]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


_columns = {}


def columns(oracle, shape, K, weights, R, name, P=None):
    """simulate(columns=True) of the named schedule on the module's paths at P periods (the longest unless given): computed
    once per request and shared, never modified."""
    P = ref.longest(shape) if P is None else P
    key = (shape, K, tuple(float(x) for x in weights), R, name, P)
    if key not in _columns:
        a = ref.multipliers(oracle, shape, K, ref.n_paths(shape), max(P, ref.longest(shape)))[:, :P]
        sched = ref.schedules(oracle, shape, K, weights)[name]
        out = ref.simulate(a, weights, R, columns=True, **(ref.cut(sched, P) if P <= ref.longest(shape) else sched))
        for x in out.values():
            x.setflags(write=False)
        _columns[key] = out
    return _columns[key]


def _sim(shape, n, P, first=0, **kw):
    import stock_market_monte_carlo_amd as S
    mode = S.MODE_GAUSSIAN if shape == "gauss" else S.MODE_TABLE
    return S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH + first, initial_capital=ref.CAPITAL, **kw)


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
    nan = np.isnan(np.float32([ost.min, ost.max]))
    assert np.array_equal(np.isnan(np.float32([st.min, st.max])), nan), tag
    assert np.array_equal(_bits([st.min, st.max])[~nan], _bits([ost.min, ost.max])[~nan]), tag
    assert np.array_equal(st.hist, ohist) and (not bins or int(st.hist.sum()) + st.underflow + st.overflow == values.size), tag
    d = values.astype(np.float64)
    with np.errstate(all="ignore"):
        _same_sum(st.sum, _fsum(d.tolist()), tag)
        _same_sum(st.sumsq, _fsum((d * d).tolist()), tag)


def _same_record(a, b, tag):
    """The rule for two device records folded over different partial layouts."""
    assert (a.count, a.below, a.underflow, a.overflow) == (b.count, b.below, b.underflow, b.overflow), tag
    assert np.array_equal(_bits([a.min, a.max]), _bits([b.min, b.max])) and np.array_equal(a.hist, b.hist), tag
    assert a.sum == pytest.approx(b.sum, rel=1e-12) and a.sumsq == pytest.approx(b.sumsq, rel=1e-12), tag


def _same_floats(got, want, tag):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), tag
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), tag


def _check_outputs(r, want, tag):
    _same_floats(r.final.cpu().numpy(), want["final"], tag)
    _same_floats(r.holdings.cpu().numpy(), want["holdings"], tag)
    _same_floats(r.paid.cpu().numpy(), want["paid"], tag)
    assert np.array_equal(r.ruin_period.cpu().numpy().view(np.uint32), want["ruin_period"]), tag
    assert np.array_equal(r.depleted_at, want["depleted_at"]) and int(r.depleted_at.sum()) == want["final"].size, tag


def _records(raw, n_bins):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    host = raw["records_raw"] if isinstance(raw["records_raw"], bytes) else raw["records_raw"].cpu().numpy().tobytes()
    rec = 64 + 8 * n_bins
    assert len(host) == rec * len(raw["periods"])
    return [stats_from_bytes(host[k * rec:(k + 1) * rec]) for k in range(len(raw["periods"]))]


def _cases():
    for shape, K in ref.SHAPES:
        yield shape, K, ref.WEIGHTS[K]


# 1
@pytest.mark.parametrize("shape,K,weights", list(_cases()))
def test_records_and_parent_outputs_are_the_restatement(oracle, engines, shape, K, weights):
    """Every schedule, R in 0 and 5, every checkpoint set: each record is the record of its column, the parent outputs are
    the restatement's on their bits, and the record of the final values is the record at P."""
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    sched = ref.schedules(oracle, shape, K, weights)
    for name in SCHEDULES:
        for R in (0, 5):
            want = columns(oracle, shape, K, weights, R, name)
            assert 0.10 <= 1.0 - want["depleted_at"][0] / n <= 0.90
            for periods in checkpoint_sets(P):
                tag = (shape, K, name, R, periods)
                r = eng.simulate_portfolio_cashflow_checkpoints(_sim(shape, n, P, **STATS), weights, periods, R, **sched[name], **ALL,
                                                                **_gauss_args(shape, K))
                assert list(r.periods) == list(periods) and len(r.checkpoints) == len(periods), tag
                for st, p in zip(r.checkpoints, periods):
                    _check_record(oracle, st, want["values"][:, p], tag + (p,))
                    assert (st.hist_lo, st.hist_hi) == (LO, HI)
                _check_outputs(r, want, tag)
                _check_record(oracle, r.stats, want["final"], tag + ("final",))
                if periods[-1] == P:
                    _same_record(r.checkpoints[-1], r.stats, tag)


# 2
@pytest.mark.parametrize("shape,K,name,R", [("t37", 3, "amount", 5), ("t2500", 2, "varying", 0), ("gauss", 4, "floor", 5),
                                            ("gauss", 1, "varying", 12)])
def test_parent_outputs_are_those_of_the_parent_call(oracle, engines, shape, K, name, R):
    """Device against device: every parent output of the new call is simulate_portfolio_cashflow_raw's of the same request
    on its bits (of the record: integers, min, max and buckets; the sums to 1e-12), and the record at P is the final one."""
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    kw = dict(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], **_gauss_args(shape, K))
    sim = _sim(shape, n, P, **STATS)
    parent = eng.simulate_portfolio_cashflow_raw(sim, ref.WEIGHTS[K], R, **ALL, **kw)
    eng.sync()
    for periods in ((P,), (3, 8, P - 1, P)):
        got = eng.simulate_portfolio_cashflow_checkpoints_raw(sim, ref.WEIGHTS[K], periods, R, **ALL, **kw)
        eng.sync()
        for key in ("final", "holdings", "paid", "ruin_period", "depleted_at"):
            assert got[key].cpu().numpy().tobytes() == parent[key].cpu().numpy().tobytes(), (key, periods)
        final = stats_from_bytes(got["stats_raw"].cpu().numpy().tobytes())
        _same_record(final, stats_from_bytes(parent["stats_raw"].cpu().numpy().tobytes()), periods)
        _same_record(_records(got, BINS)[-1], final, periods)
    # without the final record and without any parent output: the records stay what they were
    bare = eng.simulate_portfolio_cashflow_checkpoints_raw(sim, ref.WEIGHTS[K], (3, 8, P - 1, P), R, want_final=False,
                                                           want_depleted_at=False, **kw)
    eng.sync()
    assert bare["records_raw"].cpu().numpy().tobytes() == got["records_raw"].cpu().numpy().tobytes()


# 3
@pytest.mark.parametrize("T", [37, 2500])
def test_one_asset_with_weight_one_and_no_flows_is_simulate_checkpoints_on_that_column(T):
    import stock_market_monte_carlo_amd as S
    shape, column = "t%d" % T, ref.asset_table(T, 1)
    n, P = ref.n_paths(shape), 41
    eng = S.Engine(0)
    try:
        eng.set_table(column[:, 0])
        eng.set_asset_table(column)
        sim = _sim(shape, n, P, **STATS)
        for periods in checkpoint_sets(P):
            want, want_final = eng.simulate_checkpoints(sim, periods, want_final=True)
            for R in (0, 5):
                got = eng.simulate_portfolio_cashflow_checkpoints(sim, (1.0,), periods, R, want_stats=True)
                assert got.final.cpu().numpy().tobytes() == want_final.cpu().numpy().tobytes() and got.depleted_at[0] == n
                assert (got.final.cpu().numpy() > 0).all()
                for a, b, p in zip(got.checkpoints, want, periods):
                    _same_record(a, b, (T, periods, R, p))
    finally:
        eng.close()


# 4
@pytest.mark.parametrize("shape,K", [("t37", 2), ("t2500", 2), ("gauss", 3)])
def test_below_the_floor_is_depleted_by_then(oracle, engines, shape, K):
    """With below_threshold == floor == FLOOR a live value is above the threshold and a depleted one, 0, below it: `below`
    of record k is the number of paths depleted at or before periods[k]."""
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    periods = tuple(range(1, P + 1))
    own = ref.schedules(oracle, shape, K, ref.WEIGHTS[K])["fraction"]["floor"]  # the fraction schedule depletes by its own floor
    for name, floor in [(name, ref.FLOOR) for name in ref.SCHEDULES] + [("fraction", own)]:
        kw = dict(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], floor=floor)
        r = eng.simulate_portfolio_cashflow_checkpoints(_sim(shape, n, P, n_bins=0, below_threshold=floor), ref.WEIGHTS[K], periods, 5,
                                                        **kw, **_gauss_args(shape, K))
        gone = np.cumsum(r.depleted_at) - r.depleted_at[0]
        assert (name, floor) == ("fraction", ref.FLOOR) or 0 < gone[P] < n, name
        assert [st.below for st in r.checkpoints] == [int(gone[p]) for p in periods], name
        assert all(len(st.hist) == 0 and st.count == n for st in r.checkpoints)
        assert np.allclose(r.depleted_by(), gone[1:] / n, rtol=0, atol=0)


# 5
def test_the_bucket_budget_edge(oracle, engines):
    """64 checkpoints x 128 buckets = SMMC_MAX_CHECKPOINT_BINS is accepted and right; one bucket more is refused."""
    from stock_market_monte_carlo_amd import _lib
    shape, K, P = "t37", 2, 64
    eng, n = engines(shape, K), ref.n_paths(shape)
    level = float(np.float32(0.6 * ref.schedules(oracle, shape, K, ref.WEIGHTS[K])["amount"]["amount"]))  # sized for 41 periods: less for 64
    a = ref.multipliers(oracle, shape, K, n, P)
    want = ref.simulate(a, ref.WEIGHTS[K], 12, amount=level, columns=True)
    assert 0 < want["depleted_at"][0] < n
    periods = tuple(range(1, _lib.MAX_CHECKPOINTS + 1))
    assert len(periods) * 128 == _lib.MAX_CHECKPOINT_BINS
    rng = (128, LO, HI, BELOW)
    r = eng.simulate_portfolio_cashflow_checkpoints(_sim(shape, n, P, n_bins=128, hist_lo=LO, hist_hi=HI, below_threshold=BELOW),
                                                    ref.WEIGHTS[K], periods, 12, amount=level, **ALL)
    for st, p in zip(r.checkpoints, periods):
        _check_record(oracle, st, want["values"][:, p], ("edge", p), rng)
    _check_outputs(r, want, "edge")
    _check_record(oracle, r.stats, want["final"], "edge", rng)
    with pytest.raises(_lib.SmmcError, match="SMMC_MAX_CHECKPOINT_BINS"):
        eng.simulate_portfolio_cashflow_checkpoints(_sim(shape, n, P, n_bins=129, hist_lo=LO, hist_hi=HI, below_threshold=BELOW),
                                                    ref.WEIGHTS[K], periods, 12, amount=level)
    # the refusal came before any device work: the engine's next call is its own
    again = eng.simulate_portfolio_cashflow_checkpoints(_sim(shape, n, P, n_bins=128, hist_lo=LO, hist_hi=HI, below_threshold=BELOW),
                                                        ref.WEIGHTS[K], periods, 12, amount=level)
    for x, y in zip(again.checkpoints, r.checkpoints):
        assert (x.count, x.sum, x.sumsq) == (y.count, y.sum, y.sumsq) and np.array_equal(x.hist, y.hist)


# 6
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import portfolio_cashflow_reference as ref
import stock_market_monte_carlo_amd as S
out, K, R = sys.argv[3], 3, 5
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
eng.set_asset_table(ref.asset_table(37, K))
means, stds, corr = ref.gauss_setup(K)
res = {"grid": grid}
for shape, mode, kW, extra in (("t37", S.MODE_TABLE, 4, {}), ("gauss", S.MODE_GAUSSIAN, 8, {"means": means, "factor": ref.factor_of(stds, corr)})):
    P = ref.longest(shape)
    kw = ref.schedules(O, shape, K, ref.WEIGHTS[K])["varying"]
    for n in (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1):
        sim = S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL, n_bins=ref.BINS,
                                hist_lo=ref.LO, hist_hi=ref.HI, below_threshold=ref.BELOW)
        raw = eng.simulate_portfolio_cashflow_checkpoints_raw(sim, ref.WEIGHTS[K], (4, 5, 8, 9, 16, 17, P - 1, P), R, want_holdings=True,
                                                              want_paid=True, want_ruin_period=True, want_stats=True, **kw, **extra)
        eng.sync()
        for key in ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at", "records_raw"):
            res[f"{shape}:{n}:{key}"] = raw[key].cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 3, R = 5, the varying schedule, both modes: every wave makes a second and a third trip; lane k's accumulators
    and the LDS buckets persist across them, `until`, the checkpoint index and the schedule start again per path."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid, K, R = int(got["grid"]), 3, 5
    for shape, kW in (("t37", 4), ("gauss", 8)):
        P = ref.longest(shape)
        periods = (4, 5, 8, 9, 16, 17, P - 1, P)
        sizes = (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1)
        a = ref.multipliers(oracle, shape, K, max(sizes), P)
        want = ref.simulate(a, ref.WEIGHTS[K], R, columns=True, **ref.schedules(oracle, shape, K, ref.WEIGHTS[K])["varying"])
        for n in sizes:
            tag = (shape, n)
            assert np.array_equal(_bits(got[f"{shape}:{n}:final"]), _bits(want["final"][:n])), tag
            assert np.array_equal(_bits(got[f"{shape}:{n}:holdings"]), _bits(want["holdings"][:, :n])), tag
            assert np.array_equal(_bits(got[f"{shape}:{n}:paid"]), _bits(want["paid"][:n])), tag
            assert np.array_equal(got[f"{shape}:{n}:ruin_period"].view(np.uint32), want["ruin_period"][:n]), tag
            assert np.array_equal(got[f"{shape}:{n}:depleted_at"].view(np.uint64), np.bincount(want["ruin_period"][:n], minlength=P + 1)), tag
            _check_record(oracle, S.engine.stats_from_bytes(got[f"{shape}:{n}:stats_raw"].tobytes()), want["final"][:n], tag)
            recs = _records({"records_raw": got[f"{shape}:{n}:records_raw"].tobytes(), "periods": periods}, BINS)
            for st, p in zip(recs, periods):
                _check_record(oracle, st, want["values"][:n, p], tag + (p,))


# 7
@pytest.mark.parametrize("shape,K,name", [("t37", 2, "varying"), ("gauss", 2, "amount")])
def test_determinism_and_the_accumulator_is_left_zero(oracle, engines, shape, K, name):
    import stock_market_monte_carlo_amd as S
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    kw = dict(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], **_gauss_args(shape, K))
    periods = (1, 8, 9, 24, P)
    runs = []
    for _ in range(2):
        raw = eng.simulate_portfolio_cashflow_checkpoints_raw(_sim(shape, n, P, **STATS), ref.WEIGHTS[K], periods, 5, **ALL, **kw)
        eng.sync()
        runs.append({k: raw[k].cpu().numpy().tobytes() for k in KEYS + ("records_raw",)})
    assert runs[0] == runs[1]
    # a parent call straight afterwards is the parent's own: the reference's, with a record of its own
    want = columns(oracle, shape, K, ref.WEIGHTS[K], 5, name)
    r = eng.simulate_portfolio_cashflow(_sim(shape, n, P, **STATS), ref.WEIGHTS[K], 5, **ALL, **kw)
    _check_outputs(r, want, "parent after")
    _check_record(oracle, r.stats, want["final"], "parent after")
    # and a checkpoint call of the single-series kernel after that (its buckets lie where copy 0 and the depletion counters lay)
    one = S.Engine.make_sim(1000, 36, S.MODE_GAUSSIAN, 99, **STATS)
    stats, _ = eng.simulate_checkpoints(one, list(range(1, 37)))
    traj = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 36, 1000, 99), want_final=False, want_traj=True)["traj"]
    for st, p in zip(stats, range(1, 37)):
        _check_record(oracle, st, traj[:, p], ("checkpoints after", p))
    # and the new call once more: the same bytes as before
    raw = eng.simulate_portfolio_cashflow_checkpoints_raw(_sim(shape, n, P, **STATS), ref.WEIGHTS[K], periods, 5, **ALL, **kw)
    eng.sync()
    assert {k: raw[k].cpu().numpy().tobytes() for k in KEYS + ("records_raw",)} == runs[0]


# 8
@pytest.mark.parametrize("shape,K,name", [("t37", 3, "varying"), ("gauss", 3, "floor")])
def test_two_shards_split_at_an_odd_path_are_the_whole_request(oracle, engines, shape, K, name):
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes, stats_from_bytes
    eng, n, P, cut = engines(shape, K), ref.n_paths(shape), ref.longest(shape), 333
    kw = dict(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], **_gauss_args(shape, K))
    periods = (2, 8, 9, 30, P)
    rec = 64 + 8 * BINS

    def run(first, count):
        raw = eng.simulate_portfolio_cashflow_checkpoints_raw(_sim(shape, count, P, first=first, **STATS), ref.WEIGHTS[K], periods, 5,
                                                              **ALL, **kw)
        eng.sync()
        return {k: raw[k].cpu().numpy() for k in KEYS + ("records_raw",)}

    whole, lo, hi = run(0, n), run(0, cut), run(cut, n - cut)
    for key in ("final", "paid", "ruin_period"):
        assert np.concatenate([lo[key], hi[key]]).tobytes() == whole[key].tobytes(), key
    assert np.array_equal(lo["depleted_at"] + hi["depleted_at"], whole["depleted_at"])
    for k in range(len(periods)):
        part = [x["records_raw"].tobytes()[k * rec:(k + 1) * rec] for x in (lo, hi)]
        merged = stats_from_bytes(merge_stats_bytes(part))
        _same_record(merged, stats_from_bytes(whole["records_raw"].tobytes()[k * rec:(k + 1) * rec]), (shape, periods[k]))


# 9
@pytest.mark.parametrize("shape,K,name", [("t37", 4, "varying"), ("gauss", 2, "floor")])
def test_the_host_form_is_the_device_form(oracle, engines, shape, K, name):
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    kw = dict(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], **_gauss_args(shape, K))
    periods = (1, 7, 8, 9, P)
    sim = _sim(shape, n, P, **STATS)
    raw = eng.simulate_portfolio_cashflow_checkpoints_raw(sim, ref.WEIGHTS[K], periods, 12, **ALL, **kw)
    eng.sync()
    host = eng.simulate_portfolio_cashflow_checkpoints_to_host(sim, ref.WEIGHTS[K], periods, 12, **ALL, **kw)
    for key in KEYS + ("records_raw",):
        h = host[key] if isinstance(host[key], bytes) else host[key].tobytes()
        assert h == raw[key].cpu().numpy().tobytes(), key
    empty = eng.simulate_portfolio_cashflow_checkpoints_to_host(_sim(shape, 0, P, **STATS), ref.WEIGHTS[K], periods, 12, **ALL, **kw)
    assert not empty["depleted_at"].any() and empty["final"].size == 0
    for st in _records(empty, BINS):
        assert (st.count, st.below, st.underflow, st.overflow) == (0, 0, 0, 0) and not st.hist.any() and len(st.hist) == BINS


# 10
@pytest.mark.parametrize("shape,K", [("t37", 2), ("gauss", 3)])
def test_the_divide_form_never_shows(oracle, engines, shape, K):
    """A request the parent's rule proves for the fast divide, the same with SMMC_FLAG_EXACT_DIV, and one the rule cannot
    prove (a fraction): all agree with the restatement, which divides by 100."""
    from stock_market_monte_carlo_amd import _lib
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    g = _gauss_args(shape, K)
    a = ref.multipliers(oracle, shape, K, n, P)
    periods = (1, 8, 9, P - 1, P)
    for kw, kinds in ((dict(amount=27.0, floor=0.01), (_lib.DIV_FAST, _lib.DIV_EXACT)), (dict(amount=27.0, fraction=0.004, floor=0.01), (_lib.DIV_EXACT,) * 2)):
        want = ref.simulate(a, ref.WEIGHTS[K], 5, columns=True, **kw)
        assert 0 < want["depleted_at"][0] < n
        for exact, kind in zip((False, True), kinds):
            sim = _sim(shape, n, P, exact_div=exact, **STATS)
            assert eng.portfolio_cashflow_divide_kind(sim, ref.WEIGHTS[K], 5, **kw, **g) == kind
            r = eng.simulate_portfolio_cashflow_checkpoints(sim, ref.WEIGHTS[K], periods, 5, **kw, **ALL, **g)
            _check_outputs(r, want, (kw, exact))
            for st, p in zip(r.checkpoints, periods):
                _check_record(oracle, st, want["values"][:, p], (kw, exact, p))


@pytest.fixture(scope="module")
def matrix_engines():
    import stock_market_monte_carlo_amd as S
    import feature_matrix as M
    made = {}

    def get(c):
        key = ("gauss",) if c["mode"] == "gauss" else (c.get("i"), c["T"], c["K"], c["extreme"])
        if key not in made:
            made[key] = S.Engine(0)
            if c["mode"] == "table":
                made[key].set_asset_table(M.assets(c))
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _run_case(oracle, eng, c, want):
    import stock_market_monte_carlo_amd as S
    import feature_matrix as M
    bins, lo, hi, below = M.hist_range(c)
    sim = S.Engine.make_sim(c["n"], c["P"], S.MODE_GAUSSIAN if c["mode"] == "gauss" else S.MODE_TABLE, c.get("seed", M.SEED),
                            first_path=c.get("first", M.FIRST_PATH), initial_capital=c["capital"], n_bins=bins, hist_lo=lo, hist_hi=hi,
                            below_threshold=below, exact_div=c["exact"] == "flag")
    pf = {}
    if c["mode"] == "gauss":
        means, factor = M.gauss_portfolio(c)
        pf = {"means": means, "factor": factor}
    R, sched = M.rebalance(c), (want["args"][1] if "args" in want else c["schedule"])
    if c["kind"] is not None:
        kind = eng.portfolio_cashflow_divide_kind(sim, M.weights(c), R, **sched, **pf)
        assert kind == c["kind"], f"{c['id']}: the host chose divide kind {kind}, the ledger claims {c['kind']}"
    r = eng.simulate_portfolio_cashflow_checkpoints(sim, M.weights(c), c["periods"], R, **sched, **ALL, **pf)
    _check_outputs(r, want, c["id"])
    _check_record(oracle, r.stats, want["final"], c["id"], (bins, lo, hi, below))
    for st, p in zip(r.checkpoints, c["periods"]):
        _check_record(oracle, st, want["values"][:, p], (c["id"], p), (bins, lo, hi, below))


@pytest.mark.parametrize("c", CM.CASES, ids=[c["id"] for c in CM.CASES])
def test_every_instantiation(oracle, matrix_engines, c):
    """The 48 rows of the ledger, and the cases whose inputs tell the fast divide from the IEEE one, at the ledger's sizes."""
    _run_case(oracle, matrix_engines(c), c, CM.reference(oracle, c))


# 11
@pytest.fixture(scope="module")
def fuzz_cases(oracle):
    return list(fuzz.cases(oracle))  # drawn once: the generator sizes every schedule on the restatement


@pytest.mark.parametrize("i", range(fuzz.COUNT))
def test_random_requests(oracle, matrix_engines, fuzz_cases, i):
    c = fuzz_cases[i]
    _run_case(oracle, matrix_engines(c), c, fuzz.reference(oracle, c))
