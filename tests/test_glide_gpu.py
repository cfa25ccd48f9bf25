"""smmc_engine_simulate_glide on the device against the numpy restatement of its contract (tests/glide_reference.py):
final values, holdings, totals paid, periods of depletion and the depletion counts on their bits; of the record the integer
counters, buckets, min and max on their bits and the two double sums to the relative 1e-12 of tests/test_gpu_parity.py,
as tests/test_feature_matrix_gpu.py compares a portfolio cash flow.  No tolerance on any per-path output.

Shapes: those of tests/feature_matrix.py -- 64 kW 2 + 37 paths with kW = 4 (table) or 8 (Gaussian), ids from 2^32 - 100 on,
9 periods on a dense table and 5 on a four-draw table and in Gaussian mode, R = 3 -- for every one of the 36
instantiations (the rows without the flag must be FAST by the host's rule, asked before the run), and the edges: a change
after period 1, on the Philox-block boundary and one past it, on a rebalance period and off it, at P - 1 and at P, beyond
P, two in consecutive periods, an asset taken to weight 0 and brought back (EXACT without the flag), and 512 changes.
tests/test_glide_cpu.py shows on the restatement alone that no case is vacuous.  The later walk trips -- a wave's second
and third chunk must start from the request's weights again -- run in a fresh child process with SMMC_BLOCKS_PER_CU=1.

On the commit before this feature every test here fails: the symbols do not exist."""
import os
import subprocess
import sys

import numpy as np
import pytest

import glide_reference as G
import test_feature_matrix_gpu as FG

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("glide")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANTS = ("final", "holdings", "paid", "ruin_period", "stats", "depleted_at")
KEYS = tuple("stats_raw" if k == "stats" else k for k in WANTS)
ALL = {"want_" + k: True for k in WANTS}
M = G.M


def _numpy(raw):
    return {k: t.cpu().numpy() for k, t in raw.items() if k != "n_assets" and t is not None}


def _engine(made, c):
    import stock_market_monte_carlo_amd as S
    key = ("gauss",) if c["mode"] == "gauss" else ("table", c["K"], id(M.assets(c)))
    if key not in made:
        made[key] = S.Engine(0)
        if c["mode"] == "table":
            made[key].set_asset_table(M.assets(c))
    return made[key]


@pytest.fixture(scope="module")
def engines():
    made = {}
    yield lambda c: _engine(made, c)
    for e in made.values():
        e.close()


def _law(c):
    return FG._portfolio_args(c)


def _sim(c, n=None, first=0, exact=None):
    import stock_market_monte_carlo_amd as S
    bins, lo, hi, below = M.hist_range(c)
    return S.Engine.make_sim(c["n"] if n is None else n, c["P"], S.MODE_GAUSSIAN if c["mode"] == "gauss" else S.MODE_TABLE,
                             c.get("seed", M.SEED), first_path=c.get("first", M.FIRST_PATH) + first, initial_capital=c["capital"],
                             n_bins=bins, hist_lo=lo, hist_hi=hi, below_threshold=below,
                             exact_div=(c["exact"] == "flag") if exact is None else exact)


def _run(eng, c, sched, changes=None, sim=None, weights=None, R=None, **wants):
    raw = eng.simulate_glide_raw(_sim(c) if sim is None else sim, G.weights(c) if weights is None else weights,
                                 c["changes"] if changes is None else changes, c["R"] if R is None else R, **sched, **_law(c),
                                 **(wants or ALL))
    eng.sync()
    return _numpy(raw)


def _parent(eng, c, sched, sim=None, weights=None):
    raw = eng.simulate_portfolio_cashflow_raw(_sim(c) if sim is None else sim, G.weights(c) if weights is None else weights, c["R"],
                                              **sched, **_law(c), **ALL)
    eng.sync()
    return _numpy(raw)


def _same_bytes(a, b, tag, keys=KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


def check_case(oracle, eng, c):
    """A case of tests/glide_reference.py (a listed one or a fuzz case) against its restatement."""
    want, sched = G.reference(oracle, c), G.schedule(oracle, c)
    FG._kind(eng.glide_divide_kind(_sim(c), G.weights(c), c["changes"], c["R"], **sched, **_law(c)), c)
    out = _run(eng, c, sched)
    FG._check_cashflow(oracle, out, want, c, c["id"])
    FG._same_floats(out["holdings"], want["holdings"], c["id"])
    return out


# 1
@pytest.mark.parametrize("c", G.ALL_CASES, ids=[c["id"] for c in G.ALL_CASES])
def test_outputs_bit_for_bit(oracle, engines, c):
    """Every instantiation, in the divide the ledger claims for it, and every edge: all six outputs."""
    check_case(oracle, engines(c), c)


# 2
@pytest.mark.parametrize("c", [c for c in G.EDGES if c.get("edge") == "at_last"], ids=lambda c: c["id"])
def test_a_change_at_the_last_period_moves_the_final_holdings_and_not_the_final_value(oracle, engines, c):
    eng, sched = engines(c), G.schedule(oracle, c)
    got, parent = _run(eng, c, sched), _parent(eng, c, sched)
    _same_bytes(got, parent, c["id"], ("final", "paid", "ruin_period", "stats_raw", "depleted_at"))
    live = parent["ruin_period"] == 0
    assert live.any() and (got["holdings"][:, live] != parent["holdings"][:, live]).any(axis=0).mean() > 0.9
    assert got["holdings"][:, ~live].tobytes() == parent["holdings"][:, ~live].tobytes()  # a depleted path holds 0


@pytest.mark.parametrize("c", [c for c in G.EDGES if c.get("edge") == "beyond"], ids=lambda c: c["id"])
def test_changes_beyond_the_last_period_are_never_reached(oracle, engines, c):
    eng, sched = engines(c), G.schedule(oracle, c)
    _same_bytes(_run(eng, c, sched), _parent(eng, c, sched), c["id"])


# 3
IDENTITY = [c for c in G.CASES if c["K"] == 3]


@pytest.mark.parametrize("c", IDENTITY, ids=lambda c: c["id"])
def test_identity_1_without_a_change_or_with_equal_rows_it_is_the_parent(oracle, engines, c):
    """Against smmc_engine_simulate_portfolio_cashflow on the device, all six outputs byte for byte."""
    eng, sched, w = engines(c), G.schedule(oracle, c), G.weights(c)
    parent = _parent(eng, c, sched)
    assert G.fast_varying(c) or 0 < int(parent["depleted_at"].view(np.uint64)[0]) < c["n"]
    _same_bytes(_run(eng, c, sched, changes=()), parent, (c["id"], "no change"))
    same = tuple((a, w) for a, _ in c["changes"]) + ((c["P"], w),)
    _same_bytes(_run(eng, c, sched, changes=same), parent, (c["id"], "equal rows"))
    assert _run(eng, c, sched)["final"].tobytes() != parent["final"].tobytes()  # and the case's own changes do act


@pytest.mark.parametrize("c", IDENTITY, ids=lambda c: c["id"])
def test_identity_2_without_flows_and_rebalancing_nothing_trades(oracle, engines, c):
    """Zero flows and R = 0: smmc_engine_simulate_portfolio's final values and holdings whatever the changes are."""
    eng, w = engines(c), G.weights(c)
    zero = dict(amount=0.0, fraction=0.0, floor=0.0)
    got = _run(eng, c, zero, R=0)
    plain = eng.simulate_portfolio(_sim(c), w, 0, want_holdings=True, **_law(c))
    assert got["final"].tobytes() == plain.final.cpu().numpy().tobytes()
    assert got["holdings"].tobytes() == plain.holdings.cpu().numpy().tobytes()
    assert not got["ruin_period"].any() and not got["paid"].any()


# 4
@pytest.mark.parametrize("mode, T", [("table", M.DENSE), ("gauss", 0)])
def test_one_asset_is_the_parent_call(oracle, engines, mode, T):
    c = M._case("portfolio_cashflow_kernel", (0, False, False, 1, False), mode, T, K=1)
    c.update(R=G.R, changes=((2, (1.0,)), (4, (1.0,))), id=f"glide-one-asset-{mode}")
    eng, sched = engines(c), G.sized_schedule(oracle, c)
    c["schedule"] = sched
    got = check_case(oracle, eng, c)
    _same_bytes(got, _parent(eng, c, sched), c["id"])
    assert 0 < int(got["depleted_at"].view(np.uint64)[0]) < c["n"]


# 5
@pytest.mark.parametrize("c", [G.CASES[0], G.CASES[14], G.CASES[27]], ids=lambda c: c["id"])
def test_determinism_shards_and_the_host_form(oracle, engines, c):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes
    eng, n, cut, sched = engines(c), c["n"], 333, G.schedule(oracle, c)
    whole, again = _run(eng, c, sched), _run(eng, c, sched)
    lo, hi = _run(eng, c, sched, sim=_sim(c, n=cut)), _run(eng, c, sched, sim=_sim(c, n=n - cut, first=cut))
    _same_bytes(whole, again, c["id"])  # two identical calls give the same bytes
    for key in ("final", "paid", "ruin_period"):
        assert np.concatenate([lo[key], hi[key]]).tobytes() == whole[key].tobytes(), key
    assert np.concatenate([lo["holdings"], hi["holdings"]], axis=1).tobytes() == whole["holdings"].tobytes()
    assert np.array_equal(lo["depleted_at"] + hi["depleted_at"], whole["depleted_at"])
    merged = S.engine.stats_from_bytes(merge_stats_bytes([lo["stats_raw"].tobytes(), hi["stats_raw"].tobytes()]))
    want = S.engine.stats_from_bytes(whole["stats_raw"].tobytes())
    assert (merged.count, merged.below, merged.underflow, merged.overflow) == (want.count, want.below, want.underflow, want.overflow)
    assert merged.min == want.min and merged.max == want.max and np.array_equal(merged.hist, want.hist)
    assert merged.sum == pytest.approx(want.sum, rel=1e-12) and merged.sumsq == pytest.approx(want.sumsq, rel=1e-12)
    # a path does not depend on first_path: the second shard alone is the reference's tail
    assert hi["final"].tobytes() == G.reference(oracle, c)["final"][cut:].tobytes()
    # the host form, and no paths
    kw = dict(rebalance_every=c["R"], **sched, **_law(c), **ALL)
    host = eng.simulate_glide_to_host(_sim(c), G.weights(c), c["changes"], **kw)
    for key in KEYS:
        h = host[key] if isinstance(host[key], bytes) else host[key].tobytes()
        assert h == whole[key].tobytes(), key
    for empty in (eng.simulate_glide_to_host(_sim(c, n=0), G.weights(c), c["changes"], **kw), _run(eng, c, sched, sim=_sim(c, n=0))):
        assert not empty["depleted_at"].any() and empty["final"].size == 0 and empty["holdings"].shape == (c["K"], 0)
        raw = empty["stats_raw"] if isinstance(empty["stats_raw"], bytes) else empty["stats_raw"].tobytes()
        assert not np.frombuffer(raw, dtype=np.uint64)[:4].any()  # count, below, underflow, overflow
    # the result object is the parent's
    r = eng.simulate_glide(_sim(c), G.weights(c), c["changes"], c["R"], **sched, **_law(c), want_stats=True)
    assert isinstance(r, S.PortfolioCashflowResult) and r.n_assets == c["K"]
    assert np.array_equal(r.depleted_at, whole["depleted_at"].view(np.uint64)) and r.survival()[-1] == pytest.approx(r.depleted_at[0] / n)


# 6
@pytest.mark.parametrize("c", [G.CASES[5], G.CASES[18]], ids=lambda c: c["id"])
def test_null_outputs_leave_the_others_unchanged(oracle, engines, c):
    """Every single output alone, and every output left out alone: what is written is what the full call writes."""
    eng, sched = engines(c), G.schedule(oracle, c)
    full = _run(eng, c, sched)
    none = {k: False for k in ALL}
    for want in WANTS:
        key = "stats_raw" if want == "stats" else want
        only = _run(eng, c, sched, **dict(none, **{"want_" + want: True}))
        assert set(only) == {key} and only[key].tobytes() == full[key].tobytes(), want
        rest = _run(eng, c, sched, **dict(ALL, **{"want_" + want: False}))
        assert set(rest) == set(KEYS) - {key}, want
        _same_bytes(rest, full, want, rest.keys())


def test_both_divides_give_the_same_bytes_where_the_rule_allows_the_fast_one(oracle, engines):
    from stock_market_monte_carlo_amd import _lib
    for c in (c for c in G.CASES if c["kind"] == M.DIV_FAST):
        eng, sched = engines(c), G.schedule(oracle, c)
        args = (G.weights(c), c["changes"], c["R"])
        assert eng.glide_divide_kind(_sim(c, exact=False), *args, **sched, **_law(c)) == _lib.DIV_FAST, c["id"]
        assert eng.glide_divide_kind(_sim(c, exact=True), *args, **sched, **_law(c)) == _lib.DIV_EXACT, c["id"]
        _same_bytes(_run(eng, c, sched, sim=_sim(c, exact=False)), _run(eng, c, sched, sim=_sim(c, exact=True)), c["id"])


def test_bad_arguments_are_refused_on_the_device_build_too(oracle, engines):
    from stock_market_monte_carlo_amd import SmmcError
    c = G.CASES[2]
    eng, sched, row = engines(c), G.schedule(oracle, c), G.ROWS[c["K"]][0]
    bad_rows = [((0, row),), ((3, row), (3, row)), ((4, row), (2, row)), ((2, (0.5, 0.6)),), ((2, (-0.5, 1.5)),), ((2, (0.5, 0.25, 0.125, 0.125)),),
                tuple((t, row) for t in range(1, G.MAX_CHANGES + 2))]
    for changes in bad_rows:
        with pytest.raises(SmmcError):
            eng.simulate_glide_raw(_sim(c), G.weights(c), changes, c["R"], **sched, **_law(c))
        with pytest.raises(SmmcError):
            eng.glide_divide_kind(_sim(c), G.weights(c), changes, c["R"], **sched, **_law(c))


# 7
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import glide_reference as G
import test_feature_matrix_gpu as FG
import stock_market_monte_carlo_amd as S
out = sys.argv[3]
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
res = {"grid": grid}
for i, kW in ((0, 8), (24, 4)):
    c = G.CASES[i]
    if c["mode"] == "table":
        eng.set_asset_table(G.M.assets(c))
    sched = G.schedule(O, c)
    for n in (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1):
        raw = eng.simulate_glide_raw(FG._sim(dict(c, n=n)), G.weights(c), c["changes"], c["R"], want_holdings=True, want_paid=True,
                                     want_ruin_period=True, want_stats=True, **sched, **FG._portfolio_args(c))
        eng.sync()
        for key, t in raw.items():
            if key != "n_assets":
                res[f"{i}:{n}:{key}"] = t.cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 2, both modes, two changes inside the plan: every wave makes a second and a third trip, and each must start from
    the request's weights, the countdown to the first change and the first entry of the change table again."""
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid = int(got["grid"])
    for i, kW in ((0, 8), (24, 4)):
        c = G.CASES[i]
        assert c["K"] == 2 and len([a for a, _ in c["changes"] if a < c["P"]]) == 2
        sched = G.schedule(oracle, c)
        sizes = (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1)
        a = G.multipliers(oracle, dict(c, n=max(sizes)))
        for n in sizes:
            want = G.simulate(a[:n], G.weights(c), c["changes"], c["R"], capital=c["capital"], **sched)
            FG._check_cashflow(oracle, {k: got[f"{i}:{n}:{k}"] for k in KEYS}, want, dict(c, n=n), (c["id"], n))
            FG._same_floats(got[f"{i}:{n}:holdings"], want["holdings"], (c["id"], n))
