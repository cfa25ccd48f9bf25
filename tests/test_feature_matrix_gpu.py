"""Every instantiation of the seven feature-kernel families on the device against its restatement: one case per row of
the ledger (tests/feature_matrix.py: ROWS), and the EXTREME cases whose inputs tell the fast divide from the IEEE one.

Before a run is trusted the host's choice is asked for (Engine.divide_kind, cashflow_divide_kind,
cashflow_sweep_divide_kind, blocks_divide_kind, portfolio_divide_kind, portfolio_cashflow_divide_kind) and must be the
kind the ledger claims.  The comparison is each family's own: per-path outputs, integer counters, per-period counts,
buckets, min and max on their bits; the two double sums to the relative 1e-12 against math.fsum of the restated values
and of their squares; float outputs that are NaN on being NaN (payloads are no part of any contract).

Evidence that these tests bite.  Each variant was built with tools/variant_build.py (a patched scratch copy of csrc/,
never the product sources; tools/variant_build.sh takes macros only and compiles an older file list), loaded through
SMMC_LIB, and run once on the device:
- div100<true> (csrc/smmc_device.h) made to run the fast form -- EVERY exact-divide instantiation, those of
  portfolio_kernel and portfolio_cashflow_kernel among them, then silently runs the fast divide: the 13 "-extreme" cases
  of this file failed (every family, both modes); the 126 ledger rows, the flag on a tame table among them, passed.
- Two rungs returning a neighbour, in one build: PortfolioFamily::get's case 3 returning the K = 2 kernel (K = 3 -> 4 or
  a sweep width 4 -> 8 would write past the request's buffers or LDS; 3 -> 2 reads and writes inside them), and
  CashflowFamily::get returning the constant-schedule kernel for a per-period schedule.  Failed: the six
  portfolioI..Li3EE rows, the six cashflowI..Lb1EE rows and the two per-period "-extreme" cash-flow cases; the other 125
  cases passed.  (tests/test_cashflow_gpu.py's "arrays" cases and tests/test_portfolio_gpu.py's K = 3 cases fail too.)
- portfolio_kernel's high id word masked to its low two bits: every case here and all of tests/test_portfolio_gpu.py
  passed (their ids are 2^32 - 100 ..); tests/test_feature_fuzz_gpu.py::test_random_portfolios failed, first at case 5.
On the device the 139 cases take 19 s together, 0.3 s at most each but the first (2 s: the library's load)."""
import math

import numpy as np
import pytest

import feature_matrix as M

pytestmark = pytest.mark.gpu


def _ids(family):
    return [c["id"] for c in M.rows_of(family)]


@pytest.fixture(scope="module")
def engines():
    """One engine per table, made on first use."""
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(c):
        portfolio = c["family"] in ("portfolio_kernel", "portfolio_cashflow_kernel")
        key = ("gauss",) if c["mode"] == "gauss" else (portfolio, c["T"], c["K"] if portfolio else 0, c["extreme"], c["exact"] == "window")
        if key not in made:
            made[key] = S.Engine(0)
            if c["mode"] == "table":
                if portfolio:
                    made[key].set_asset_table(M.assets(c))
                else:
                    made[key].set_table(M.series(c))
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _sim(c):
    import stock_market_monte_carlo_amd as S
    bins, lo, hi, below = M.hist_range(c)
    kw = {}
    if c["mode"] == "gauss" and c["family"] not in ("portfolio_kernel", "portfolio_cashflow_kernel"):
        kw = dict(zip(("gauss_mean", "gauss_std"), M.gauss_law(c)))
    return S.Engine.make_sim(c["n"], c["P"], S.MODE_GAUSSIAN if c["mode"] == "gauss" else S.MODE_TABLE, c.get("seed", M.SEED), first_path=c.get("first", M.FIRST_PATH),
                             initial_capital=c["capital"], n_bins=bins, hist_lo=lo, hist_hi=hi, below_threshold=below,
                             exact_div=c["exact"] == "flag", **kw)


def _same_floats(got, want, tag):
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


def _check_record(oracle, st, values, c, tag, stats_range=None):
    bins, lo, hi, below = stats_range or M.hist_range(c)
    values = np.ascontiguousarray(values, dtype=np.float32)
    ost, ohist = oracle.values_stats(values, below, bins, lo, hi)
    assert st.count == ost.count == values.size, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    _same_floats([st.min, st.max], [ost.min, ost.max], tag)  # on their bits: -0.0 is not +0.0
    assert np.array_equal(st.hist, ohist) and (not bins or int(st.hist.sum()) + st.underflow + st.overflow == values.size), tag
    d = values.astype(np.float64)
    with np.errstate(all="ignore"):
        _same_sum(st.sum, _fsum(d.tolist()), tag)
        _same_sum(st.sumsq, _fsum((d * d).tolist()), tag)


def _kind(got, c):
    if c["kind"] is None:  # a fuzz case claims none
        return
    assert got == c["kind"], f"{c['id']}: the host chose divide kind {got}, the ledger claims {c['kind']}"


def _portfolio_args(c):
    if c["mode"] != "gauss":
        return {}
    means, factor = M.gauss_portfolio(c)
    return {"means": means, "factor": factor}


@pytest.mark.parametrize("c", M.rows_of("checkpoints_kernel"), ids=_ids("checkpoints_kernel"))
def test_checkpoints(oracle, engines, c):
    check_checkpoints(oracle, engines(c), c)


def check_checkpoints(oracle, eng, c):
    sim, want = _sim(c), M.reference(oracle, c)
    _kind(eng.divide_kind(sim, keepdata=True), c)
    stats, final = eng.simulate_checkpoints(sim, want["args"], want_final=True)
    assert len(stats) == len(want["args"])
    for st, p in zip(stats, want["args"]):
        _check_record(oracle, st, want["traj"][:, p], c, (c["id"], p))
    _same_floats(final.cpu().numpy(), want["traj"][:, c["P"]], c["id"])


@pytest.mark.parametrize("c", M.rows_of("excursions_kernel"), ids=_ids("excursions_kernel"))
def test_excursions(oracle, engines, c):
    check_excursions(oracle, engines(c), c)


def check_excursions(oracle, eng, c):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    import excursions_reference as xref
    sim, want = _sim(c), M.reference(oracle, c)
    _kind(eng.divide_kind(sim, keepdata=True), c)
    names = xref.FIELDS + ("stats", "drawdown_stats", "first_below_at", "first_reach_at")
    raw = eng.simulate_excursions_raw(sim, *want["args"], xref.DD_THRESHOLD, **{"want_" + k: True for k in names})
    eng.sync()
    out = {k: t.cpu().numpy() for k, t in raw.items()}
    for k in ("final", "peak", "low", "drawdown"):
        _same_floats(out[k], want[k], (c["id"], k))
    for k in ("drawdown_period", "underwater", "first_below", "first_reach"):
        assert np.array_equal(out[k].view(np.uint32), want[k]), (c["id"], k)
    for k in ("first_below_at", "first_reach_at"):
        assert np.array_equal(out[k].view(np.uint64), want[k]) and int(out[k].sum()) == c["n"], (c["id"], k)
    _check_record(oracle, stats_from_bytes(out["stats"].tobytes()), want["final"], c, (c["id"], "stats"))
    _check_record(oracle, stats_from_bytes(out["drawdown_stats"].tobytes()), want["drawdown"], c, (c["id"], "drawdown_stats"),
                  (M.hist_range(c)[0], 0.0, 1.0, xref.DD_THRESHOLD))


def _check_cashflow(oracle, out, want, c, tag):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    _same_floats(out["final"], want["final"], tag)
    _same_floats(out["paid"], want["paid"], tag)
    assert np.array_equal(out["ruin_period"].view(np.uint32), want["ruin_period"]), tag
    dep = out["depleted_at"].view(np.uint64)
    assert dep.size == c["P"] + 1 and int(dep.sum()) == c["n"] and np.array_equal(dep, want["depleted_at"]), tag
    _check_record(oracle, stats_from_bytes(out["stats_raw"].tobytes()), want["final"], c, tag)


ALL = dict(want_final=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)


@pytest.mark.parametrize("c", M.rows_of("cashflow_kernel"), ids=_ids("cashflow_kernel"))
def test_cashflow(oracle, engines, c):
    check_cashflow(oracle, engines(c), c)


def check_cashflow(oracle, eng, c):
    sim, want = _sim(c), M.reference(oracle, c)
    _kind(eng.cashflow_divide_kind(sim, **want["args"]), c)
    raw = eng.simulate_cashflow_raw(sim, **want["args"], **ALL)
    eng.sync()
    _check_cashflow(oracle, {k: t.cpu().numpy() for k, t in raw.items()}, want, c, c["id"])


@pytest.mark.parametrize("c", M.rows_of("cashflow_sweep_kernel"), ids=_ids("cashflow_sweep_kernel"))
def test_cashflow_sweep(oracle, engines, c):
    check_cashflow_sweep(oracle, engines(c), c)


def check_cashflow_sweep(oracle, eng, c):
    sim, want = _sim(c), M.reference(oracle, c)
    am, fr, fl = ([sc[i] for sc in want["args"]] for i in range(3))
    assert len(set(want["args"])) == len(want["args"]) == c["S"]  # distinct scenarios
    _kind(eng.cashflow_sweep_divide_kind(sim, am, fr, fl), c)
    raw = eng.simulate_cashflow_sweep_raw(sim, am, fr, fl, **ALL)
    eng.sync()
    out = {k: t.cpu().numpy() for k, t in raw.items()}
    assert out["final"].shape == (c["S"], c["n"]) and out["depleted_at"].shape == (c["S"], c["P"] + 1)
    for s, one in enumerate(want["scenarios"]):
        _check_cashflow(oracle, {k: v[s] for k, v in out.items()}, one, c, (c["id"], s))


@pytest.mark.parametrize("c", M.rows_of("blocks_kernel"), ids=_ids("blocks_kernel"))
def test_blocks(oracle, engines, monkeypatch, c):
    monkeypatch.setenv("SMMC_BLOCKS_READ", c["read"])
    check_blocks(oracle, engines(c), c)


def check_blocks(oracle, eng, c):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    sim, want = _sim(c), M.reference(oracle, c)
    _kind(eng.blocks_divide_kind(sim, c["L"]), c)
    raw = eng.simulate_blocks_raw(sim, c["L"], want_final=True, want_chunk_stats=True, want_stats=True)
    eng.sync()
    _same_floats(raw["final"].cpu().numpy(), want["final"], c["id"])
    _check_record(oracle, stats_from_bytes(raw["stats_raw"].cpu().numpy().tobytes()), want["final"], c, c["id"])
    if np.isfinite(want["final"]).all() and not c["extreme"] and c["n"]:  # the chunk statistics to the 1e-6 / 1e-5 of tests/test_blocks_gpu.py
        cm, cv = oracle.chunk_mean_var(want["final"])
        assert np.allclose(raw["chunk_mean"].cpu().numpy(), cm, rtol=1e-6, atol=0.0), c["id"]
        assert np.allclose(raw["chunk_var"].cpu().numpy(), cv, rtol=1e-5, atol=1e-6 * float(np.max(cv) + 1)), c["id"]


@pytest.mark.parametrize("c", M.rows_of("portfolio_kernel"), ids=_ids("portfolio_kernel"))
def test_portfolio(oracle, engines, c):
    check_portfolio(oracle, engines(c), c)


def check_portfolio(oracle, eng, c):
    sim, want = _sim(c), M.reference(oracle, c)
    w, g = M.weights(c), _portfolio_args(c)
    _kind(eng.portfolio_divide_kind(sim, w, want["args"], **g), c)
    r = eng.simulate_portfolio(sim, w, want["args"], want_holdings=True, want_stats=True, **g)
    _same_floats(r.final.cpu().numpy(), want["final"], c["id"])
    _same_floats(r.holdings.cpu().numpy(), want["holdings"], c["id"])
    _check_record(oracle, r.stats, want["final"], c, c["id"])


@pytest.mark.parametrize("c", M.rows_of("portfolio_cashflow_kernel"), ids=_ids("portfolio_cashflow_kernel"))
def test_portfolio_cashflow(oracle, engines, c):
    check_portfolio_cashflow(oracle, engines(c), c)


def check_portfolio_cashflow(oracle, eng, c):
    sim, want = _sim(c), M.reference(oracle, c)
    w, g = M.weights(c), _portfolio_args(c)
    R, sched = want["args"]
    _kind(eng.portfolio_cashflow_divide_kind(sim, w, R, **sched, **g), c)
    raw = eng.simulate_portfolio_cashflow_raw(sim, w, R, **sched, **g, want_holdings=True, want_paid=True, want_ruin_period=True,
                                              want_stats=True, want_depleted_at=True)
    eng.sync()
    out = {k: t.cpu().numpy() for k, t in raw.items() if k != "n_assets"}
    _check_cashflow(oracle, out, want, c, c["id"])
    _same_floats(out["holdings"], want["holdings"], c["id"])
