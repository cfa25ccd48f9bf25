"""Regime-switching Gaussian paths (smmc_engine_simulate_regimes and its _to_host form, through
stock_market_monte_carlo_amd.regimes) on the GPU against the numpy restatement over the CPU oracle
(tests/regimes_reference.py).

Compared as bits: the final values; the chunk means and variances, against the restatement's one-pass sums in the kernels'
own association (stationary_reference.chunk_mean_var_device_order); the record's counters, minimum, maximum and every
bucket.  The record's two binary64 sums are added per lane, per wave, per workgroup and then over the launch's workgroups,
an order that follows the launch shape and that no restatement of the contract knows: they are held to the relative 1e-12
of tests/test_gpu_parity.py.  That holds for the two identities as well: smmc_engine_simulate_portfolio is a wave walk with
another launch shape, and it has no chunk statistics; its final values are compared as bits, the record as above.

Shapes: 2 * 256 + 37 paths (two full chunks and a ragged last wave), ids from 2^32 - 100 (the id crosses word 1 inside the
launch), both halves of the seed non-zero; P on both sides of the 4-period block of normals and of the 8-period segment;
regimes (0.9, 3.5) and (-1.5, 7.0), so that one wrong state changes the bits."""
import contextlib

import numpy as np
import pytest

import blocks_reference as bref
import regimes_reference as ref
import stationary_reference as sref

pytestmark = pytest.mark.gpu

N = 2 * 256 + 37
PERIODS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 360)
# mean durations (40, 8); (1, 1), which flips every period; (2, 65536 / 65535), values at the q16 edges
LEAVES = ((1638, 8192), (65536, 65536), (32768, 65535))
START = ref.stationary_start(LEAVES[0])  # the stationary share of regime 1 under mean durations (40, 8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _sim(n, P, first=ref.FIRST_PATH, exact_div=False, n_bins=ref.BINS, capital=ref.CAPITAL, seed=ref.SEED):
    import stock_market_monte_carlo_amd as S
    # gauss_mean and gauss_std are not read: values that would change every bit if they were
    return S.Engine.make_sim(n, P, S.MODE_GAUSSIAN, seed, first_path=first, initial_capital=capital, gauss_mean=-37.0, gauss_std=11.0,
                             n_bins=n_bins, hist_lo=ref.LO, hist_hi=ref.HI, below_threshold=ref.BELOW, exact_div=exact_div)


def _host(raw):
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in raw.items()}
    if out["stats_raw"] is not None:
        out["stats_raw"] = out["stats_raw"].tobytes()
    return out


def _run(eng, sim, leave, start1, means=ref.MEANS, stds=ref.STDS, final=True, chunks=True, stats=True):
    import stock_market_monte_carlo_amd as S
    raw = S.simulate_regimes_raw(eng, sim, means, stds, leave_q16=leave, start1_q16=start1, want_final=final, want_chunk_stats=chunks,
                                 want_stats=stats)
    eng.sync()
    return _host(raw)


def _check_record(raw, want, n, tag):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    st, ost = stats_from_bytes(raw), want["stats"]
    assert st.count == ost.count == n, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert np.array_equal(st.hist, want["hist"]), tag
    if n:
        assert st.min == ost.min and st.max == ost.max, tag
    if np.isfinite(ost.sumsq):
        assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag
    else:
        assert st.sum == ost.sum and st.sumsq == ost.sumsq, tag


def _check(got, want, n, tag):
    if got["final"] is not None:
        assert got["final"].size == n and np.array_equal(_bits(got["final"]), _bits(want["final"])), tag
    if got["stats_raw"] is not None:
        _check_record(got["stats_raw"], want, n, tag)
    if got["chunk_mean"] is not None:
        assert got["chunk_mean"].size == got["chunk_var"].size == -(-n // 256), tag
    if got["chunk_mean"] is not None and n:
        cm, cv = sref.chunk_mean_var_device_order(want["final"])
        assert np.array_equal(_bits(got["chunk_mean"]), _bits(cm)) and np.array_equal(_bits(got["chunk_var"]), _bits(cv)), tag
        if np.isfinite(want["final"]).all():
            assert np.allclose(cm, want["chunk_mean"], rtol=1e-6, atol=0.0), tag
            assert np.allclose(cv, want["chunk_var"], rtol=1e-5, atol=1e-6 * float(np.max(want["chunk_var"]) + 1)), tag


@pytest.mark.parametrize("P", PERIODS)
def test_against_the_restatement(eng, oracle, P):
    for leave in LEAVES:
        start1 = ref.stationary_start(leave)
        _check(_run(eng, _sim(N, P), leave, start1), ref.cached_result(oracle, N, P, leave, start1), N, (P, leave))


@pytest.mark.parametrize("n", [0, 1, 255])
def test_few_paths_and_none(eng, oracle, n):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    leave = LEAVES[0]
    got = _run(eng, _sim(n, 41), leave, START)
    _check(got, ref.cached_result(oracle, n, 41, leave, START), n, n)
    assert stats_from_bytes(got["stats_raw"]).count == n and got["final"].size == n


# ---- the identities, against the engine's own simulate_portfolio -----------------------------------------------------

def _portfolio(eng, sim, mean, std):
    raw = eng.simulate_portfolio_raw(sim, (1.0,), 0, means=(mean,), factor=((std,),), want_final=True, want_stats=True)
    eng.sync()
    return raw["final"].cpu().numpy(), raw["stats_raw"].cpu().numpy().tobytes()


def _against_portfolio(eng, oracle, got, sim, mean, std, n, tag):
    final, record = _portfolio(eng, sim, mean, std)
    assert np.array_equal(_bits(got["final"]), _bits(final)), tag
    print(tag, "record bytes equal:", got["stats_raw"] == record)
    _check_record(got["stats_raw"], bref.record_of(oracle, final, ref.BINS, ref.LO, ref.HI, ref.BELOW), n, tag)
    _check_record(record, bref.record_of(oracle, final, ref.BINS, ref.LO, ref.HI, ref.BELOW), n, tag)


@pytest.mark.parametrize("P", (1, 7, 41, 360))
def test_equal_regimes_are_one_asset(eng, oracle, P):
    """Identity 1: mean[0] == mean[1] and std[0] == std[1], with any probabilities."""
    sim = _sim(N, P)
    for leave, start1 in (((1638, 8192), START), ((65536, 65536), 32768), ((0, 0), 0), ((12345, 54321), 65536)):
        got = _run(eng, sim, leave, start1, means=(0.9, 0.9), stds=(3.5, 3.5))
        _against_portfolio(eng, oracle, got, sim, 0.9, 3.5, N, (P, leave, start1))


@pytest.mark.parametrize("P", (1, 9, 360))
def test_a_regime_never_left_is_one_asset(eng, oracle, P):
    """Identity 2: start1_q16 = 0 and leave_q16[0] = 0 is regime 0's numbers whatever regime 1 holds; start1_q16 = 65536 and
    leave_q16[1] = 0 is regime 1's."""
    sim = _sim(N, P)
    _against_portfolio(eng, oracle, _run(eng, sim, (0, 40000), 0), sim, ref.MEANS[0], ref.STDS[0], N, (P, "regime 0"))
    _against_portfolio(eng, oracle, _run(eng, sim, (40000, 0), 65536), sim, ref.MEANS[1], ref.STDS[1], N, (P, "regime 1"))


# ---- the edges of the probabilities ----------------------------------------------------------------------------------

@pytest.mark.parametrize("start1", (0, 1, 65535, 65536))
def test_the_edges_of_start1(eng, oracle, start1):
    for P in (1, 9):
        _check(_run(eng, _sim(N, P), (1638, 8192), start1), ref.cached_result(oracle, N, P, (1638, 8192), start1), N, (P, start1))


@pytest.mark.parametrize("q", (0, 1, 65535, 65536))
@pytest.mark.parametrize("side", (0, 1))
def test_the_edges_of_leave(eng, oracle, q, side):
    leave = (q, 8192) if side == 0 else (8192, q)
    _check(_run(eng, _sim(N, 41), leave, 32768), ref.cached_result(oracle, N, 41, leave, 32768), N, leave)


# ---- the divides -----------------------------------------------------------------------------------------------------

def _kind(eng, sim, leave, start1, means, stds):
    import stock_market_monte_carlo_amd as S
    return S.regimes_divide_kind(eng, sim, means, stds, leave_q16=leave, start1_q16=start1)


def test_fast_divide_on_calm_regimes(eng, oracle):
    from stock_market_monte_carlo_amd import _lib
    means, stds, leave = (0.5, -0.5), (0.8, 1.5), (1638, 8192)
    assert _kind(eng, _sim(N, 360), leave, START, means, stds) == _lib.DIV_FAST
    assert _kind(eng, _sim(N, 360, exact_div=True), leave, START, means, stds) == _lib.DIV_EXACT
    want = ref.cached_result(oracle, N, 360, leave, START, means, stds)
    _check(_run(eng, _sim(N, 360), leave, START, means, stds), want, N, "fast")
    _check(_run(eng, _sim(N, 360, exact_div=True), leave, START, means, stds), want, N, "fast, exact")


def test_exact_divide_without_a_positive_lower_bound(eng, oracle):
    """Regime 1 with 100 - 1.5 - 7 * 15 < 0: no bounds that keep its multiplier positive."""
    from stock_market_monte_carlo_amd import _lib
    means, stds, leave = (0.9, -1.5), (3.5, 15.0), (1638, 8192)
    assert _kind(eng, _sim(N, 97), leave, START, means, stds) == _lib.DIV_EXACT
    with np.errstate(all="ignore"):
        _check(_run(eng, _sim(N, 97), leave, START, means, stds), ref.cached_result(oracle, N, 97, leave, START, means, stds), N, "exact")


CRASH = dict(means=(0.5, -40.0), stds=(1.0, 8.0), leave=(328, 656), start1=21845, P=360, n=2048)


def test_redo_of_paths_that_leave_the_checked_window(eng, oracle):
    """A calm regime and one that loses 40 % a period with deviation 8: the union of the bounds is [3.999, 116.001], so the
    window is [2^(-88 + 7 log2(100 / 3.999)), 2^(126 - 7 log2 1.16001 - log2 116.001)] (divide_kind, smmc_capi.cpp).  Part of
    the paths, not all, are outside it at one of the kernel's tests (after periods 8, 16, ...) and are redone with the IEEE
    divide: asserted on the restatement before the device is asked."""
    from stock_market_monte_carlo_amd import _lib
    c = CRASH
    sim = _sim(c["n"], c["P"])
    lo_a, hi_a = 100.0 - 40.0 - 7.0 * float(np.nextafter(np.float32(8.0), np.float32(np.inf))) - 1e-3, 100.0 - 40.0 + 56.0 + 1e-3
    hi_a = max(hi_a, 100.5 + 7.0 * float(np.nextafter(np.float32(1.0), np.float32(np.inf))) + 1e-3)
    lo = np.float32(2.0 ** (-88.0 + 7.0 * np.log2(100.0 / lo_a)))
    hi = np.float32(2.0 ** (126.0 - 7.0 * max(0.0, np.log2(hi_a / 100.0)) - np.log2(hi_a)))
    at = ref.values_at_window_tests(oracle, ref.SEED, ref.FIRST_PATH, c["n"], c["P"], c["means"], c["stds"], c["leave"], c["start1"])
    left = (~((at > lo) & (at < hi))).any(axis=1)
    print(f"crash case: window [{lo:g}, {hi:g}], {left.mean():.3f} of the paths leave it")
    assert 0.0 < left.mean() < 1.0
    assert _kind(eng, sim, c["leave"], c["start1"], c["means"], c["stds"]) == _lib.DIV_CHECKED
    want = ref.cached_result(oracle, c["n"], c["P"], c["leave"], c["start1"], c["means"], c["stds"])
    with np.errstate(all="ignore"):
        _check(_run(eng, sim, c["leave"], c["start1"], c["means"], c["stds"]), want, c["n"], "checked")
        _check(_run(eng, _sim(c["n"], c["P"], exact_div=True), c["leave"], c["start1"], c["means"], c["stds"]), want, c["n"], "exact")


# ---- the chunk walk --------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _one_block_per_cu(monkeypatch):
    """An engine whose grid is one workgroup per compute unit (the knob is read when the engine is made)."""
    import stock_market_monte_carlo_amd as S
    monkeypatch.setenv("SMMC_BLOCKS_PER_CU", "1")
    e = S.Engine(0)
    try:
        grid, _, cus = e.geometry()
        assert grid == cus  # host_enqueue_paths caps its grid at this
        yield e, cus
    finally:
        e.close()


def test_when_workgroups_walk_several_chunks(oracle, monkeypatch):
    """The chunk walk and its alternating reduction slots under this walk: with 3 vgrid + 2 chunks workgroups 0 and 1 make a
    fourth trip, the second on a last chunk of 7 paths; with 2 vgrid - 1 the last workgroup is one trip short; with 2 vgrid -
    2 + 1 the last is, and the one before it ends on a chunk of one path."""
    leave = LEAVES[0]
    with _one_block_per_cu(monkeypatch) as (eng, cus):
        sizes = [256 * (3 * cus + 1) + 7, 256 * (2 * cus - 1), 256 * (2 * cus - 2) + 1]
        final = ref.finals_bulk(oracle, ref.SEED, ref.FIRST_PATH, max(sizes), 41, ref.MEANS, ref.STDS, leave, START)
        for n in sizes:
            _check(_run(eng, _sim(n, 41), leave, START), bref.record_of(oracle, final[:n]), n, n)


# ---- the host form, prefixes, fuzz -----------------------------------------------------------------------------------

def test_to_host_against_the_device_result(oracle, monkeypatch):
    """1000 paths through chunks of 256 into a pageable buffer: the device call's values, merged record and chunks."""
    import stock_market_monte_carlo_amd as S
    monkeypatch.setenv("SMMC_HOST_CHUNK_PATHS", "256")
    eng = S.Engine(0)  # the knobs are read when an engine is created
    try:
        n, leave, sim = 1000, LEAVES[0], _sim(1000, 41)
        dev = _run(eng, sim, leave, START)
        host, st, (cm, cv) = S.simulate_regimes_to_host(eng, sim, ref.MEANS, ref.STDS, leave_q16=leave, start1_q16=START,
                                                        out=np.full(n, -1.0, dtype=np.float32), want_stats=True, want_chunk_stats=True)
        want = ref.cached_result(oracle, n, 41, leave, START)
        assert np.array_equal(_bits(host), _bits(dev["final"])) and np.array_equal(_bits(host), _bits(want["final"]))
        ost = want["stats"]
        assert (st.count, st.below, st.underflow, st.overflow) == (n, ost.below, ost.underflow, ost.overflow)
        assert st.min == ost.min and st.max == ost.max and np.array_equal(st.hist, want["hist"])
        assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12)
        # chunks of 256 paths are the chunk statistics' own groups: the device call's bits
        assert np.array_equal(_bits(cm), _bits(dev["chunk_mean"])) and np.array_equal(_bits(cv), _bits(dev["chunk_var"]))
        # mean durations (40, 8) are leave_q16 (1638, 8192); their stationary share of regime 1 is START / 65536
        plain, none, (no_cm, no_cv) = S.simulate_regimes_to_host(eng, sim, ref.MEANS, ref.STDS, mean_durations=(40, 8))
        assert none is None and no_cm is None and no_cv is None and np.array_equal(_bits(plain), _bits(host))
    finally:
        eng.close()


def test_the_first_paths_of_a_longer_run(eng):
    """A path does not depend on n_paths: the first n final values of a run of 1000 are the run of n."""
    whole = _run(eng, _sim(1000, 41), LEAVES[0], START, chunks=False, stats=False)["final"]
    for n in (1, 255, 300, 512):
        assert np.array_equal(_bits(_run(eng, _sim(n, 41), LEAVES[0], START, chunks=False, stats=False)["final"]), _bits(whole[:n])), n


def test_the_first_periods_of_a_longer_run(eng, oracle):
    """Identity 3 on the device, through the restatement's multipliers: the value after P' periods of the P-period request's
    draws is the P'-period request."""
    leave = LEAVES[0]
    a = ref.multipliers(oracle, ref.SEED, ref.FIRST_PATH, N, 33, ref.MEANS, ref.STDS, leave, START)
    for p in (1, 7, 8, 9, 17):
        v = np.full(N, ref.CAPITAL, np.float32)
        for t in range(p):
            v = (v * a[:, t]) / np.float32(100.0)
        assert np.array_equal(_bits(_run(eng, _sim(N, p), leave, START, chunks=False, stats=False)["final"]), _bits(v)), p


def _fuzz_cases():
    rng = np.random.default_rng(0x2E61)
    out = []
    for i in range(40):
        q = lambda: int(rng.choice([int(rng.integers(0, 65537)), int(rng.integers(0, 65537)), 0, 65536, int(rng.integers(1, 64))]))  # noqa: E731
        out.append(dict(leave=(q(), q()), start1=q(), means=(float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3))),
                        stds=(float(rng.uniform(0, 9)), float(rng.uniform(0, 9))), P=int(rng.integers(1, 401)), n=int(rng.integers(1, 2001)),
                        seed=int(rng.integers(1, 1 << 63)) * 2 + int(rng.integers(0, 2)), first=int(rng.integers(0, 1 << 62))))
    return out


FUZZ = _fuzz_cases()


@pytest.mark.parametrize("c", FUZZ, ids=["l%d-%d-s%d-P%d-n%d" % (c["leave"] + (c["start1"], c["P"], c["n"])) for c in FUZZ])
def test_seeded_fuzz(eng, oracle, c):
    want = ref.result(oracle, c["n"], c["P"], c["leave"], c["start1"], c["means"], c["stds"], seed=c["seed"], first_path=c["first"])
    got = _run(eng, _sim(c["n"], c["P"], first=c["first"], seed=c["seed"]), c["leave"], c["start1"], c["means"], c["stds"])
    _check(got, want, c["n"], c)


def test_refusals_on_the_device(eng):
    import stock_market_monte_carlo_amd as S
    with pytest.raises(S.SmmcError, match="SMMC_MODE_GAUSSIAN"):
        S.simulate_regimes(eng, S.Engine.make_sim(10, 5, S.MODE_TABLE, 1), ref.MEANS, ref.STDS, leave_q16=(1, 1), start1_q16=0)
    with pytest.raises(S.SmmcError, match="V2"):
        S.simulate_regimes(eng, S.Engine.make_sim(10, 5, S.MODE_GAUSSIAN, 1, stream=2), ref.MEANS, ref.STDS, leave_q16=(1, 1), start1_q16=0)
    with pytest.raises(ValueError):
        S.simulate_regimes(eng, _sim(10, 5), ref.MEANS, ref.STDS, leave_q16=(65537, 1), start1_q16=0)
    with pytest.raises(ValueError):
        S.simulate_regimes(eng, _sim(10, 5), ref.MEANS, ref.STDS)
    with pytest.raises(ValueError):
        S.simulate_regimes(eng, _sim(10, 5), ref.MEANS, ref.STDS, leave_q16=(0, 0))
