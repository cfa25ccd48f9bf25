"""Counter stream v3's Gaussian paths_kernel runs 512-thread workgroups made of two 256-thread virtual blocks that
share one staged copy of the draw tables (smmc_kernels.hip, paths_halves).  The halves share the workgroup's barriers,
so the launches here are the ones in which a half has nothing to do while the other works: one virtual block (the
second half idle), an odd number of them, and more chunks than virtual blocks so that the halves of a workgroup make a
different number of trips.  Final values, the statistics record and the block means against the CPU oracle, compared
as tests/test_gpu_parity.py compares them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SIZES = [1, 255, 256, 257, 511, 513, 256 * 3, 256 * 16385 + 7]
HIST = dict(n_bins=100, hist_lo=0.0, hist_hi=20000.0)


@pytest.fixture(scope="module")
def eng():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _periods(n):
    return 360 if n <= 1024 else 9  # the large launches are about the chunk walk, and the oracle runs on the CPU


def _oracle(oracle, n, p, first=0, **kw):
    return oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, p, n, SEED, first_path=first, **kw))


def _same_bits(got, want):
    return np.array_equal(np.asarray(got).view(np.uint32), want.view(np.uint32))


def _check_stats(st, o, n, with_hist):
    os_ = o["stats"]
    assert st.count == n == os_.count
    assert (st.below, st.underflow, st.overflow) == (os_.below, os_.underflow, os_.overflow)
    if with_hist:
        assert np.array_equal(st.hist, o["hist"])
        assert int(st.hist.sum()) + st.underflow + st.overflow == n
    assert st.min == os_.min and st.max == os_.max
    assert st.sum == pytest.approx(os_.sum, rel=1e-12)
    assert st.sumsq == pytest.approx(os_.sumsq, rel=1e-12)


def _check_chunks(r, o, oracle):
    cm, cv = oracle.chunk_mean_var(o["final"])
    np.testing.assert_allclose(r.chunk_mean.cpu().numpy(), cm, rtol=1e-6)
    np.testing.assert_allclose(r.chunk_var.cpu().numpy(), cv, rtol=1e-5, atol=1e-6 * float(np.max(cv) + 1))


@pytest.mark.parametrize("n", SIZES)
def test_everything_at_once(eng, oracle, n):
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN
    p = _periods(n)
    r = eng.simulate(Engine.make_sim(n, p, MODE_GAUSSIAN, SEED, **HIST), want_final=True, want_chunk_stats=True,
                     want_stats=True)
    st = eng.read_stats(r.stats_raw)
    o = _oracle(oracle, n, p, **HIST)
    assert _same_bits(r.final.cpu().numpy(), o["final"])
    _check_stats(st, o, n, True)
    _check_chunks(r, o, oracle)


@pytest.mark.parametrize("n", SIZES)
def test_without_chunk_statistics_and_histogram(eng, oracle, n):
    """No block means: the chunk loop has no barrier at all; no histogram: nothing shared between the halves."""
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN
    p = _periods(n)
    o = _oracle(oracle, n, p)
    plain = eng.simulate(Engine.make_sim(n, p, MODE_GAUSSIAN, SEED))
    assert _same_bits(plain.final.cpu().numpy(), o["final"])
    r = eng.simulate(Engine.make_sim(n, p, MODE_GAUSSIAN, SEED), want_final=True, want_stats=True)
    assert _same_bits(r.final.cpu().numpy(), o["final"])
    _check_stats(eng.read_stats(r.stats_raw), o, n, False)
    r = eng.simulate(Engine.make_sim(n, p, MODE_GAUSSIAN, SEED), want_final=True, want_chunk_stats=True)
    assert _same_bits(r.final.cpu().numpy(), o["final"])
    _check_chunks(r, o, oracle)


@pytest.mark.parametrize("n", SIZES)
def test_statistics_only(eng, oracle, n):
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN
    p = _periods(n)
    r = eng.simulate(Engine.make_sim(n, p, MODE_GAUSSIAN, SEED, **HIST), want_final=False, want_stats=True)
    assert r.final is None
    _check_stats(eng.read_stats(r.stats_raw), _oracle(oracle, n, p, **HIST), n, True)


@pytest.mark.parametrize("n", SIZES[:-1] + [256 * 40 + 3])
def test_first_path_above_32_bits(eng, oracle, n):
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN
    for first in ((1 << 32) - 100, (1 << 40) + 12345):  # the first one crosses 2^32 inside the launch
        r = eng.simulate(Engine.make_sim(n, 36, MODE_GAUSSIAN, SEED, first_path=first, **HIST), want_final=True,
                         want_chunk_stats=True, want_stats=True)
        o = _oracle(oracle, n, 36, first=first, **HIST)
        assert _same_bits(r.final.cpu().numpy(), o["final"]), first
        _check_stats(eng.read_stats(r.stats_raw), o, n, True)
        _check_chunks(r, o, oracle)


@pytest.mark.parametrize("n", SIZES[:-1] + [256 * 40 + 3])
def test_all_three_divides(eng, oracle, n):
    """Reciprocal-multiply, range-checked (a draw wide enough that the window cannot be proven) and IEEE divide."""
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN, _lib
    for kind, kw in ((_lib.DIV_FAST, {}), (_lib.DIV_CHECKED, {"gauss_mean": 2.0, "gauss_std": 9.0}),
                     (_lib.DIV_EXACT, {"exact_div": True})):
        sim = Engine.make_sim(n, 360, MODE_GAUSSIAN, SEED, first_path=5, **HIST, **kw)
        assert eng.divide_kind(sim) == kind
        r = eng.simulate(sim, want_final=True, want_chunk_stats=True, want_stats=True)
        okw = {k: v for k, v in kw.items() if k != "exact_div"}
        o = _oracle(oracle, n, 360, first=5, **HIST, **okw)
        assert _same_bits(r.final.cpu().numpy(), o["final"]), kind
        _check_stats(eng.read_stats(r.stats_raw), o, n, True)
        _check_chunks(r, o, oracle)


def test_halves_with_different_trip_counts_on_a_small_grid(oracle, monkeypatch):
    """One virtual block per CU (SMMC_BLOCKS_PER_CU, read when the engine is made): every workgroup walks many chunks,
    and with a chunk count of k vgrid + 1 the first half of workgroup 0 makes one trip more than every other half;
    with k vgrid + 2 its second half takes a ragged last chunk."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN
    monkeypatch.setenv("SMMC_BLOCKS_PER_CU", "1")
    e = S.Engine(0)
    try:
        vgrid, _, cus = e.geometry()
        assert vgrid == cus
        for n in (256 * (3 * vgrid + 1), 256 * (3 * vgrid + 1) + 7, 256 * (2 * vgrid - 1)):
            r = e.simulate(Engine.make_sim(n, 9, MODE_GAUSSIAN, SEED, **HIST), want_final=True, want_chunk_stats=True,
                           want_stats=True)
            o = _oracle(oracle, n, 9, **HIST)
            assert _same_bits(r.final.cpu().numpy(), o["final"]), n
            _check_stats(e.read_stats(r.stats_raw), o, n, True)
            _check_chunks(r, o, oracle)
    finally:
        e.close()
