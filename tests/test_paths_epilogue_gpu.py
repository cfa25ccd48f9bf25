"""The chunk statistics of paths_kernel as a bit-exact contract.

Every 256-path chunk's mean and population variance come from the device's own final values, added in binary64 in one
fixed association (smmc_kernels.hip, the block after simulate_path):

    per wave of 64 lanes   v[i] += v[i + off] for off = 32, 16, 8, 4, 2, 1 (lane 0's value: ((x0 + x32) + (x16 + x48)) + ...),
                           once for the values and once for their squares; lanes beyond the launch's last path add 0
    per chunk              ((w0 + w1) + w2) + w3 over its four waves
    mean = t1 / n_in,  var = t2 / n_in - mean * mean,  var > 0 ? var : 0 (a NaN becomes 0), both rounded to binary32

with n_in the number of paths the chunk holds.  The sum of squares is not exact in binary64, so another association
gives other bits.  This file restates that in numpy and requires EQUAL BITS; the existing suites compare the chunk
statistics with the CPU oracle to 1e-6 only.  The restatement was validated against the build BEFORE the wave
reductions moved from ds_bpermute shuffles to DPP / v_permlane*_swap and the full chunk's divide became a multiply by
2^-8: it passed there unchanged, and passes on this one (profiles/angle_mask_epilogue/README.md).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
CHUNK = 256


@pytest.fixture(scope="module")
def eng(table):
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    e.set_table(table)
    yield e
    e.close()


def _tree(a):
    """Lane 0 of `for (off = 32; off > 0; off >>= 1) v += shfl_down(v, off)` over the last axis (64 lanes)."""
    for off in (32, 16, 8, 4, 2, 1):
        a = a[..., :off] + a[..., off:2 * off]
    return a[..., 0]


def kernel_chunk_stats(final):
    """(mean, variance) per chunk as binary32, from the final values, in the kernel's association."""
    n = final.size
    n_chunks = (n + CHUNK - 1) // CHUNK
    x = np.zeros(n_chunks * CHUNK, dtype=np.float64)
    x[:n] = final.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        w1 = _tree(x.reshape(n_chunks, 4, 64))
        w2 = _tree((x * x).reshape(n_chunks, 4, 64))
        t1 = ((w1[:, 0] + w1[:, 1]) + w1[:, 2]) + w1[:, 3]
        t2 = ((w2[:, 0] + w2[:, 1]) + w2[:, 2]) + w2[:, 3]
        n_in = np.minimum(CHUNK, n - CHUNK * np.arange(n_chunks)).astype(np.float64)
        mean = t1 / n_in
        var = t2 / n_in - mean * mean
        var = np.where(var > 0.0, var, 0.0)
        return mean.astype(np.float32), var.astype(np.float32)


def _check(eng, sim, what=""):
    r = eng.simulate(sim, want_final=True, want_chunk_stats=True, want_stats=True)
    final = r.final.cpu().numpy()
    mean, var = kernel_chunk_stats(final)
    got_mean, got_var = r.chunk_mean.cpu().numpy(), r.chunk_var.cpu().numpy()
    bad_m = np.flatnonzero(got_mean.view(np.uint32) != mean.view(np.uint32))
    bad_v = np.flatnonzero(got_var.view(np.uint32) != var.view(np.uint32))
    assert bad_m.size == 0, (what, "mean", bad_m[:8], got_mean[bad_m[:8]], mean[bad_m[:8]])
    assert bad_v.size == 0, (what, "variance", bad_v[:8], got_var[bad_v[:8]], var[bad_v[:8]])
    # ... and without the statistics record and the final-value store beside them (other branches of the chunk loop)
    r2 = eng.simulate(sim, want_final=False, want_chunk_stats=True)
    assert np.array_equal(r2.chunk_mean.cpu().numpy().view(np.uint32), mean.view(np.uint32)), what
    assert np.array_equal(r2.chunk_var.cpu().numpy().view(np.uint32), var.view(np.uint32)), what
    return final


# a multiple of 256; a ragged last chunk with n mod 256 in {1, 63, 64, 255}; fewer than 256 paths; fewer than 64; an odd
# (5, 1) and an even number of chunks -- of virtual blocks, while the grid is wider than the launch
SIZES = [256 * 8, 256 * 4 + 1, 256 * 5 + 63, 256 * 4 + 64, 256 * 5 + 255, 256, 200, 65, 64, 37, 1]
HIST = dict(n_bins=100, hist_lo=0.0, hist_hi=20000.0)


def _divides(mode_name):
    """(expected divide, periods, make_sim arguments): fast, range-checked and IEEE divide of the mode."""
    from stock_market_monte_carlo_amd import _lib
    if mode_name == "table":  # the bundled table: provably safe for 360 periods, not for 1000
        return ((_lib.DIV_FAST, 360, {}), (_lib.DIV_CHECKED, 1000, {}), (_lib.DIV_EXACT, 360, {"exact_div": True}))
    return ((_lib.DIV_FAST, 360, {}), (_lib.DIV_CHECKED, 360, {"gauss_mean": 2.0, "gauss_std": 9.0}),
            (_lib.DIV_EXACT, 360, {"exact_div": True}))


def _mode(mode_name):
    from stock_market_monte_carlo_amd import MODE_GAUSSIAN, MODE_TABLE
    return {"table": MODE_TABLE, "gaussian": MODE_GAUSSIAN}[mode_name]


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
@pytest.mark.parametrize("n", SIZES)
def test_chunk_statistics_have_the_bits_of_the_kernels_association(eng, mode_name, n):
    from stock_market_monte_carlo_amd import Engine
    for kind, periods, kw in _divides(mode_name):
        sim = Engine.make_sim(n, periods, _mode(mode_name), SEED, first_path=5, **HIST, **kw)
        assert eng.divide_kind(sim) == kind
        _check(eng, sim, (mode_name, n, kind))


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_many_chunks_per_virtual_block(eng, mode_name):
    """More chunks than the grid is wide: every workgroup walks several chunks (the scratch slots alternate)."""
    from stock_market_monte_carlo_amd import Engine
    vgrid, _, _ = eng.geometry()
    for n in (CHUNK * (2 * vgrid + 3) + 63, CHUNK * (3 * vgrid + 1)):
        _check(eng, Engine.make_sim(n, 9, _mode(mode_name), SEED, **HIST), (mode_name, n))


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_first_path_above_32_bits(eng, mode_name):
    from stock_market_monte_carlo_amd import Engine
    for first in ((1 << 32) - 100, (1 << 40) + 12345):  # the first one crosses 2^32 inside the launch
        for n in (256 * 40 + 3, 256 * 3, 255):
            _check(eng, Engine.make_sim(n, 36, _mode(mode_name), SEED, first_path=first, **HIST), (mode_name, first, n))


def test_halves_with_different_trip_counts(table, monkeypatch):
    """One virtual block per CU: with k vgrid + 1 chunks the first half of workgroup 0 makes one trip more than every
    other half, with k vgrid + 2 its second half takes the ragged last chunk, with 2 vgrid - 1 the last half is one
    trip short; an idle half goes through the reduction and the barrier with every lane adding 0."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import Engine
    monkeypatch.setenv("SMMC_BLOCKS_PER_CU", "1")
    e = S.Engine(0)
    try:
        e.set_table(table)
        vgrid, _, cus = e.geometry()
        assert vgrid == cus
        for n in (256 * (3 * vgrid + 1), 256 * (3 * vgrid + 1) + 7, 256 * (2 * vgrid - 1), 256 * (2 * vgrid - 2) + 1):
            for mode_name in ("gaussian", "table"):
                _check(e, Engine.make_sim(n, 9, _mode(mode_name), SEED, **HIST), (mode_name, n))
    finally:
        e.close()


def test_paths_that_overflow_to_infinity(eng):
    """A draw that grows by almost a quarter per period on average: four paths in ten pass binary32's largest number
    within 360 periods (the CPU oracle counts 1267 of 3072).  A chunk that holds one has mean inf and, inf - inf being
    NaN and a NaN not above 0, variance 0.  At a slightly lower growth only the luckiest paths get there (26 of 16384)
    and chunks with an infinite mean lie between chunks without."""
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN
    for n in (256 * 12, 256 * 7 + 63):
        sim = Engine.make_sim(n, 360, MODE_GAUSSIAN, SEED, gauss_mean=24.2, gauss_std=10.0, **HIST)
        final = _check(eng, sim, ("overflow", n))
        assert np.isinf(final).any() and np.isfinite(final).any()
        mean, var = kernel_chunk_stats(final)
        assert np.isinf(mean).all() and (var == 0).all()
    sim = Engine.make_sim(256 * 64, 360, MODE_GAUSSIAN, SEED, gauss_mean=22.8, gauss_std=10.0, **HIST)
    final = _check(eng, sim, "rare overflow")
    mean, _ = kernel_chunk_stats(final)
    assert np.isinf(mean).any() and np.isfinite(mean).any()
