"""The device's draws from CHOSEN words (smmc_engine_selftest_draws -> draw_words_kernel -> the path kernels' own
stage_tables, bm3_issue / bm3_finish, bm_issue / bm_finish, digits4 and the sparse draw): every radius bin, angle
sector and table entry of both Gaussian streams that a word can reach, and every digit boundary of the table draws,
instead of the few a seed happens to give.  The sets and the references are those of tests/draw_words.py, which
tests/test_draw_words_cpu.py validates with the oracle alone (coverage: 464 of 512 v3 bins -- the rest hold no
integer --, 2048 sectors, 898 of 1056 v2 radius entries, 256 v2 angle entries).

Every launch is compared twice: bit for bit with oracle.multipliers_of_words, and with the float64 / big-integer
references under the bounds the CPU file asserts for the oracle, so that an error shared by the oracle and the
kernels' tables cannot pass through staging alone.

Measured on an MI355X: the device's bits equal the oracle's everywhere, so its largest errors are the oracle's:
0.71 of the bound for stream v3 (5.6e-5 at std 9, bound 7.9e-5), 0.50 for v2 (3.8e-6, bound 7.6e-6)."""
import ctypes as C
import functools

import numpy as np
import pytest

import draw_words as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gauss_refs():
    return {(stream, name): W.gauss_reference(w, stream) for stream in (3, 2) for name, w in W.gauss_sets(stream).items()}


def _gauss_sim(mean, std, stream, **kw):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(1, 1, S.MODE_GAUSSIAN, 0, gauss_mean=mean, gauss_std=std, stream=stream, **kw)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("stream", [3, 2])
@pytest.mark.parametrize("mean,std", W.GAUSS_PARAMS)
def test_gaussian_draws_of_every_bin_and_sector(eng, oracle, gauss_refs, mean, std, stream, form):
    p = oracle.make_params(oracle.MODE_GAUSSIAN, 1, 1, 0, gauss_mean=mean, gauss_std=std, stream=stream)
    for name, w in W.gauss_sets(stream).items():
        got = eng.selftest_draws(_gauss_sim(mean, std, stream), w, form=form)
        assert got.shape == (w.shape[0], 4)
        want = oracle.multipliers_of_words(p, w)
        err, bound = W.gauss_error(got, w, stream, mean, std, gauss_refs[stream, name])
        print(f"stream v{stream} form {form} {name} mean {mean} std {std}: max error {err.max():.3g}, "
              f"{float((err / bound).max()):.3f} of the bound; {int((got.view(np.uint32) != want.view(np.uint32)).sum())} "
              f"of {got.size} draws differ from the oracle")
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (name, bad[:4].tolist(), [hex(int(x)) for x in w[bad[0][0]]])
        assert np.all(err <= bound), (name, int(np.argmax(err / bound)))


@functools.lru_cache(maxsize=None)
def _table_case(T):
    w = W.table_words(T)
    return w, W.table_reference(w, T)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("stream", [3, 2])
@pytest.mark.parametrize("T", W.TABLE_LENGTHS)
def test_table_draws_of_every_digit_boundary(eng, oracle, T, stream, form):
    import stock_market_monte_carlo_amd as S
    eng.set_table(W.index_table(T))  # set_table accepts every length of the list (1 .. SMMC_MAX_TABLE): none is dropped
    w, want_idx = _table_case(T)
    got = eng.selftest_draws(S.Engine.make_sim(1, 1, S.MODE_TABLE, 0, stream=stream), w, form=form)
    assert got.shape == want_idx.shape == (w.shape[0], 8 if T <= 2048 else 4)
    p = oracle.make_params(oracle.MODE_TABLE, 1, 1, 0, table=W.index_table(T), stream=stream)
    assert np.array_equal(got.view(np.uint32), oracle.multipliers_of_words(p, w).view(np.uint32))
    idx = got.astype(np.float64) - 100.0
    assert np.array_equal(idx, want_idx.astype(np.float64)) and idx.max() == T - 1 and idx.min() == 0


def test_invariants(eng, oracle):
    sim = _gauss_sim(0.5, 0.83333, 3)
    a = W.gauss_v3_angle()
    got = eng.selftest_draws(sim, a).view(np.uint32)
    blocks = got[:, :2].reshape(4, 4, -1, 2)  # [first word][top two bits][sector and residual]
    assert blocks.shape[2] == 3 * 2048
    for t in range(1, 4):
        assert np.array_equal(blocks[:, 0], blocks[:, t])  # the top two bits of the angle word change nothing
    # u = 1/2 from either side: one radius (and here one angle)
    w = np.array([[0x7FFFFFFF, 5, 0x7FFFFFC0, 5], [0x80000000, 5, 0x7FFFFFFF, 5]], dtype=np.uint32)
    m = eng.selftest_draws(_gauss_sim(0.0, 1.0, 3), w).view(np.uint32).reshape(4, 2)
    assert np.all(m == m[0])
    # the two forms agree, an odd count too, and nothing is written past the items
    for stream, w in ((3, W.gauss_v3_radius()[:4097]), (2, W.gauss_v2_radius()[:4097])):
        s = _gauss_sim(-3.0, 9.0, stream)
        one, two = eng.selftest_draws(s, w, form=0), eng.selftest_draws(s, w, form=1)
        assert w.shape[0] % 2 == 1 and np.array_equal(one.view(np.uint32), two.view(np.uint32))
        assert np.array_equal(eng.selftest_draws(s, w[:1], form=1).view(np.uint32), one[:1].view(np.uint32))
    # n = 0: OK, the width is reported, the buffers are not touched
    out = np.full(8, 7.0, dtype=np.float32)
    draws = C.c_uint32(99)
    L = eng._L
    assert L.smmc_engine_selftest_draws(eng._h, C.byref(sim), None, 0, 1, out.ctypes.data_as(C.c_void_p), C.byref(draws)) == 0
    assert draws.value == 4 and np.all(out == 7.0)
    assert eng.selftest_draws(sim, np.zeros((0, 4), dtype=np.uint32)).shape == (0, 4)


def test_argument_errors(eng):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import _lib
    L = eng._L
    w = np.zeros((2, 4), dtype=np.uint32)
    out = np.zeros((2, 8), dtype=np.float32)
    wp, op = w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    eng.set_table(W.index_table(3))
    with pytest.raises(_lib.SmmcError, match="SMMC_FLAG_STREAM_REF"):
        eng.selftest_draws(S.Engine.make_sim(1, 1, S.MODE_TABLE, 0, stream="ref"), w)
    sim = _gauss_sim(0.5, 0.83333, 3)
    assert L.smmc_engine_selftest_draws(eng._h, C.byref(sim), None, 2, 0, op, None) == -1
    assert L.smmc_engine_selftest_draws(eng._h, C.byref(sim), wp, 2, 0, None, None) == -1
    assert L.smmc_engine_selftest_draws(eng._h, C.byref(sim), wp, 2, 2, op, None) == -1
    assert L.smmc_engine_selftest_draws(None, C.byref(sim), wp, 2, 0, op, None) == -1
    assert L.smmc_engine_selftest_draws(eng._h, None, wp, 2, 0, op, None) == -1
    sim.struct_size -= 4
    assert L.smmc_engine_selftest_draws(eng._h, C.byref(sim), wp, 2, 0, op, None) == -1
    assert b"struct_size" in L.smmc_last_error()
    assert np.all(out == 0.0)
    with pytest.raises(ValueError):
        eng.selftest_draws(_gauss_sim(0.5, 0.83333, 3), np.zeros((2, 3), dtype=np.uint32))


@pytest.mark.parametrize("mode_name", ["gaussian", "gaussian_v2", "table", "table_v2", "table2049"])
def test_the_path_kernels_draw_what_the_self_test_draws(oracle, table, mode_name):
    """2000 paths x 36 periods: the Philox words of every block from the oracle, through selftest_draws, compounded
    with oracle.many_updates, against Engine.simulate's final values bit for bit -- the entry cannot drift from the
    kernels it stands for."""
    import stock_market_monte_carlo_amd as S
    n, periods, seed, first = 2000, 36, 0x5EED0123456789AB, (1 << 32) - 1000
    stream = 2 if mode_name.endswith("_v2") else 3
    gaussian = mode_name.startswith("gaussian")
    tab = None if gaussian else (W.index_table(2049) * np.float32(0.01) - np.float32(10.0) if mode_name == "table2049" else table)
    mode = S.MODE_GAUSSIAN if gaussian else S.MODE_TABLE
    e = S.Engine(0)
    try:
        if tab is not None:
            e.set_table(tab)
        sim = S.Engine.make_sim(n, periods, mode, seed, first_path=first, stream=stream)
        final = e.simulate(sim).final.cpu().numpy()
        d = 4 if gaussian or tab.size > 2048 else 8
        blocks = (periods + d - 1) // d
        path = first + np.repeat(np.arange(n, dtype=np.uint64), blocks)
        blk = np.tile(np.arange(blocks, dtype=np.uint64), n)
        lo, hi, tag = path & np.uint64(W.M32), path >> np.uint64(32), np.full(path.size, 1 if gaussian else 0, dtype=np.uint64)
        ctr = np.stack([blk, lo, hi, tag] if stream == 3 else [lo, hi, blk, tag], axis=1).astype(np.uint32)
        words = oracle.philox4x32_10_bulk(ctr, [seed & W.M32, seed >> 32])
        a = e.selftest_draws(sim, words)
    finally:
        e.close()
    assert a.shape == (n * blocks, d)
    a = a.reshape(n, blocks * d)[:, :periods]
    assert a.min() > 50.0 and a.max() < 200.0  # a - 100 is exact there, and 100 + (a - 100) is a again
    want = np.array([oracle.many_updates(1000.0, a[i] - np.float32(100.0), periods)[-1] for i in range(n)], dtype=np.float32)
    assert np.array_equal(final.view(np.uint32), want.view(np.uint32))
