"""The word sets of tests/draw_words.py and its independent references, validated with the oracle alone: the sets
reach every bin, sector, entry and digit boundary that can be reached, and oracle.multipliers_of_words -- the very
function the oracle's path loop calls after Philox -- agrees with float64 Box-Muller and with big-integer digits on
all of them.  tests/test_draw_words_gpu.py then asks the same of the device.

Measured here (the oracle, every set and parameter setting): the largest error is 0.71 of the bound for counter
stream v3 (5.6e-5 at std 9) and 0.50 for v2; with std 1e-3 and 0 the draw is within half a unit in the last place."""
import numpy as np
import pytest

import draw_words as W


@pytest.fixture(scope="module")
def gauss_refs():
    return {(stream, name): W.gauss_reference(w, stream) for stream in (3, 2) for name, w in W.gauss_sets(stream).items()}


def test_v3_sets_reach_every_bin_and_sector():
    w = W.gauss_v3_radius()
    side, b = W.v3_bin(w[:, 0])
    hit = set(zip(side.tolist(), b.tolist()))
    reachable = W.reachable_v3_bins()
    # 2 x (1 + 2 + 4 + 28 x 8 + 1): octaves of 1, 2 and 4 integers, 28 full ones, and the single value 2^31
    assert len(reachable) == 464 and hit == reachable
    # every octave's every sub-interval from e = 3 on, both sides; the top octave's first bin from both sides
    for s in (0, 1):
        assert {(s, W.v3_bin_of(e, j)) for e in range(3, 31) for j in range(8)} <= hit
        assert (s, W.v3_bin_of(31, 0)) in hit
    assert (0, 0) in hit and 0 in w[:, 0]  # pattern 0 reads bin 0
    # every first word meets all eight angles
    first, counts = np.unique(w[:, 0], return_counts=True)
    assert first.size == W.v3_radius_first_words().size and np.all(counts == 8)
    # every d of the octaves below 2^3, the corners, and both sides of a rounding point of the last octave
    d = set(W._i32(w[:, 0]).tolist())
    assert set(range(-7, 8)) <= d and {2 ** 31 - 1, -2 ** 31, 2 ** 31 - 65, 2 ** 31 - 64} <= d
    a = W.gauss_v3_angle()
    assert np.array_equal(np.bincount(W.v3_sector(a[:, 1]), minlength=2048), np.full(2048, 3 * 4 * 4))
    assert np.array_equal(np.bincount((a[:, 1] >> 30).astype(np.int64), minlength=4), np.full(4, a.shape[0] // 4))
    # the second pair of every item is another item's first: both halves of the draw see the whole set
    for s in (w, a):
        assert np.array_equal(np.unique(s[:, :2], axis=0), np.unique(s[:, 2:], axis=0))


def test_v2_sets_reach_every_entry():
    w = W.gauss_v2_radius()
    hit = set(W.v2_entry(w[:, 0]).tolist())
    reachable = W.reachable_v2_entries()
    # 2 x (1 + 1 + 2 + 4 + 8 + 27 x 16 + 1): odd integers only below 2^5, 27 full octaves, and the single value 2^32
    assert len(reachable) == 898 and hit == reachable and min(hit) == 0 and max(hit) == 528 + 16 * 32 < 1056
    a = W.gauss_v2_angle()
    e = W.v2_angle_entry(a[:, 1])
    assert np.all(np.bincount(e, minlength=256) >= 4 * 4) and e.max() == 255
    # the rounding add wraps in 32 bits: the words from 0xFF800000 up read entry 0, never an entry 256
    top = a[:, 1] >= 0xFF800000
    assert top.sum() >= 4 and np.all(e[top] == 0)


def test_table_sets_hold_every_digit_boundary():
    for T in W.TABLE_LENGTHS:
        assert W.index_table(T).size == T
        w = W.table_words(T)[:-100000].astype(np.uint64)
        if T <= 2048:
            x = set(((w[:, 0] << np.uint64(32)) | w[:, 1]).tolist()) | set(((w[:, 2] << np.uint64(32)) | w[:, 3]).tolist())
            assert {0, 2 ** 64 - 1} <= x
            for j in range(1, T):
                c = -(-j * 2 ** 64 // T)
                assert c in x and c - 1 in x
        else:
            u = set(w.ravel().tolist())
            assert {0, 0xFFFFFFFF} <= u
            for j in range(1, T):
                c = -(-j * 2 ** 32 // T)
                assert c in u and c - 1 in u


@pytest.mark.parametrize("stream", [3, 2])
def test_oracle_gaussian_draws_against_float64(oracle, gauss_refs, stream):
    worst = 0.0
    for name, w in W.gauss_sets(stream).items():
        for mean, std in W.GAUSS_PARAMS:
            p = oracle.make_params(oracle.MODE_GAUSSIAN, 1, 1, 0, gauss_mean=mean, gauss_std=std, stream=stream)
            got = oracle.multipliers_of_words(p, w)
            err, bound = W.gauss_error(got, w, stream, mean, std, gauss_refs[stream, name])
            ratio = float((err / bound).max())
            print(f"stream v{stream} {name} mean {mean} std {std}: max error {err.max():.3g}, {ratio:.3f} of the bound")
            worst = max(worst, ratio)
            assert np.all(err <= bound), (name, mean, std, int(np.argmax(err / bound)))
    assert worst > 0.25  # the bound is not slack by more than a factor of four on these sets


def test_oracle_bulk_entry_is_the_path_loop(oracle, table):
    """multipliers_of_words of a path's Philox words gives that path's returns (the path loop calls the same function)."""
    seed = 0x0123456789ABCDEF
    key = [seed & 0xFFFFFFFF, seed >> 32]
    for mode, stream, tab in ((oracle.MODE_GAUSSIAN, 3, None), (oracle.MODE_GAUSSIAN, 2, None), (oracle.MODE_TABLE, 3, table),
                              (oracle.MODE_TABLE, 2, table), (oracle.MODE_TABLE, 3, W.index_table(2049))):
        p = oracle.make_params(mode, 40, 1, seed, table=tab, stream=stream)
        path = (5 << 32) + 77
        lo, hi = path & 0xFFFFFFFF, path >> 32
        ctr = np.array([[b, lo, hi, mode] if stream == 3 else [lo, hi, b, mode] for b in range(10)], dtype=np.uint32)
        words = oracle.philox4x32_10_bulk(ctr, key)
        assert np.array_equal(words[3], oracle.philox4x32_10(ctr[3], key))
        a = oracle.multipliers_of_words(p, words).ravel()[:40]
        r = oracle.counter_path_returns(p, path)
        assert np.array_equal((np.float32(100.0) + r).view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("T", W.TABLE_LENGTHS)
def test_oracle_table_draws_against_big_integers(oracle, T):
    w = W.table_words(T)
    want = W.table_reference(w, T)
    assert want.shape == (w.shape[0], 8 if T <= 2048 else 4) and want.min() == 0 and want.max() == T - 1
    for stream in (3, 2):
        p = oracle.make_params(oracle.MODE_TABLE, 1, 1, 0, table=W.index_table(T), stream=stream)
        a, idx = oracle.multipliers_of_words(p, w, want_indices=True)
        assert np.array_equal(idx.astype(np.int64), want)
        assert np.array_equal(a.astype(np.float64) - 100.0, want.astype(np.float64))
        assert idx.max() < T


def test_oracle_invariants_on_given_words(oracle):
    p = oracle.make_params(oracle.MODE_GAUSSIAN, 1, 1, 0)
    a = W.gauss_v3_angle()
    got = oracle.multipliers_of_words(p, a).view(np.uint32)
    q = a.shape[0] // 4 // 4  # per first word: four settings of the top bits, one after the other
    blocks = got[:, :2].reshape(4, 4, -1, 2)
    assert blocks.shape[2] == 3 * 2048 == q and all(np.array_equal(blocks[:, 0], blocks[:, t]) for t in range(1, 4))
    w = np.array([[0x7FFFFFFF, 5, 0x7FFFFFC0, 5], [0x80000000, 5, 0x7FFFFFFF, 5]], dtype=np.uint32)
    p0 = oracle.make_params(oracle.MODE_GAUSSIAN, 1, 1, 0, gauss_mean=0.0, gauss_std=1.0)
    m = oracle.multipliers_of_words(p0, w).view(np.uint32).reshape(4, 2)
    # one radius (u = 1/2 from either side, test_numerics_cpu.py) and one angle: with std 1 the staged coefficients are the
    # table's own, so the multipliers are the same bits
    assert np.all(m == m[0])
    assert oracle.multipliers_of_words(p, np.zeros((0, 4), dtype=np.uint32)).shape == (0, 4)
