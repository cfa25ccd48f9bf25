"""Chosen "Philox" words for the draw self-test (smmc_engine_selftest_draws, oracle.multipliers_of_words), the bin
each word lands in, and references that share nothing with the oracle or the kernels.

TEST INFRASTRUCTURE, like blocks_reference.py.  tests/test_draw_words_cpu.py validates the sets and the references
with the oracle alone; tests/test_draw_words_gpu.py feeds the same sets to the device.

An item is four 32-bit words (u0, u1, u2, u3) in the place of one Philox block's output.  A Gaussian draw makes two
pairs of normals of it, from (u0, u1) and (u2, u3): first word radius, second word angle.  A dense table draw
(T <= 2048) makes four base-T digits of each 64-bit half (u0:u1), (u2:u3); a sparse one an index of every word.

Where a word lands, as smmc_kernels.hip documents it (written again here in numpy, not taken from the oracle):

  v3 radius  d = the word read as int32, f = fl(d) in binary32.  The bin is bits [20, 28) of f's pattern (the
             exponent's low five bits and three mantissa bits), the side its sign.  With |f| in [2^e, 2^(e+1)) the
             octave field is (e - 1) mod 32; d = 0 has pattern 0 and reads bin 0 of side 0.
  v3 angle   sector = bits [19, 30) of the second word; the top two bits are not used.
  v2 radius  w = word ^ (word >>a 31), f = fl(2 w + 1): entry = 528 side + 16 (exponent - 127) + top four mantissa
             bits; 33 octaves of 16.
  v2 angle   entry = (word + 0x00800000) >> 24 in 32-bit arithmetic: the words from 0xFF800000 up wrap to entry 0.

Not every bin has a word: an octave of integers below 2^3 (v3) or 2^5 (v2, odd integers only) is shorter than its
row of bins, and the top octave holds the one value 2^31 (v3) or 2^32 (v2).  reachable_v3_bins() and
reachable_v2_entries() enumerate the small octaves exhaustively and state the rest: 464 of v3's 512 bins and 898
of v2's 1056 entries can be read at all.
"""
import functools

import numpy as np

M32 = 0xFFFFFFFF

# (gauss_mean, gauss_std): bench.py's headline configuration, the unit normal, a wide and a narrow one, no spread.
# 100 + mean is exact in binary32 for every one of them, so the draw's only roundings are those of its own steps.
GAUSS_PARAMS = [(0.5, 0.83333), (0.0, 1.0), (-3.0, 9.0), (0.5, 1e-3), (0.5, 0.0)]
TABLE_LENGTHS = [1, 2, 3, 1127, 2047, 2048, 2049, 12289]  # 2048: last dense (eight draws a block), 2049: first sparse

# second words of the radius sets: eight angles spread over the circle, the unused top bits varied
_RADIUS_ANGLES = [(k << 27) + 0x02D5A7 + ((k * 3 & 3) << 30) & M32 for k in range(8)]
# first words of the angle sets: the deepest tail, next to U = 1/2, and one ordinary word per side
_V3_ANGLE_RADII = [0x00000003, 0x7FFFFF00, 0x12345678, 0xC0FFEE11]
_V2_ANGLE_RADII = [0x00000001, 0x7FFFFF00, 0x12345678, 0xC0FFEE11]


def _items(first, second):
    """One item per (first word, second word): (u0, u1) = (first, second); (u2, u3) the pair of the item half a set on."""
    a = np.asarray(first, dtype=np.uint64).astype(np.uint32).ravel()
    b = np.asarray(second, dtype=np.uint64).astype(np.uint32).ravel()
    assert a.size == b.size
    h = a.size // 2
    return np.stack([a, b, np.roll(a, h), np.roll(b, h)], axis=1)


def _cross(first, second):
    f = np.asarray(first, dtype=np.uint64)
    s = np.asarray(second, dtype=np.uint64)
    return _items(np.repeat(f, s.size), np.tile(s, f.size))


# ---- where a word lands ---------------------------------------------------------------------------------------------

def _i32(words):
    d = np.asarray(words, dtype=np.uint64).astype(np.int64)
    return np.where(d >= 2 ** 31, d - 2 ** 32, d)


def v3_bin(words):
    """(side, bin) of counter stream v3's radius table for each first word: bin in 0 .. 255."""
    bits = _i32(words).astype(np.float32).view(np.uint32)
    return (bits >> np.uint32(31)).astype(np.int64), ((bits >> np.uint32(20)) & np.uint32(0xFF)).astype(np.int64)


def v3_bin_of(e, j):
    """The bin of sub-interval j of the octave |f| in [2^e, 2^(e+1))."""
    return ((e - 1) % 32) * 8 + j


def v3_sector(words):
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(19)) & np.uint64(2047)).astype(np.int64)


def _v2_w1(words):
    u = np.asarray(words, dtype=np.uint64)
    side = u >> np.uint64(31)
    w = np.where(side == 1, u ^ np.uint64(M32), u)
    return side.astype(np.int64), 2 * w + 1  # odd, below 2^32


def v2_entry(words):
    """Entry 0 .. 1055 of counter stream v2's radius table for each first word."""
    side, w1 = _v2_w1(words)
    bits = w1.astype(np.float32).view(np.uint32).astype(np.int64)
    return 528 * side + (bits >> 19) - 127 * 16


def v2_angle_entry(words):
    return (((np.asarray(words, dtype=np.uint64) + np.uint64(0x00800000)) & np.uint64(M32)) >> np.uint64(24)).astype(np.int64)


def reachable_v3_bins():
    """{(side, bin)} that some int32 reaches.  Octaves e < 8 by enumeration of every d; 8 <= e <= 30 hold 2^e >= 256
    integers, at least 32 in each of the eight bins; e = 31 is |f| = 2^31 alone (d = INT32_MIN, and the positive d that
    round up to it), its bin the first of its row."""
    d = np.arange(-255, 256, dtype=np.int64)
    side, b = v3_bin(d & M32)
    out = set(zip(side.tolist(), b.tolist()))
    for s in (0, 1):
        out |= {(s, v3_bin_of(e, j)) for e in range(8, 31) for j in range(8)}
        out.add((s, v3_bin_of(31, 0)))
    return out


def reachable_v2_entries():
    """Entries that some word reaches.  2 w + 1 below 2^10 by enumeration; octaves 10 .. 31 hold at least 32 odd
    integers per entry; octave 32 is fl(2 w + 1) = 2^32 alone, the first entry of its row."""
    w = np.arange(0, 512, dtype=np.uint64)
    out = set(v2_entry(w).tolist()) | set(v2_entry(w ^ np.uint64(M32)).tolist())
    for s in (0, 1):
        out |= {528 * s + 16 * e + j for e in range(10, 32) for j in range(16)}
        out.add(528 * s + 16 * 32)
    return out


# ---- the word sets ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def v3_radius_first_words():
    """Both signs, octaves e = 0 .. 30, every sub-interval: first, middle and last |d| of the bin; every d for e < 3;
    from e = 24 on (fl(d) rounds) the |d| on both sides of the point below each bin's upper edge where fl(d) starts to
    round up into the next bin or octave; 0, +-1, INT32_MAX, INT32_MIN and the two words the oracle's tests name."""
    mags = {1, 2, 3, 4, 5, 6, 7, 2 ** 31 - 1, 0x7FFFFFC0, 2 ** 31 - 65, 2 ** 31 - 64}
    for e in range(3, 31):
        for j in range(8):
            lo, hi = (8 + j) << (e - 3), (9 + j) << (e - 3)
            mags |= {lo, (lo + hi) // 2, hi - 1}
            if e >= 24:
                half = 1 << (e - 24)  # half a unit in the last place of the octave
                mags |= {hi - half - 1, hi - half, hi - half + 1, lo + half, lo + half + 1}
    mags = sorted(m for m in mags if 0 < m < 2 ** 31)
    d = [0] + mags + [-m for m in mags] + [-2 ** 31]
    return np.array([x & M32 for x in d], dtype=np.uint64)


def gauss_v3_radius():
    return _cross(v3_radius_first_words(), _RADIUS_ANGLES)


def gauss_v3_angle():
    """Every sector, its first, middle and last residual, each setting of the two unused top bits, four radii."""
    low = np.array([(i << 19) + r for i in range(2048) for r in (0, 1 << 18, (1 << 19) - 1)], dtype=np.uint64)
    ub = (low[None, :] | (np.arange(4, dtype=np.uint64)[:, None] << np.uint64(30))).ravel()
    return _cross(_V3_ANGLE_RADII, ub)


@functools.lru_cache(maxsize=None)
def v2_radius_first_words():
    """As v3_radius_first_words for v2's 2 x 33 x 16 entries, where the float is fl(2 w + 1)."""
    ws = set(range(0, 64)) | {2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 64, 2 ** 31 - 65}
    for e in range(5, 32):
        for j in range(16):
            lo, hi = (16 + j) << (e - 4), (17 + j) << (e - 4)  # 2 w + 1 in [lo, hi)
            ws |= {lo // 2, (lo + hi) // 4, (hi - 2) // 2}
            if e >= 24:
                x = (hi - (1 << (e - 24))) // 2  # 2 w + 1 next to where fl() starts to round up to hi
                ws |= {x - 2, x - 1, x, x + 1, lo // 2 + (1 << (e - 24)) // 2 + 1}
    ws = sorted(w for w in ws if 0 <= w < 2 ** 31)
    return np.array(ws + [w ^ M32 for w in ws], dtype=np.uint64)


def gauss_v2_radius():
    return _cross(v2_radius_first_words(), _RADIUS_ANGLES)


def gauss_v2_angle():
    """Every entry: the first and last word that round to it, its own angle and the last before the rounding add
    carries -- among them 0xFF800000 .. 0xFFFFFFFF, where the add wraps to entry 0."""
    ub = np.array([((i << 24) + o) & M32 for i in range(256) for o in (-0x00800001, -0x00800000, 0, 0x007FFFFF)]
                  + [0xFF800000, 0xFF800001, 0xFFFFFFFF, 0xFF7FFFFF], dtype=np.uint64)
    return _cross(_V2_ANGLE_RADII, ub)


@functools.lru_cache(maxsize=None)
def _random_cached():
    rng = np.random.default_rng(20261018)
    w = rng.integers(0, 2 ** 32, size=(100000, 4), dtype=np.uint64).astype(np.uint32)
    w.setflags(write=False)
    return w


def random_words():
    return _random_cached()


def gauss_sets(stream):
    """{name: (n, 4) uint32} for a Gaussian stream (3 or 2)."""
    if stream == 2:
        return {"radius": gauss_v2_radius(), "angle": gauss_v2_angle(), "random": random_words()}
    return {"radius": gauss_v3_radius(), "angle": gauss_v3_angle(), "random": random_words()}


def _spread(top, count=512):
    """0 .. top: all of them when few, else the ends and `count` values between."""
    if top <= 4 * count:
        return list(range(top + 1))
    return sorted(set(range(4)) | {top - k for k in range(4)} | {top * k // count for k in range(count + 1)})


def dense_fractions(T):
    """64-bit fractions x at the boundaries of each of the four base-T digits: ceil(m 2^64 / T^(k+1)) and the value
    before it, for m spread over 0 .. T^(k+1) (every m for the first digit); 0 and all ones."""
    xs = {0, 2 ** 64 - 1}
    for k in range(4):
        den = T ** (k + 1)
        for m in (range(T + 1) if k == 0 else _spread(den)):
            c = -(-m * 2 ** 64 // den)
            xs |= {c % 2 ** 64, (c - 1) % 2 ** 64}
    return sorted(xs)


def table_words(T):
    """(n, 4) uint32 for a table of T entries: dense_fractions in both 64-bit halves, or for a sparse table every
    boundary ceil(j 2^32 / T) and the word before it in every position; plus the random quadruples."""
    if T <= 2048:
        x = np.array(dense_fractions(T), dtype=np.uint64)
        y = np.roll(x, x.size // 2 + 1)
        w = np.stack([x >> np.uint64(32), x & np.uint64(M32), y >> np.uint64(32), y & np.uint64(M32)], axis=1)
    else:
        us = {0, M32}
        for j in range(T + 1):
            c = -(-j * 2 ** 32 // T)
            us |= {c % 2 ** 32, (c - 1) % 2 ** 32}
        u = np.array(sorted(us), dtype=np.uint64)
        u = np.concatenate([u, u[: (-u.size) % 4]])
        q = u.size // 4
        w = np.stack([u[:q], u[q:2 * q][::-1], u[2 * q:3 * q], u[3 * q:][::-1]], axis=1)
    return np.concatenate([w.astype(np.uint32), random_words()])


def index_table(T):
    """Returns in percent with r[i] = i: the multiplier 100 + i is exact in binary32, so a - 100 is the index drawn."""
    t = np.arange(T, dtype=np.float32)
    assert np.array_equal((np.float32(100.0) + t).astype(np.float64), 100.0 + np.arange(T, dtype=np.float64))
    return t


# ---- references -------------------------------------------------------------------------------------------------------

def table_reference(words, T):
    """The indices of every item by exact Python integers: (n, 8) dense, (n, 4) sparse."""
    out = []
    for u0, u1, u2, u3 in np.asarray(words, dtype=np.uint64).tolist():
        if T <= 2048:
            row = []
            for x in ((u0 << 32) | u1, (u2 << 32) | u3):
                for _ in range(3):
                    prod = x * T
                    row.append(prod >> 64)
                    x = prod & (2 ** 64 - 1)
                row.append(((x >> 32) * T) >> 32)
        else:
            row = [(u * T) >> 32 for u in (u0, u1, u2, u3)]
        out.append(row)
    return np.array(out, dtype=np.int64)


def gauss_reference(words, stream):
    """(z, r): the four unit normals of every item in float64, (n, 4), and the radius behind each, from the streams'
    definitions: v3 u = |fl(d)| / 2^32 (2^-33 for d = 0), theta = 2 pi (ub mod 2^30) / 2^30; v2 u = fl(2 w + 1) / 2^33,
    theta = 2 pi ub / 2^32; the side decides between ln u and log1p(-u)."""
    w = np.asarray(words, dtype=np.uint64)
    z = np.empty(w.shape, dtype=np.float64)
    rr = np.empty(w.shape, dtype=np.float64)
    for k in (0, 2):
        ua, ub = w[:, k], w[:, k + 1]
        if stream == 2:
            side, w1 = _v2_w1(ua)
            u = w1.astype(np.float32).astype(np.float64) / 2.0 ** 33
            neg = side == 1
            th = 2 * np.pi * ub.astype(np.float64) / 2.0 ** 32
        else:
            d = _i32(ua)
            f = d.astype(np.float32).astype(np.float64)
            u = np.where(d == 0, 2.0 ** -33, np.abs(f) / 2.0 ** 32)
            neg = d < 0
            th = 2 * np.pi * (ub % np.uint64(2 ** 30)).astype(np.float64) / 2.0 ** 30
        r = np.where(neg, np.sqrt(-2 * np.log1p(-u)), np.sqrt(-2 * np.log(u)))
        z[:, k], z[:, k + 1] = r * np.cos(th), r * np.sin(th)
        rr[:, k] = rr[:, k + 1] = r
    return z, rr


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def gauss_error(got, words, stream, mean, std, ref=None):
    """(error, bound) per draw of multipliers `got` against 100 + mean + std z.

    v3: std times what tests/test_numerics_cpu.py asserts for the oracle's unit draw, 1.0e-6 (1 + r), plus one unit in
    the last place of the multiplier for the final fma.  v2: std times that file's 2e-6 for its unit draw, plus one unit
    in the last place each for its two last roundings, the return fma(r std, cos, mean) and 100 + return."""
    z, r = ref if ref is not None else gauss_reference(words, stream)
    m, s = float(np.float32(mean)), float(np.float32(std))
    want = 100.0 + m + s * z
    if stream == 2:
        bound = abs(s) * 2e-6 + ulp32(m + s * z) + ulp32(want)
    else:
        bound = abs(s) * 1.0e-6 * (1 + r) + ulp32(want)
    return np.abs(np.asarray(got, dtype=np.float64) - want), bound
