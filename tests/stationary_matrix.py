"""The ledger of stationary_kernel's instantiations (csrc/smmc_kernels.hip), the cases that harden the stationary bootstrap
the way tests/feature_matrix.py hardens the older families, and their restatement.

stationary_kernel<kDiv, kDense> is compiled for three divides x two table layouts; launch_stationary picks one from the
host's divide kind and table_is_dense(table_len).  ROWS lists the six by their template arguments, each with ONE request
that makes the host choose it through stock_market_monte_carlo_amd.stationary: tests/test_stationary_matrix_cpu.py asserts
that ROWS names exactly what is compiled, tests/test_stationary_matrix_gpu.py asks the host for the kind, then runs the row
at q = 1/12 and 1/2 and P = 9, 13 and 16 -- a remainder of one period and of five, the two sides of the second candidate
block that the four-draw layout skips when at most four periods are left, and no remainder.  Path ids start at 2^32 - 100:
the low word wraps inside the first chunk.

How a row is reached.  EXACT: the flag on a tame table.  CHECKED: no flag, capital 2^100 on feature_matrix's "window"
series (every eighth month +300 %), the pattern of the blocks rows: smmc_engine_stationary_divide_kind is
host_divide_kind(e, sim, true), the very rule smmc_engine_blocks_divide_kind asks, and host_divide() below restates it --
9 periods of +300 % from 2^100 are not provable (100 + 18 + log2 400 + 1 > 127), the window's upper end is
2^(126 - 14 - log2 400) = 2^103.4 > 2^102.  FAST: that table's tame twin from 1000.

Beyond the ledger:
- WILD: inputs for which the two divides give DIFFERENT bits (feature_matrix's wild months from a capital near
  2^-114 / 100), on both layouts; the host cannot prove them and must say EXACT without the flag.
- WINDOW: CHECKED launches of 360, 363 and 367 periods on +100 % / -50 % tables, part of whose paths leave the window at
  one of the kernel's tests (after periods 8, 16, ..: redone with the IEEE divide) and some of whose paths are inside it
  at every test and outside it only after the last 3 or 7 periods, where no test follows and the host's margin of seven
  periods alone keeps the fast divide in its domain.  "redo" and "redo-2049" (blocks_reference.redo_table, and its
  pattern repeated) drift upwards and leave at the top, where both divides agree on every product -- an overflow is inf
  either way -- so they check the redo's walk, not its divide.  "mirror" and "mirror-2049" (five -49 %, three +97 %)
  drift downwards: their leavers go on below 2^-114, where the fast divide is wrong, so a redo that is skipped, or that
  runs the fast divide, changes bits.
- EDGES: the largest LDS layout (16384 entries, 4096 buckets); runs that wrap from the table's last entry to its first;
  path ids that wrap at 2^64.
"""
import functools
import math

import numpy as np

import blocks_reference as bref
import stationary_reference as ref
from feature_matrix import EXTREME_CAPITAL, TINY, _series, compound, fast_div100

f32 = np.float32
SEED = ref.SEED
N = 2 * 256 + 37                   # two whole chunks and a ragged one
N_SHARE = 2048                     # where a share of the paths is asserted
CROSSING = (1 << 32) - 100         # the id's low word wraps inside the first chunk
WRAPPING = (1 << 64) - 300         # the id itself wraps inside the launch
DENSE, FOUR = 2048, 2049           # the two sides of table_is_dense
MAX_TABLE, MAX_BINS = 16384, 4096  # SMMC_MAX_TABLE, SMMC_MAX_BINS (include/smmc.h)
DIV_FAST, DIV_EXACT, DIV_CHECKED = 0, 1, 2
SIGNATURE = "ib"                   # stationary_kernel's template parameters as the Itanium ABI spells their types
ROW_QS = (5461, 32768)
ROW_PS = (9, 13, 16)


def mangled(args):
    """The template-argument list of an instantiation as it appears in the kernel's symbol: I Li2E Lb0E E."""
    return "I" + "".join(f"L{t}{int(v)}E" for t, v in zip(SIGNATURE, args)) + "E"


# ---- inputs ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def table_of(key):
    """'tame-T', 'window-T', 'wild-T' (feature_matrix._series); 'redo' and 'mirror' (8 entries: five +100 % and three -50 %,
    five -49 % and three +97 %) and 'redo-2049', 'mirror-2049' (the pattern repeated); anything else is
    blocks_reference.table_of's.  Computed once, shared, read-only."""
    kind, _, length = key.partition("-")
    if kind in ("tame", "window", "wild"):
        return _series(int(length), kind)
    if kind in ("redo", "mirror"):
        t = bref.redo_table() if kind == "redo" else np.array([-49.0] * 5 + [97.0] * 3, dtype=f32)
        t = np.resize(t, int(length)) if length else t
        t.setflags(write=False)
        return t
    return bref.table_of(key)


def hist_range(capital, n_bins=bref.BINS):
    """(n_bins, lo, hi, below) of a case's record: blocks_reference's for its capital, scaled with the capital otherwise."""
    if capital == bref.CAPITAL:
        return n_bins, bref.LO, bref.HI, bref.BELOW
    return n_bins, 0.0, float(f32(4.0 * capital)), float(f32(0.9 * capital))


def _case(name, table, P, q, n=N, first=CROSSING, capital=bref.CAPITAL, flag=False, kind=None, n_bins=bref.BINS, **kw):
    c = dict(table=table, P=P, q=q, n=n, first=first, capital=capital, flag=flag, kind=kind, seed=SEED)
    c["hist"] = hist_range(capital, n_bins)
    c.update(kw)
    c["id"] = f"{name}-{table}-P{P}-q{q}" + ("-flag" if flag else "")
    return c


def with_flag(c):
    """The same request with SMMC_FLAG_EXACT_DIV: the same restatement (results never depend on the divide)."""
    return dict(c, flag=True, kind=DIV_EXACT, id=c["id"] + "-flag")


def _rows():
    """(template arguments, the row's request); the GPU test runs the request at every (q, P) of ROW_QS x ROW_PS."""
    out = []
    for T in (DENSE, FOUR):
        dense = T <= DENSE
        out.append(dict(args=(DIV_FAST, dense), case=_case("row", f"tame-{T}", 9, 5461, kind=DIV_FAST)))
        out.append(dict(args=(DIV_EXACT, dense), case=_case("row", f"tame-{T}", 9, 5461, flag=True, kind=DIV_EXACT)))
        out.append(dict(args=(DIV_CHECKED, dense), case=_case("row", f"window-{T}", 9, 5461, capital=2.0 ** 100, kind=DIV_CHECKED)))
    for r in out:
        r["id"] = "stationary" + mangled(r["args"])
    return out


def row_cases(row):
    """The row's request at every run length and renewal probability the ledger runs it at."""
    c = row["case"]
    return [_case("row", c["table"], P, q, capital=c["capital"], flag=c["flag"], kind=c["kind"]) for q in ROW_QS for P in ROW_PS]


# Inputs that tell the divides apart: the wild months from 7e-37.  An ending at NaN takes two 3e38 % months (the second
# product overflows) and then the -100 % month (inf * 0): about 4e-5 of the paths within nine periods.  At q = 16384 and
# 549 paths the restatement has 95 .. 168 paths with a differing quotient and 72 .. 118 at 0, but 0 .. 2 at inf and none
# at NaN, on either table.  So q was moved: on 7 * 256 + 37 paths the dense table has all three endings at every
# multiple of 1024 from 23552 to 44032, and q = 32768 (a coin) has them on both tables.  Measured there, of 1829 paths
# (tests/test_stationary_matrix_cpu.py prints them): with a differing quotient / never / ending at 0 / at inf / at NaN --
#   wild-2048  P = 9: 310 (16.9 %) / 1519 / 260 / 2 / 1      P = 13: 452 (24.7 %) / 1377 / 373 / 5 / 1
#   wild-2049  P = 9: 326 (17.8 %) / 1503 / 240 / 8 / 1      P = 13: 470 (25.7 %) / 1359 / 345 / 10 / 1
N_WILD = 7 * 256 + 37
WILD = [_case("wild", f"wild-{T}", P, 32768, n=N_WILD, capital=EXTREME_CAPITAL["table"], kind=DIV_EXACT) for T in (DENSE, FOUR)
        for P in (9, 13)]

# The checked window: 2048 paths, q = 16384.  The upward tables start from 1000 (window [2^-81, 2^111.4]: grow = shrink =
# 1 bit per period); the downward ones (-49 % and +97 %: multipliers that are no powers of two -- with 50 and 200 every
# quotient is a power of two and the fast divide is right even among the subnormals) from 2^-20, which puts the end of
# their median path (-0.24 bits per period) near 2^-106: most paths pass the window's lower end, 2^-81.2, and part of
# them go on below 2^-114.  Measured on the restatement, P = 360 / 363 / 367 (the CPU test prints them): the share of
# paths outside the window at one of the kernel's tests; the paths inside it at every test and outside it after the last
# period; the paths that left at a test and form a product on which the two divides differ --
#   redo          0.255             0 / 20 / 61         0
#   redo-2049     0.250             0 / 30 / 59         0
#   mirror        0.953             0 / 13 / 24         263 / 303 / 347
#   mirror-2049   0.952             0 / 17 / 26         275 / 309 / 353
# No path that stays inside the window at every test forms a product on which the divides differ: the host's margin.
MIRROR_CAPITAL = 2.0 ** -20
WINDOW = [_case("window", t, P, 16384, n=N_SHARE, kind=DIV_CHECKED, capital=MIRROR_CAPITAL if t.startswith("mirror") else bref.CAPITAL)
          for t in ("redo", "redo-2049", "mirror", "mirror-2049") for P in (360, 363, 367)]

LARGEST = [_case("largest", str(MAX_TABLE), 13, q, n_bins=MAX_BINS) for q in (0, 1, 5461, 65535, 65536)]
# one run per path (q = 0): 40 of 2049 and 366 of 16384 starts run past the table's end
INDEX_WRAP = [_case("index-wrap", "2049", 41, 0), _case("index-wrap", str(MAX_TABLE), 367, 0)]
ID_WRAP = [_case("id-wrap", t, 13, 5461, first=WRAPPING) for t in ("bundled", "2049")]
EDGES = LARGEST + INDEX_WRAP + ID_WRAP

ROWS = _rows()
CASES = [c for r in ROWS for c in row_cases(r)] + WILD + WINDOW + EDGES


# ---- the host's rule, restated ---------------------------------------------------------------------------------------

def host_divide(c):
    """divide_kind of csrc/smmc_capi.cpp for a case, restated in binary64: (kind, window lo, window hi), the window as
    the binary32 values the kernel compares with (0, 0 unless CHECKED)."""
    none = (DIV_EXACT, f32(0.0), f32(0.0))
    if c["flag"]:
        return none
    with np.errstate(all="ignore"):
        a = f32(100.0) + table_of(c["table"])
    cap = float(f32(c["capital"]))
    if not (cap > 0.0 and math.isfinite(cap)) or not np.isfinite(a).all():
        return none
    lo_a, hi_a = float(a.min()), float(a.max())
    if not lo_a > 0.0:
        return none
    grow, shrink = max(0.0, math.log2(hi_a / 100.0)), max(0.0, -math.log2(lo_a / 100.0))
    top, bottom, lc, P = math.log2(hi_a), min(0.0, math.log2(lo_a)), math.log2(cap), float(c["P"])
    if lc + P * grow + top + 1.0 < 127.0 and lc - P * shrink + bottom - 1.0 > -89.0:
        return (DIV_FAST, f32(0.0), f32(0.0))
    hi_w, lo_w = 127.0 - 1.0 - 7.0 * grow - top, -89.0 + 1.0 + 7.0 * shrink - bottom
    if not (lo_w + 2.0 < lc < hi_w - 2.0):
        return none
    return (DIV_CHECKED, f32(2.0 ** lo_w), f32(2.0 ** hi_w))


# ---- the restatement -------------------------------------------------------------------------------------------------

def indices(oracle, c):
    """[n, P] table index of every period of every path of a case."""
    return ref.indices_bulk(oracle, table_of(c["table"]), c["seed"], c["first"], c["n"], c["P"], c["q"])


def first_candidates(oracle, c):
    """[n] the candidate start of period 0: where a path's first run begins."""
    return ref.candidates(oracle, table_of(c["table"]), c["seed"], c["first"], c["n"], 1)[:, 0]


def walk(oracle, c):
    """(values [n, P + 1], products [n, P]) of a case: feature_matrix.compound over the multipliers the walk reads."""
    with np.errstate(all="ignore"):
        a = (f32(100.0) + table_of(c["table"]))[indices(oracle, c)]
    return compound(a, c["capital"])


def fast_divide_differs(oracle, c):
    """bool [n]: div100<false> of some product of the path is not the IEEE quotient's bits (feature_matrix's, on this walk)."""
    x = walk(oracle, c)[1]
    with np.errstate(all="ignore"):
        q = x / f32(100.0)
    fq = fast_div100(x)
    return ((q.view(np.uint32) != fq.view(np.uint32)) & ~(np.isnan(q) & np.isnan(fq))).any(axis=1)


def below_the_fast_domain(oracle, c):
    """bool [n]: the path forms a non-zero product below 2^-114, or one that is not finite (feature_matrix.left_window)."""
    x = walk(oracle, c)[1]
    with np.errstate(all="ignore"):
        return (((np.abs(x) < f32(TINY)) & (x != 0)) | ~np.isfinite(x)).any(axis=1)


def window_leavers(oracle, c):
    """(left at a test [n], left only after the last period [n]): stationary_reference.values_at_window_tests -- the values
    after periods 8, 16, .., where stationary_kernel tests SMMC_DIV_CHECKED's window -- extended by the value after the
    last period, which the kernel does not test when P is no multiple of 8."""
    kind, lo, hi = host_divide(c)
    assert kind == DIV_CHECKED, c["id"]
    at = ref.values_at_window_tests(oracle, table_of(c["table"]), c["seed"], c["first"], c["n"], c["P"], c["q"], c["capital"])
    last = reference(oracle, c)["final"]
    assert at.shape == (c["n"], c["P"] // 8)
    if c["P"] % 8 == 0:
        assert np.array_equal(at[:, -1].view(np.uint32), last.view(np.uint32))
    with np.errstate(all="ignore"):
        at_test = (~((at > lo) & (at < hi))).any(axis=1)
        after = ~((last > lo) & (last < hi))
    return at_test, ~at_test & after


@functools.lru_cache(maxsize=None)
def _reference(oracle, table, n, P, q, seed, first, capital, hist):
    out = ref.result(oracle, table_of(table), n, P, q, seed=seed, first_path=first, capital=capital, n_bins=hist[0], lo=hist[1],
                     hi=hist[2], below=hist[3])
    for k in ("final", "hist", "chunk_mean", "chunk_var"):
        out[k].setflags(write=False)
    return out


def reference(oracle, c, n_bins=None):
    """stationary_reference.result of a case (dict(final, stats, hist, chunk_mean, chunk_var)): computed once per request,
    shared, never modified.  n_bins: another bucket count on the case's range."""
    hist = c["hist"] if n_bins is None else (n_bins,) + tuple(c["hist"][1:])
    return _reference(oracle, c["table"], c["n"], c["P"], c["q"], c["seed"], c["first"], c["capital"], tuple(hist))
