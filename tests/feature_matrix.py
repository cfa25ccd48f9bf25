"""The ledger of the feature kernels' instantiations, and the restatement of every case it runs.

The seven families on the wave-walk skeleton or the block walk (csrc/smmc_kernels.hip: launch_wave_walk, the *Family::get
switches, launch_blocks) are compiled for every combination of their template arguments.  ROWS lists each instantiation
by those arguments together with ONE case -- mode, table length, divide request, K, constant or per-period schedule, S,
block length, SMMC_BLOCKS_READ -- that makes the host choose it through the public entry point.
tests/test_feature_matrix_cpu.py asserts that ROWS names exactly the instantiations the kernels compile to (none missing,
none extra: a new template parameter fails there until its rows are written); tests/test_feature_matrix_gpu.py runs every
row, and the EXTREME cases below, against reference() here.

Shapes: 64 kW 2 + 37 paths with kW = 4 (table) or 8 (Gaussian) waves per workgroup -- whole chunks, a ragged one and
inactive lanes; 9 periods for dense tables (a Philox block yields eight draws), 5 for four-draw tables and Gaussian mode
(four draws): one whole block and a partial one.  Table lengths 2048 and 2049 are the two sides of table_is_dense.
Sweeps of S = 2, 3 and 5 take the widths 2, 4 and 8, the last two padded.  A blocks launch is CHECKED only where the host's
window rule (divide_kind, smmc_capi.cpp) holds, and that rule reasons about a whole eight-period block: 126 - P g - top <=
log2(capital) < 124 - 7 g - top has no solution below P = 8, so the CHECKED rows of both table forms run 9 periods, from a
capital of 2^100 on a table whose best month is +300 % (g = 2, top = log2 400).

The IEEE-divide rows are reached by the flag on a tame table (the rest of the kernel is checked, the divide is not: inside
the proven domain both divides give the same bits).  EXTREME adds, per family and mode, inputs for which the two divides
DIFFER.  div100 (csrc/smmc_device.h) equals the IEEE quotient for every product of magnitude >= 2^-114 and for 0, inf and
NaN; it differs only below 2^-114.  So the extreme inputs start from a capital near 2^-114 / 100: part of the paths pass
below the window, part never do; the wild table's -99 % months take paths on to subnormals and to 0, its -100 % month to 0
and its 3e38 % month back up and to inf (0 * inf: NaN).  left_window() and fast_divide_differs() state that on the
restatement alone, for tests/test_feature_matrix_cpu.py.

The twelve per-period FAST rows of portfolio_cashflow_kernel check the contribution arm only: the host proves the fast
divide for a per-period schedule only when every amount is <= 0 and every fraction 0 (divide_rule,
csrc/smmc_portfolio_cashflow.cpp: its second shape asks for a constant amount), so no path of theirs is depleted; the
per-period depletion arm runs in the twelve exact-divide rows and in tests/test_feature_fuzz_gpu.py."""
import functools
import math

import numpy as np

import blocks_reference as bref
import cashflow_reference as cref
import excursions_reference as xref
import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

f32 = np.float32
SEED = 0x5EED0123456789AB
FIRST_PATH = (1 << 32) - 100       # the id crosses 2^32 inside every launch
CAPITAL = 1000.0
BINS, LO, HI, BELOW = 64, 0.0, 4000.0, 1000.0
GAUSS_MEAN, GAUSS_STD = 0.6, 4.3
FLOOR = 0.01
TINY = 2.0 ** -114                 # below it div100<false> is not the IEEE quotient
DENSE, FOUR = 2048, 2049           # the two sides of table_is_dense
FAMILIES = ("checkpoints_kernel", "cashflow_kernel", "cashflow_sweep_kernel", "excursions_kernel", "blocks_kernel",
            "portfolio_kernel", "portfolio_cashflow_kernel")
# the template parameters of each family, in order, as the Itanium ABI spells their types (i: int, b: bool)
SIGNATURES = {"checkpoints_kernel": "ibb", "cashflow_kernel": "ibbb", "cashflow_sweep_kernel": "ibbi", "excursions_kernel": "ibb",
              "blocks_kernel": "ibb", "portfolio_kernel": "ibbi", "portfolio_cashflow_kernel": "ibbib"}
MODE_TABLE, MODE_GAUSSIAN = 0, 1
DIV_FAST, DIV_EXACT, DIV_CHECKED = 0, 1, 2
SWEEP_S = {2: 2, 4: 3, 8: 5}       # width -> the S of its row


def mangled(family, args):
    """The template-argument list of an instantiation as it appears in the kernel's symbol: I Li1E Lb0E ... E."""
    return "I" + "".join(f"L{t}{int(v)}E" for t, v in zip(SIGNATURES[family], args)) + "E"


def _modes():
    """(kMode, kDense, mode name, table length) of the ladder's three rungs."""
    return [(MODE_GAUSSIAN, False, "gauss", 0), (MODE_TABLE, True, "table", DENSE), (MODE_TABLE, False, "table", FOUR)]


def _case(family, args, mode, T, **kw):
    c = dict(family=family, args=tuple(args), mode=mode, T=T, exact=None, K=1, varying=False, S=1, L=3, read=None, extreme=False,
             capital=CAPITAL, kind=DIV_FAST)
    c.update(kw)
    c["n"] = 64 * (8 if mode == "gauss" else 4) * 2 + 37
    c.setdefault("P", 9 if (mode == "table" and T <= DENSE) else 5)
    c["id"] = family.replace("_kernel", "") + mangled(family, args) + ("-extreme" if c["extreme"] else "")
    return c


def _rows():
    out = []
    for kmode, dense, mode, T in _modes():
        for exact in (False, True):
            div = dict(exact="flag", kind=DIV_EXACT) if exact else {}
            out.append(_case("checkpoints_kernel", (kmode, exact, dense), mode, T, **div))
            out.append(_case("excursions_kernel", (kmode, exact, dense), mode, T, **div))
            for varying in (False, True):
                out.append(_case("cashflow_kernel", (kmode, exact, dense, varying), mode, T, varying=varying, **div))
            for width, S in SWEEP_S.items():
                out.append(_case("cashflow_sweep_kernel", (kmode, exact, dense, width), mode, T, S=S, **div))
            for K in (1, 2, 3, 4):
                out.append(_case("portfolio_kernel", (kmode, exact, dense, K), mode, T, K=K, **div))
                for varying in (False, True):
                    out.append(_case("portfolio_cashflow_kernel", (kmode, exact, dense, K, varying), mode, T, K=K, varying=varying, **div))
    for dense, T in ((True, DENSE), (False, FOUR)):
        for wide in (False, True):
            read = "b128" if wide else "b32"
            out.append(_case("blocks_kernel", (DIV_FAST, dense, wide), "table", T, read=read))
            out.append(_case("blocks_kernel", (DIV_EXACT, dense, wide), "table", T, read=read, exact="flag", kind=DIV_EXACT))
            out.append(_case("blocks_kernel", (DIV_CHECKED, dense, wide), "table", T, read=read, exact="window", kind=DIV_CHECKED,
                             capital=2.0 ** 100, P=9))
    return out


def _extreme():
    """Per family and mode one case whose inputs tell the two divides apart; each reaches an exact-divide instantiation
    without the flag: the host cannot prove the fast divide for it."""
    out = []
    for kmode, dense, mode, T in _modes():
        if mode == "table" and not dense:
            continue
        x = dict(exact="unprovable", kind=DIV_EXACT, extreme=True, capital=EXTREME_CAPITAL[mode])
        out.append(_case("checkpoints_kernel", (kmode, True, dense), mode, T, **x))
        out.append(_case("excursions_kernel", (kmode, True, dense), mode, T, **x))
        out.append(_case("cashflow_kernel", (kmode, True, dense, True), mode, T, varying=True, **x))
        out.append(_case("cashflow_sweep_kernel", (kmode, True, dense, 4), mode, T, S=3, **x))
        if mode == "table":  # the smaller holding, 0.4 of the capital, starts where a single series does
            x = dict(x, capital=EXTREME_CAPITAL[mode] / 0.4)
        out.append(_case("portfolio_kernel", (kmode, True, dense, 2), mode, T, K=2, **x))
        out.append(_case("portfolio_cashflow_kernel", (kmode, True, dense, 2, False), mode, T, K=2, **x))
    out.append(_case("blocks_kernel", (DIV_EXACT, True, False), "table", DENSE, read="b32", exact="unprovable", kind=DIV_EXACT,
                     extreme=True, capital=EXTREME_CAPITAL["table"]))
    return out


# the extreme inputs: capitals a little above 2^-114 / 100 = 4.8e-37 (see the module's docstring), a Gaussian law that
# shrinks a path by 0.6 +- 0.2 per period, and the wild months
EXTREME_CAPITAL = {"table": 7.0e-37, "gauss": 4.0e-36}
EXTREME_GAUSS = (-40.0, 20.0)


# ---- inputs ----

@functools.lru_cache(maxsize=None)
def _series(T, kind):
    rng = np.random.default_rng(4000 + T)
    t = np.clip(rng.normal(0.6, 4.3, T), -25.0, 25.0).astype(f32)
    i = np.arange(T)
    if kind == "window":      # every eighth month +300 %: the fast divide is not provable from 2^100, the window rule holds
        t[i % 8 == 3] = 300.0
    elif kind == "wild":      # -99 % (a = 1), -100 % (a = 0) and 3e38 % months among the tame ones
        t[i % 16 == 1] = -99.0
        t[i % 64 == 5] = -100.0
        t[i % 64 == 7] = 3.0e38
    t.setflags(write=False)
    return t


def series(c):
    """The single-series returns table of a table-mode case (None in Gaussian mode)."""
    if c["mode"] != "table":
        return None
    if "table" in c:  # a fuzz case (tests/feature_fuzz.py) carries its own inputs; so below
        return c["table"]
    return _series(c["T"], "wild" if c["extreme"] else ("window" if c["exact"] == "window" else "tame"))


@functools.lru_cache(maxsize=None)
def _assets(T, K, wild):
    t = pref.asset_table(T, K)
    if wild:
        t = t.copy()
        i = np.arange(T)
        for k in range(K):
            t[i % 16 == 1 + k, k] = -99.0
        t[i % 64 == 5, 0] = -100.0
        t[i % 64 == 7, K - 1] = 3.0e38
        t.setflags(write=False)
    return t


def assets(c):
    """The joint table [T, K] of a table-mode portfolio case (None in Gaussian mode)."""
    if c["mode"] != "table":
        return None
    return c["assets"] if "assets" in c else _assets(c["T"], c["K"], c["extreme"])


def gauss_law(c):
    """(mean, std) of a single-series case in Gaussian mode."""
    if "law" in c:
        return c["law"]
    return EXTREME_GAUSS if c["extreme"] else (GAUSS_MEAN, GAUSS_STD)


def gauss_portfolio(c):
    """(means [K], factor [K, K]) of a Gaussian portfolio case."""
    if "pf" in c:
        return c["pf"]
    means, stds, corr = pref.gauss_setup(c["K"])
    if c["extreme"]:
        means, stds = [EXTREME_GAUSS[0] + 2.0 * k for k in range(c["K"])], [EXTREME_GAUSS[1] - 3.0 * k for k in range(c["K"])]
    return [float(m) for m in means], pref.factor_of(stds, corr)


def weights(c):
    return tuple(c["weights"]) if "weights" in c else pref.WEIGHTS[c["K"]]


def rebalance(c):
    return c.get("R", 2)


def checkpoints_of(c):
    if "periods" in c:
        return c["periods"]
    return [1, 4, 8, 9] if c["P"] == 9 else [1, 4, 5]


def levels(c):
    """(lower, target) of an excursions case: 0.9 and 1.1 of the capital (tame), 0.05 and 0.5 of it (extreme, shrinking)."""
    if "levels" in c:
        return c["levels"]
    lo, hi = (0.05, 0.5) if c["extreme"] else (0.9, 1.1)
    return float(f32(c["capital"] * lo)), float(f32(c["capital"] * hi))


def hist_range(c):
    """(n_bins, lo, hi, below) of a case's record: the module's for capital 1000, scaled with the capital otherwise."""
    if "hist" in c:
        return c["hist"]
    s = c["capital"] / CAPITAL
    return BINS, 0.0, float(f32(HI * s)), float(f32(BELOW * s))


def _level(growth, P, capital):
    """The constant amount that exhausts a path of total growth `growth` over P periods exactly at its end
    (portfolio_cashflow_reference._scale): with m = (1 + r)^P a level withdrawal A leaves capital (m - A (m - 1) / r)."""
    m = float(growth)
    r = m ** (1.0 / P) - 1.0
    return float(f32(capital * m * r / (m - 1.0))) if abs(m - 1.0) > 1e-9 else float(f32(capital / P))


def schedule(c, median_growth):
    """The cash-flow arguments of a case, sized by the case's own capital and median zero-flow growth so that about half
    of the paths are depleted: dict(amount, fraction, floor) or dict(amounts, fractions, floor); for a sweep a list of S
    (amount, fraction, floor).  The FAST rows keep to what the host's rules prove (csrc/smmc_cashflow.cpp: fractions in
    [0, 1], a positive floor; csrc/smmc_portfolio_cashflow.cpp: fraction 0 and a positive floor, or contributions only)."""
    if "schedule" in c:
        return c["schedule"]
    P, cap = c["P"], c["capital"]
    level = _level(median_growth, P, cap)
    floor = float(f32(FLOOR * cap / CAPITAL))
    if c["family"] == "cashflow_sweep_kernel":
        S = c["S"]
        return [(float(f32(level * (0.96 + 0.08 * s / max(S - 1, 1)))), 0.002 * (s % 2), float(f32(floor * (1 + 4000 * (s == 1))))) for s in range(S)]
    if not c["varying"]:
        return dict(amount=level, fraction=0.0, floor=floor)
    if c["family"] == "portfolio_cashflow_kernel" and c["kind"] == DIV_FAST:  # contributions only: what the rule proves
        return dict(amounts=(-0.02 * cap * (1 + np.arange(P) % 3)).astype(f32), fractions=np.zeros(P, f32), floor=floor)
    am = (level * np.linspace(0.6, 1.6, P)).astype(f32)
    am[0] = f32(-0.02 * cap)                                             # a contribution first
    return dict(amounts=am, fractions=np.where(np.arange(P) % 2 == 0, 0.0, 0.004).astype(f32), floor=floor)


# ---- multipliers and references ----

def _ids(c, seed, first):
    """(seed, first path) of a case: the module's unless the case or the caller names its own."""
    return (c.get("seed", SEED) if seed is None else seed), (c.get("first", FIRST_PATH) if first is None else first)


def single_multipliers(oracle, c, seed=None, first=None):
    """[n, P] multipliers of a single-series case, the oracle's own."""
    seed, first = _ids(c, seed, first)
    mean, std = gauss_law(c)
    mode = oracle.MODE_GAUSSIAN if c["mode"] == "gauss" else oracle.MODE_TABLE
    return cref.multipliers(oracle, mode, series(c), c["n"], c["P"], first_path=first, seed=seed, gauss_mean=mean, gauss_std=std)


def portfolio_multipliers(oracle, c, seed=None, first=None):
    """[n, P, K] multipliers of a portfolio case."""
    seed, first = _ids(c, seed, first)
    if c["mode"] == "table":
        return pref.table_multipliers(oracle, assets(c), seed, first, c["n"], c["P"])
    means, factor = gauss_portfolio(c)
    return pref.gauss_multipliers(oracle, means, factor, seed, first, c["n"], c["P"])


def block_indices(oracle, c, seed=None, first=None):
    """[n, P] table indices of a blocks case."""
    seed, first = _ids(c, seed, first)
    T, L, P = c["T"], c["L"], c["P"]
    s = bref.starts_bulk(oracle, series(c), seed, first, c["n"], -(-P // L))
    t = np.arange(P)
    return (s[:, t // L] + t % L) % T


def path_multipliers(oracle, c, seed=None, first=None):
    """The multipliers every product of a case is formed with: [n, P] or [n, P, K]."""
    if c["family"] in ("portfolio_kernel", "portfolio_cashflow_kernel"):
        return portfolio_multipliers(oracle, c, seed, first)
    if c["family"] == "blocks_kernel":
        return (f32(100.0) + series(c))[block_indices(oracle, c, seed, first)]
    return single_multipliers(oracle, c, seed, first)


def compound(a, capital):
    """[n, P + 1] plain compounding of the multipliers a [n, P] in binary32, and the products [n, P] it divides."""
    a = np.asarray(a, dtype=f32)
    n, P = a.shape
    v = np.empty((n, P + 1), f32)
    x = np.empty((n, P), f32)
    v[:, 0] = f32(capital)
    with np.errstate(all="ignore"):
        for t in range(P):
            x[:, t] = v[:, t] * a[:, t]
            v[:, t + 1] = x[:, t] / f32(100.0)
    return v, x


def fast_div100(x):
    """div100<false> of csrc/smmc_device.h restated: fma(x, ch, fl(x cl)) with 1/100 = ch + cl."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        return pref.fma32(x, f32(0.01), x * f32(float.fromhex("0x1.eb851ep-33")))


def products(oracle, c):
    """The products of the zero-flow paths of a case: [n, P] (a portfolio: [n, P * K], of the buy-and-hold holdings)."""
    a = path_multipliers(oracle, c)
    if a.ndim == 2:
        return compound(a, c["capital"])[1]
    w = np.asarray(weights(c), f32)
    return np.concatenate([compound(a[:, :, k], float(f32(c["capital"]) * w[k]))[1] for k in range(c["K"])], axis=1)


def left_window(oracle, c):
    """bool [n]: the path forms a product the fast divide is not proven for -- non-zero below 2^-114, or not finite."""
    x = products(oracle, c)
    with np.errstate(all="ignore"):
        return (((np.abs(x) < f32(TINY)) & (x != 0)) | ~np.isfinite(x)).any(axis=1)


def fast_divide_differs(oracle, c):
    """bool [n]: div100<false> of some product of the path is not the IEEE quotient's bits."""
    x = products(oracle, c)
    with np.errstate(all="ignore"):
        q = x / f32(100.0)
    fq = fast_div100(x)
    return ((q.view(np.uint32) != fq.view(np.uint32)) & ~(np.isnan(q) & np.isnan(fq))).any(axis=1)


def ends_degenerate(oracle, c):
    """bool [n]: the zero-flow path ends at inf, NaN, 0 or a subnormal."""
    a = path_multipliers(oracle, c)
    if a.ndim == 3:
        v = pref.simulate(a, weights(c), 0, capital=c["capital"])[0][:, -1]
    else:
        v = compound(a, c["capital"])[0][:, -1]
    return ~np.isfinite(v) | (np.abs(v) < np.finfo(f32).tiny)


def median_growth(oracle, c):
    """The median zero-flow growth of a case's paths over its P periods (1 where it is not a positive number)."""
    a = path_multipliers(oracle, c)
    with np.errstate(all="ignore"):
        if a.ndim == 3:
            v = pref.simulate(a, weights(c), 0, capital=c["capital"])[0][:, -1]
        else:
            v = compound(a, c["capital"])[0][:, -1]
        m = float(np.nanmedian(v.astype(np.float64))) / c["capital"]
    return m if math.isfinite(m) and m > 0 else 1.0


def trajectories(oracle, c, seed=None, first=None):
    """[n, P + 1] of a checkpoints or excursions case: the oracle engine's own."""
    seed, first = _ids(c, seed, first)
    mean, std = gauss_law(c)
    mode = oracle.MODE_GAUSSIAN if c["mode"] == "gauss" else oracle.MODE_TABLE
    p = oracle.make_params(mode, c["P"], c["n"], seed, first_path=first, initial_capital=c["capital"], table=series(c),
                           gauss_mean=mean, gauss_std=std)
    return oracle.counter_mc(p, want_final=False, want_traj=True)["traj"]


def reference(oracle, c):
    """What the entry point of a case must return, from the family's own restatement; per family:
    checkpoints: dict(traj); excursions: excursions_reference.excursions' dict; cashflow: dict(final, paid, ruin_period,
    depleted_at); sweep: a list of those; blocks: dict(final); portfolio: dict(final, holdings); portfolio cash flows:
    portfolio_cashflow_reference.simulate's dict.  Every dict also carries `args`, the feature's own arguments."""
    fam = c["family"]
    if fam == "checkpoints_kernel":
        return {"traj": trajectories(oracle, c), "args": checkpoints_of(c)}
    if fam == "excursions_kernel":
        out = xref.excursions(trajectories(oracle, c), *levels(c))
        out["args"] = levels(c)
        return out
    if fam == "blocks_kernel":
        a = path_multipliers(oracle, c)
        return {"final": compound(a, c["capital"])[0][:, -1].copy(), "args": c["L"]}
    sched = None if fam == "portfolio_kernel" else schedule(c, None if "schedule" in c else median_growth(oracle, c))
    if fam in ("cashflow_kernel", "cashflow_sweep_kernel"):
        a = single_multipliers(oracle, c)
        one = lambda am, fr, fl: dict(zip(("final", "paid", "ruin_period", "depleted_at"),  # noqa: E731
                                          cref.simulate_multipliers(a, am, fr, fl, c["capital"])))
        if fam == "cashflow_sweep_kernel":
            return {"scenarios": [one(*sc) for sc in sched], "args": sched}
        out = one(sched.get("amounts", sched.get("amount")), sched.get("fractions", sched.get("fraction")), sched["floor"])
        out["args"] = sched
        return out
    a = portfolio_multipliers(oracle, c)
    R = rebalance(c)
    if fam == "portfolio_kernel":
        values, holdings = pref.simulate(a, weights(c), R, capital=c["capital"])
        return {"final": values[:, -1].copy(), "holdings": holdings, "args": R}
    out = pcref.simulate(a, weights(c), R, capital=c["capital"], **sched)
    out["args"] = (R, sched)
    return out


def depleted_share(ref):
    """Share of depleted paths of a cash-flow reference (a sweep: per scenario)."""
    if "scenarios" in ref:
        return [float((r["ruin_period"] > 0).mean()) for r in ref["scenarios"]]
    return float((ref["ruin_period"] > 0).mean())


ROWS = _rows()
EXTREME = _extreme()
CASES = ROWS + EXTREME


def rows_of(family, cases=None):
    return [c for c in (CASES if cases is None else cases) if c["family"] == family]
