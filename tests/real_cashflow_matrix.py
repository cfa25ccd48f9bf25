"""The ledger of real_cashflow_kernel's instantiations, in the manner of tests/feature_matrix.py (whose helpers it uses and
which it does not edit): one row per compiled combination of <kMode, kExactDiv, kDense, K, kVarying> -- three rungs of
the mode ladder, two divides, K = 1 .. 3 invested assets, constant or per-period schedule: 36 -- with ONE request each
that makes the host choose it through smmc_engine_simulate_real_cashflow.  tests/test_real_cashflow_cpu.py compares ROWS
with the compiled symbol names; tests/test_real_cashflow_gpu.py runs every row, and the EXTREME ones, against reference().

Shapes are feature_matrix's: 64 kW 2 + 37 paths, 9 periods for dense tables and 5 otherwise, table lengths 2048 and 2049.
The joint table is portfolio_reference.asset_table(T, K + 1) with the inflation column of real_cashflow_reference
(0.25 + 0.1 c); the Gaussian law is real_cashflow_reference.gauss_law(K).

FAST rows.  The host proves the reciprocal-multiply form for contributions only (csrc/smmc_real_cashflow.cpp), so a FAST
row pays in 2 % of the capital (constant) or 2, 4, 6 % in turn (per period) and is depleted by its FLOOR: the median over
the paths of the lowest real value a path reaches with floor 0 -- about half of the paths pass under it.  The IEEE rows
are reached by the flag on the same laws with a withdrawal sized, as the other references size theirs, from the median
real zero-flow growth.  EXTREME adds one row per mode that starts near 2^-114 / 100 on wild ASSET series (the inflation
series stays tame: the index must stay a positive finite number for final_real to say anything): the host cannot prove
the fast divide for them, and a fast divide running where EXACT is due gives other bits."""
import functools

import numpy as np

import feature_matrix as M
import portfolio_reference as pref
import real_cashflow_reference as ref

f32 = np.float32
FAMILY = "real_cashflow_kernel"
SIGNATURE = "ibbib"
DIV_FAST, DIV_EXACT = M.DIV_FAST, M.DIV_EXACT


def mangled(args):
    """The template-argument list of an instantiation as it appears in the kernel's symbol."""
    return "I" + "".join(f"L{t}{int(v)}E" for t, v in zip(SIGNATURE, args)) + "E"


def _case(args, mode, T, **kw):
    c = dict(family=FAMILY, args=tuple(args), mode=mode, T=T, exact=None, K=1, varying=False, extreme=False, capital=M.CAPITAL,
             kind=DIV_FAST)
    c.update(kw)
    c["n"] = 64 * (8 if mode == "gauss" else 4) * 2 + 37
    c["P"] = 9 if (mode == "table" and T <= M.DENSE) else 5
    c["id"] = "real_cashflow" + mangled(args) + ("-extreme" if c["extreme"] else "")
    return c


def _rows():
    out = []
    for kmode, dense, mode, T in M._modes():
        for exact in (False, True):
            div = dict(exact="flag", kind=DIV_EXACT) if exact else {}
            for K in (1, 2, 3):
                for varying in (False, True):
                    out.append(_case((kmode, exact, dense, K, varying), mode, T, K=K, varying=varying, **div))
    return out


def _extreme():
    out = []
    for kmode, dense, mode, T in M._modes():
        if mode == "table" and not dense:
            continue
        cap = M.EXTREME_CAPITAL[mode] / (0.4 if mode == "table" else 1.0)  # the smaller holding starts where a single series does
        out.append(_case((kmode, True, dense, 2, False), mode, T, K=2, exact="unprovable", kind=DIV_EXACT, extreme=True, capital=cap))
    return out


ROWS = _rows()
EXTREME = _extreme()
CASES = ROWS + EXTREME


# ---- inputs ----

@functools.lru_cache(maxsize=None)
def _joint(T, K, wild):
    t = pref.asset_table(T, K + 1).copy()
    t[:, K] = f32(0.25) + f32(0.1) * t[:, K]
    if wild:  # feature_matrix's wild months, in the asset columns only
        i = np.arange(T)
        for k in range(K):
            t[i % 16 == 1 + k, k] = -99.0
        t[i % 64 == 5, 0] = -100.0
        t[i % 64 == 7, K - 1] = 3.0e38
    t.setflags(write=False)
    return t


def joint_table(c):
    """[T, K + 1] of a table-mode case (None in Gaussian mode)."""
    if c["mode"] != "table":
        return None
    return c["assets"] if "assets" in c else _joint(c["T"], c["K"], c["extreme"])


def gauss_law(c):
    """(means [K + 1], factor [K + 1, K + 1]) of a Gaussian case."""
    if "pf" in c:
        return c["pf"]
    means, factor = ref.gauss_law(c["K"])
    if c["extreme"]:  # feature_matrix's shrinking assets; the inflation series keeps its law
        K = c["K"]
        m, stds, corr = pref.gauss_setup(K + 1)
        m = [M.EXTREME_GAUSS[0] + 2.0 * k for k in range(K)] + [ref.INFLATION_MEAN]
        stds = [M.EXTREME_GAUSS[1] - 3.0 * k for k in range(K)] + [ref.INFLATION_STD]
        means, factor = [float(x) for x in m], pref.factor_of(stds, corr)
    return means, factor


def weights(c):
    return tuple(c["weights"]) if "weights" in c else pref.WEIGHTS[c["K"]]


def rebalance(c):
    return c.get("R", 2)


def multipliers(oracle, c):
    """[n, P, K + 1] joint multipliers of a case."""
    seed, first = c.get("seed", M.SEED), c.get("first", M.FIRST_PATH)
    if c["mode"] == "table":
        return pref.table_multipliers(oracle, joint_table(c), seed, first, c["n"], c["P"])
    means, factor = gauss_law(c)
    return pref.gauss_multipliers(oracle, means, factor, seed, first, c["n"], c["P"])


def schedule(oracle, c):
    """The cash-flow arguments of a case (see the module's docstring): dict(amount, fraction, floor) or dict(amounts,
    fractions, floor), amounts and floor in money of period 0."""
    if "schedule" in c:
        return c["schedule"]
    P, cap, a, w, R = c["P"], c["capital"], multipliers(oracle, c), weights(c), rebalance(c)
    if c["kind"] == DIV_FAST:  # contributions, and a floor that about half of the paths pass under
        flow = dict(amounts=(-0.02 * cap * (1 + np.arange(P) % 3)).astype(f32), fractions=np.zeros(P, f32)) if c["varying"] \
            else dict(amount=float(f32(-0.02 * cap)), fraction=0.0)
        run = ref.simulate(a, w, R, capital=cap, columns=True, **flow)
        with np.errstate(all="ignore"):
            lowest = (run["values"][:, 1:] / run["indices"][:, 1:]).min(axis=1)
        return dict(flow, floor=float(f32(np.median(lowest))))
    with np.errstate(all="ignore"):
        m = float(np.nanmedian(ref.simulate(a, w, 0, capital=cap)["final_real"].astype(np.float64))) / cap
    level = M._level(m if np.isfinite(m) and m > 0 else 1.0, P, cap)
    floor = float(f32(M.FLOOR * cap / M.CAPITAL))
    if not c["varying"]:
        return dict(amount=level, fraction=0.0, floor=floor)
    am = (level * np.linspace(0.6, 1.6, P)).astype(f32)
    am[0] = f32(-0.02 * cap)                                             # a contribution first
    return dict(amounts=am, fractions=np.where(np.arange(P) % 2 == 0, 0.0, 0.004).astype(f32), floor=floor)


def reference(oracle, c):
    """real_cashflow_reference.simulate's dict for a case, and `args`: (R, the schedule's keyword arguments)."""
    sched = schedule(oracle, c)
    out = ref.simulate(multipliers(oracle, c), weights(c), rebalance(c), capital=c["capital"], **sched)
    out["args"] = (rebalance(c), sched)
    return out


def hist_range(c):
    return M.hist_range(c)


def asset_products(oracle, c):
    """[n, P * K] products of the zero-flow buy-and-hold holdings of a case: what left_window() and fast_divide_differs()
    of tests/feature_matrix.py are stated on."""
    a = multipliers(oracle, c)
    w = np.asarray(weights(c), f32)
    return np.concatenate([M.compound(a[:, :, k], float(f32(c["capital"]) * w[k]))[1] for k in range(c["K"])], axis=1)
