"""The guardrails contract of include/smmc.h (smmc_engine_simulate_guardrails) restated with numpy float32 over the
multipliers of tests/portfolio_reference.py: the reference of tests/test_guardrails_cpu.py, tests/test_guardrails_gpu.py and
the fuzz (tests/guardrails_fuzz.py).

Every operation is one numpy binary32 operation (numpy never fuses); the value is the left-to-right binary32 sum of the
holdings (portfolio_reference.value); fminf / fmaxf are np.fmin / np.fmax (the other operand for a NaN); a depleted path
is kept where it is by masks, never by the arithmetic.  The step up to the review is the one of
tests/portfolio_cashflow_reference.py with the per-path amount in force in the place of the schedule's entry.

CASES are the shapes of tests/feature_matrix.py -- 64 kW 2 + 37 paths, ids from 2^32 - 100 on, 9 periods on a dense table,
5 on a four-draw table and in Gaussian mode -- for every instantiation of guardrails_kernel: three rungs of the mode ladder
times K = 1 .. 4.  rule() sizes each case's amount, bands, clamps and floor from the case's own paths so that cuts,
raises, clamped amounts and depletion all happen and none happens to every path; tests/test_guardrails_cpu.py asserts
that on this restatement alone."""
import functools

import numpy as np

import feature_matrix as M
import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

f32 = np.float32
INF = float("inf")
SEED, FIRST_PATH, CAPITAL = M.SEED, M.FIRST_PATH, M.CAPITAL
BINS, LO, HI, BELOW = M.BINS, M.LO, M.HI, M.BELOW
OUTPUTS = ("final", "holdings", "paid", "ruin_period", "depleted_at", "amount_last", "amount_lowest", "cuts", "raises", "cuts_at",
           "raises_at")
SHARED = ("final", "holdings", "paid", "ruin_period", "depleted_at")  # what the parent call has too
RULE_KEYS = ("amount", "review_every", "upper", "lower", "cut", "raise_", "index", "amount_min", "amount_max", "floor")


def make_rule(amount, review_every=12, upper=INF, lower=0.0, cut=0.9, raise_=1.1, index=1.0, amount_min=0.0, amount_max=INF,
              floor=0.0):
    """The arguments of Engine.simulate_guardrails that make an smmc_guardrails, with its defaults, as binary32 values."""
    r = dict(amount=amount, review_every=int(review_every), upper=upper, lower=lower, cut=cut, raise_=raise_, index=index,
             amount_min=amount_min, amount_max=amount_max, floor=floor)
    return {k: (v if k == "review_every" else float(f32(v))) for k, v in r.items()}


def simulate(a, weights, rebalance_every, rule, capital=CAPITAL):
    """a [n, P, K] multipliers -> dict of final [n], holdings [K, n], paid [n], ruin_period [n] (uint32), depleted_at
    [P + 1] (uint64), amount_last [n], amount_lowest [n], cuts [n], raises [n] (uint32), cuts_at [P + 1], raises_at [P + 1]
    (uint64)."""
    a = np.asarray(a, dtype=f32)
    n, P, K = a.shape
    w_k = np.asarray(weights, dtype=f32)
    assert w_k.size == K
    R, E = int(rebalance_every), int(rule["review_every"])
    index, upper, lower, cut, raise_ = (f32(rule[k]) for k in ("index", "upper", "lower", "cut", "raise_"))
    amount_min, amount_max, floor = f32(rule["amount_min"]), f32(rule["amount_max"]), f32(rule["floor"])
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        h = [np.full(n, f32(capital) * w_k[k], dtype=f32) for k in range(K)]
        v = np.zeros(n, f32)
        paid = np.zeros(n, f32)
        ruin = np.zeros(n, np.uint32)
        alive = np.ones(n, bool)
        cur = np.full(n, f32(rule["amount"]), dtype=f32)
        lowest = cur.copy()
        cuts = np.zeros(n, np.uint32)
        raises = np.zeros(n, np.uint32)
        cuts_at = np.zeros(P + 1, np.uint64)
        raises_at = np.zeros(P + 1, np.uint64)
        for t in range(1, P + 1):
            hc = [(h[k] * a[:, t - 1, k]) / f32(100.0) for k in range(K)]
            g = pref.value(hc)
            w = cur
            vn = g - w
            ok = alive & (vn > floor)                # False for NaN
            dies = alive & ~ok
            if R and t % R == 0 and t != P:
                hn = [vn * w_k[k] for k in range(K)]
            else:
                hn = [hc[k] - w * w_k[k] for k in range(K)]
            paid = np.where(ok, paid + w, np.where(dies, paid + np.fmax(g, zero), paid)).astype(f32)
            h = [np.where(ok, hn[k], np.where(dies, zero, h[k])).astype(f32) for k in range(K)]
            v = np.where(ok, vn, np.where(dies, zero, v)).astype(f32)
            ruin[dies] = t
            alive = ok
            if E and t % E == 0 and t != P:
                c = cur * index
                is_cut = ok & (c > vn * upper)                  # False for NaN
                is_raise = ok & ~is_cut & (c < vn * lower)
                c = np.where(is_cut, c * cut, np.where(is_raise, c * raise_, c)).astype(f32)
                c = np.fmin(np.fmax(c, amount_min), amount_max)
                cur = np.where(ok, c, cur).astype(f32)
                lowest = np.fmin(lowest, cur)
                cuts += is_cut
                raises += is_raise
                cuts_at[t] = np.count_nonzero(is_cut)
                raises_at[t] = np.count_nonzero(is_raise)
    assert all(x.dtype == f32 for x in h) and all(x.dtype == f32 for x in (v, paid, cur, lowest))
    return {"final": v, "holdings": np.stack(h), "paid": paid, "ruin_period": ruin,
            "depleted_at": np.bincount(ruin, minlength=P + 1).astype(np.uint64), "amount_last": cur, "amount_lowest": lowest,
            "cuts": cuts, "raises": raises, "cuts_at": cuts_at, "raises_at": raises_at}


def indexed_amounts(rule, P):
    """float32 [P]: the amount in force in every period when no band and no clamp ever acts -- A0 multiplied by `index`
    once per passed review, in binary32 (identity 2: the parent call's amounts[])."""
    E = int(rule["review_every"])
    out = np.empty(P, f32)
    cur = f32(rule["amount"])
    for t in range(1, P + 1):
        out[t - 1] = cur
        if E and t % E == 0 and t != P:
            cur = f32(cur * f32(rule["index"]))
    return out


# ---- the cases run on the device ----

def case(mode, T, K, **kw):
    """A case in the manner of tests/feature_matrix.py (its helpers read mode, T, K, n, P, capital, extreme and, from a
    fuzz case, assets / pf / weights / seed / first)."""
    c = dict(mode=mode, T=T, K=K, capital=CAPITAL, extreme=False)
    c.update(kw)
    c.setdefault("n", 64 * (8 if mode == "gauss" else 4) * 2 + 37)
    c.setdefault("P", 9 if (mode == "table" and T <= M.DENSE) else 5)
    c.setdefault("E", 2)
    c.setdefault("R", 4 if c["P"] == 9 else 3)   # with E = 2 and P = 9: reviews with a rebalance (4, 8) and without one (2, 6)
    c.setdefault("id", f"{mode}{T or ''}-K{K}-P{c['P']}-E{c['E']}-R{c['R']}" + (f"-{kw['edge']}" if "edge" in kw else ""))
    return c


MODES = [("gauss", 0), ("table", M.DENSE), ("table", M.FOUR)]
CASES = [case(mode, T, K) for mode, T in MODES for K in (1, 2, 3, 4)]
# the edges: one period; a review after every period; E = P (no review at P, so none at all); E > P; clamps shut; a
# review that falls with a rebalance inside the partial block (a whole block and a partial one of three periods)
EDGES = [case("table", M.DENSE, 2, P=1, edge="P1"), case("gauss", 0, 2, E=1, edge="E1"), case("table", M.FOUR, 4, E=5, edge="EP"),
         case("table", M.DENSE, 1, E=10, edge="EgtP"), case("gauss", 0, 4, edge="shut"),
         case("table", M.FOUR, 3, P=7, E=3, R=2, edge="partial"), case("table", M.DENSE, 3, P=11, E=5, R=2, edge="partial")]


def multipliers(oracle, c):
    return M.portfolio_multipliers(oracle, c)


def weights(c):
    return M.weights(c)


def _quantile32(x, q, least=0.0):
    """The quantile of the finite entries as a binary32 value, at least `least` (and `least` where there is none)."""
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x)]
    return max(float(f32(np.quantile(x, q))), least) if x.size else least


# how rule() shapes a rule; the fuzz draws its own
SHAPE = dict(bands=(0.35, 0.65), cut=0.75, raise_=1.25, index=1.02, amount_min=0.8, amount_max=1.5, floor=0.25)


def sized_rule(oracle, c, shape=None, head=None):
    """The smmc_guardrails of a case, sized by the case's own paths (as feature_matrix.schedule sizes a schedule by the
    median growth), from the PARENT restatements alone; with the module's SHAPE:
      amount      twice the median per-period growth of the zero-flow paths times the capital, at least 0.4 % of it;
      floor       the lower quartile of the lowest value the paths take with that constant amount: about a quarter deplete;
      bands       the 35 % and 65 % quantiles of the withdrawal rate fl(A0 index) / v at the first review (where there is
                  none: at the last period) -- about a third is cut there, a third raised, a third left;
      cut, raise  0.75 and 1.25, index 1.02, clamps [0.8 A0, 1.5 A0]: a first cut is clamped, a second raise too.
    head: size on the first `head` paths only."""
    shape = SHAPE if shape is None else shape
    if head is not None:
        c = dict(c, n=min(c["n"], head))
    P, E, R, cap = c["P"], c["E"], c["R"], c["capital"]
    a, w = multipliers(oracle, c), weights(c)
    with np.errstate(all="ignore"):
        m = float(np.nanmedian(pref.simulate(a, w, R, capital=cap)[0][:, -1].astype(np.float64))) / cap
        growth = (m if np.isfinite(m) and m > 1e-3 else 1e-3) ** (1.0 / P) - 1.0
        amount = float(f32(cap * max(2.0 * growth, 0.004)))
        values = pcref.simulate(a, w, R, amount=amount, capital=cap, columns=True)["values"]
        floor = _quantile32(values[:, 1:].min(axis=1), shape["floor"])
        rate = float(f32(f32(amount) * f32(shape["index"]))) / values[:, E if 0 < E < P else P].astype(np.float64)
    lower = _quantile32(rate, shape["bands"][0])
    return make_rule(amount, E, upper=_quantile32(rate, shape["bands"][1], lower), lower=lower, cut=shape["cut"], raise_=shape["raise_"],
                     index=shape["index"], amount_min=shape["amount_min"] * amount, amount_max=shape["amount_max"] * amount, floor=floor)


def rule(oracle, c):
    """The smmc_guardrails of a case: sized_rule() with the module's SHAPE, computed once.  A case that carries its own
    `rule` (the fuzz) keeps it; the edge 'shut' has amount_min == A0 == amount_max."""
    if "rule" in c:
        return c["rule"]
    return dict(_rule(oracle, c["mode"], c["T"], c["K"], c["n"], c["P"], c["E"], c["R"], c.get("edge") == "shut"))


@functools.lru_cache(maxsize=None)
def _rule(oracle, mode, T, K, n, P, E, R, shut):
    r = sized_rule(oracle, case(mode, T, K, n=n, P=P, E=E, R=R))
    if shut:
        r["amount_min"] = r["amount_max"] = r["amount"]
    return tuple(r.items())


@functools.lru_cache(maxsize=None)
def _reference(oracle, key):
    c = _BY_ID[key]
    out = simulate(multipliers(oracle, c), weights(c), c["R"], rule(oracle, c), capital=c["capital"])
    for x in out.values():
        x.setflags(write=False)
    return out


_BY_ID = {c["id"]: c for c in CASES + EDGES}
assert len(_BY_ID) == len(CASES) + len(EDGES)


def reference(oracle, c):
    """simulate() of a case: CASES and EDGES computed once and shared, never modified; any other case (the fuzz) afresh."""
    if c["id"] in _BY_ID and _BY_ID[c["id"]] is c:
        return _reference(oracle, c["id"])
    return simulate(multipliers(oracle, c), weights(c), c["R"], rule(oracle, c), capital=c["capital"])


def hist_range(c):
    return c["hist"] if "hist" in c else (BINS, LO, HI, BELOW)
