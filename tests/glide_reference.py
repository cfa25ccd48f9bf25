"""The glide-path contract of include/smmc.h (smmc_engine_simulate_glide) restated with numpy float32 over the oracle's
multipliers: tests/portfolio_cashflow_reference.py's recurrence with the weights indexed by period -- every trade at the
end of period t (the initial purchase at t = 0, a rebalance or the settlement of the flow after) uses W(t), the row of the
last change with after <= t, the call's own weights before the first.  The reference of tests/test_glide_cpu.py,
tests/test_glide_gpu.py and the two fuzz tests, and the list of the cases they run.

A case is a dict in the form of tests/feature_matrix.py's portfolio cash-flow cases (its inputs, schedule sizing and
multipliers are that module's), with R, `changes` -- a tuple of (after, weights) -- and `glide`, the instantiation's
template arguments.  Shapes as there: 64 kW 2 + 37 paths with kW = 4 (table) or 8 (Gaussian), ids from 2^32 - 100 on, 9
periods on a dense table (eight draws per Philox block) and 5 on a four-draw table and in Gaussian mode, R = 3."""
import functools

import numpy as np

import feature_matrix as M
import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

f32 = np.float32
SEED, FIRST_PATH, CAPITAL = M.SEED, M.FIRST_PATH, M.CAPITAL
R = 3
MAX_ASSETS, MAX_CHANGES = 4, 512
KEYS = ("final", "holdings", "paid", "ruin_period", "depleted_at")
# target vectors per K beside pref.WEIGHTS[K], every weight positive, each summing to 1 within 1e-6 as binary32
ROWS = {2: ((0.2, 0.8), (0.85, 0.15), (0.45, 0.55)),
        3: ((0.1, 0.2, 0.7), (0.7, 0.2, 0.1), (0.25, 0.5, 0.25)),
        4: ((0.05, 0.15, 0.3, 0.5), (0.55, 0.25, 0.15, 0.05), (0.1, 0.4, 0.4, 0.1))}
# a vector that takes an asset to weight 0 (the row after it brings it back)
ROWS_WITH_ZERO = {2: (0.0, 1.0), 3: (0.5, 0.0, 0.5), 4: (0.25, 0.5, 0.0, 0.25)}


def weights_at(weights, changes, P):
    """[P + 1, K] float32: W(t) for t = 0 .. P."""
    w = np.empty((P + 1, len(weights)), f32)
    w[:] = np.asarray(weights, f32)
    for after, row in changes:  # strictly increasing: a later change overwrites the tail of an earlier one
        if after <= P:
            w[after:] = np.asarray(row, f32)[:len(weights)]
    return w


def simulate(a, weights, changes, rebalance_every, amount=0.0, fraction=0.0, floor=0.0, amounts=None, fractions=None, capital=CAPITAL):
    """a [n, P, K] multipliers -> portfolio_cashflow_reference.simulate's dict for the glide path (weights, changes)."""
    a = np.asarray(a, dtype=f32)
    n, P, K = a.shape
    W = weights_at(weights, changes, P)
    Rb = int(rebalance_every)
    am = np.broadcast_to(np.asarray(amount if amounts is None else amounts, f32), (P,))
    fr = np.broadcast_to(np.asarray(fraction if fractions is None else fractions, f32), (P,))
    floor, zero = f32(floor), f32(0.0)
    with np.errstate(all="ignore"):
        h = [np.full(n, f32(capital) * W[0, k], dtype=f32) for k in range(K)]
        v = pref.value(h)
        paid = np.zeros(n, f32)
        ruin = np.zeros(n, np.uint32)
        alive = np.ones(n, bool)
        for t in range(1, P + 1):
            hc = [(h[k] * a[:, t - 1, k]) / f32(100.0) for k in range(K)]
            g = pref.value(hc)
            w = am[t - 1] + g * fr[t - 1]
            vn = g - w
            ok = alive & (vn > floor)
            dies = alive & ~ok
            if Rb and t % Rb == 0 and t != P:
                hn = [vn * W[t, k] for k in range(K)]
            else:
                hn = [hc[k] - w * W[t, k] for k in range(K)]
            paid = np.where(ok, paid + w, np.where(dies, paid + np.fmax(g, zero), paid)).astype(f32)
            h = [np.where(ok, hn[k], np.where(dies, zero, h[k])).astype(f32) for k in range(K)]
            v = np.where(ok, vn, np.where(dies, zero, v)).astype(f32)
            ruin[dies] = t
            alive = ok
    assert all(x.dtype == f32 for x in h) and v.dtype == f32 and paid.dtype == f32
    return {"final": v, "holdings": np.stack(h), "paid": paid, "ruin_period": ruin,
            "depleted_at": np.bincount(ruin, minlength=P + 1).astype(np.uint64)}


# ---- the cases ----

def _case(kmode, dense, mode, T, exact, K, varying, changes, tag, **kw):
    c = M._case("portfolio_cashflow_kernel", (kmode, exact, dense, K, varying), mode, T, K=K, varying=varying,
                **(dict(exact="flag", kind=M.DIV_EXACT) if exact else {}))
    c.update(R=R, changes=tuple((int(a), tuple(float(x) for x in w)) for a, w in changes), glide=(kmode, exact, dense, K, varying))
    if kw.pop("unprovable", False):
        c["exact"] = "unprovable"  # the IEEE divide without the flag: the host cannot prove the fast one
    c.update(kw)
    c["id"] = "glide" + M.mangled("portfolio_cashflow_kernel", c["glide"]) + ("-" + tag if tag else "")
    return c


def _instantiations():
    """One case per instantiation: a change off the rebalance periods and one on a rebalance period, every weight positive;
    the rows without the flag are FAST by the rule (a constant amount and a positive floor, or contributions only)."""
    out = []
    for kmode, dense, mode, T in M._modes():
        P = 9 if dense else 5
        for exact in (False, True):
            for K in (2, 3, 4):
                for varying in (False, True):
                    out.append(_case(kmode, dense, mode, T, exact, K, varying, ((2, ROWS[K][0]), (6 if dense else 3, ROWS[K][1])), ""))
    return out


def _edges():
    out = []
    for kmode, dense, mode, T, K in ((M.MODE_TABLE, True, "table", M.DENSE, 2), (M.MODE_GAUSSIAN, False, "gauss", 0, 3)):
        P, B = (9, 8) if dense else (5, 4)  # B: the last period of the first Philox block
        a, b, z = ROWS[K][0], ROWS[K][1], ROWS_WITH_ZERO[K]
        named = {"after1": ((1, a),), "boundary": ((B, a),), "past_boundary": ((B + 1, a),), "on_rebalance": ((3, a),),
                 "off_rebalance": ((4, a),), "before_last": ((P - 1, a),), "at_last": ((P, a),), "beyond": ((P + 1, a), (P + 7, b)),
                 "consecutive": ((2, a), (3, b)),
                 "most": tuple((t, ROWS[K][t % 3]) for t in range(1, MAX_CHANGES + 1))}
        for edge, changes in named.items():
            out.append(_case(kmode, dense, mode, T, False, K, False, changes, edge, edge=edge))
        # an asset taken to weight 0 and brought back: the rule cannot prove the fast divide, no flag needed
        out.append(_case(kmode, dense, mode, T, True, K, False, ((2, z), (4, b)), "zero_and_back", edge="zero_and_back", unprovable=True))
    return out


CASES = _instantiations()
EDGES = _edges()
ALL_CASES = CASES + EDGES


def weights(c):
    return M.weights(c)


def multipliers(oracle, c, seed=None, first=None):
    return M.portfolio_multipliers(oracle, c, seed, first)


hist_range = M.hist_range


def is_identity(c):
    """No change can reach a trade that moves the final value or a holding: none at or before P."""
    return not any(a <= c["P"] for a, _ in c["changes"])


def fast_varying(c):
    """A FAST row with per-period amounts: contributions only, so nothing depletes (exempt, as in the parent's ledger)."""
    return c["varying"] and c["kind"] == M.DIV_FAST


def _scaled(sched, s):
    """The schedule with every withdrawal (a positive amount) multiplied by s, rounded to binary32."""
    out = dict(sched)
    if "amounts" in out:
        am = np.asarray(out["amounts"], f32)
        out["amounts"] = np.where(am > 0, (am.astype(np.float64) * s).astype(f32), am).astype(f32)
    elif out["amount"] > 0:
        out["amount"] = float(f32(out["amount"] * s))
    return out


def sized_schedule(oracle, c):
    """feature_matrix.schedule's shapes for a case, sized on the restatement alone: from the median zero-flow growth of the
    case's OWN glide path, then its withdrawals scaled by the factor a bisection over [2^-8, 2^8] finds, stopping at the
    first at which between 20 % and 40 % of the paths deplete -- fewer than half, so that the final values of more than
    half can differ from the run without changes.  A schedule of contributions only (a FAST row with per-period amounts)
    depletes nothing and is taken as it is."""
    a = multipliers(oracle, c)
    zero = simulate(a, weights(c), c["changes"], c["R"], capital=c["capital"])["final"].astype(np.float64)
    m = float(np.nanmedian(zero)) / c["capital"]
    base = M.schedule(c, m if np.isfinite(m) and m > 0 else 1.0)
    if fast_varying(c):
        return base
    lo, hi, sched = -8.0, 8.0, base
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        sched = _scaled(base, 2.0 ** mid)
        share = depleted_share(simulate(a, weights(c), c["changes"], c["R"], capital=c["capital"], **sched))
        if 0.2 <= share <= 0.4:
            break
        lo, hi = (mid, hi) if share < 0.2 else (lo, mid)
    return sched


@functools.lru_cache(maxsize=None)
def _schedule(oracle, cid):
    return sized_schedule(oracle, BY_ID[cid])


def schedule(oracle, c):
    """The cash-flow arguments of a case (a fuzz case carries its own)."""
    if "schedule" in c:
        return c["schedule"]
    return _schedule(oracle, c["id"])


@functools.lru_cache(maxsize=None)
def _reference(oracle, cid, glide):
    c = BY_ID[cid]
    out = simulate(multipliers(oracle, c), weights(c), c["changes"] if glide else (), c["R"], capital=c["capital"], **schedule(oracle, c))
    for x in out.values():
        x.setflags(write=False)
    return out


def reference(oracle, c, glide=True):
    """simulate() of a listed case (glide=False: of the same case without its changes): computed once, shared, read-only."""
    if c["id"] in BY_ID and BY_ID[c["id"]] is c:
        return _reference(oracle, c["id"], bool(glide))
    return simulate(multipliers(oracle, c), weights(c), c["changes"] if glide else (), c["R"], capital=c["capital"], **schedule(oracle, c))


BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)


def depleted_share(out):
    return float((out["ruin_period"] > 0).mean())


def differing_share(a, b):
    """Share of paths whose final values differ in bits."""
    return float((np.ascontiguousarray(a["final"]).view(np.uint32) != np.ascontiguousarray(b["final"]).view(np.uint32)).mean())


def parent(oracle, c, w=None):
    """portfolio_cashflow_reference.simulate of the case's paths and schedule at one weight vector."""
    return pcref.simulate(multipliers(oracle, c), weights(c) if w is None else w, c["R"], capital=c["capital"], **schedule(oracle, c))


# ---- the divide rule on the restatement ----

def products(oracle, c):
    """[n, P * K] every product h_k * a_k(t) the case's paths form (a depleted path's are 0)."""
    a = multipliers(oracle, c)
    n, P, K = a.shape
    W = weights_at(weights(c), c["changes"], P)
    s = schedule(oracle, c)
    am = np.broadcast_to(np.asarray(s.get("amounts", s.get("amount", 0.0)), f32), (P,))
    fr = np.broadcast_to(np.asarray(s.get("fractions", s.get("fraction", 0.0)), f32), (P,))
    floor, zero = f32(s.get("floor", 0.0)), f32(0.0)
    out = np.empty((n, P, K), f32)
    with np.errstate(all="ignore"):
        h = [np.full(n, f32(c["capital"]) * W[0, k], dtype=f32) for k in range(K)]
        alive = np.ones(n, bool)
        for t in range(1, P + 1):
            for k in range(K):
                out[:, t - 1, k] = h[k] * a[:, t - 1, k]
            hc = [out[:, t - 1, k] / f32(100.0) for k in range(K)]
            g = pref.value(hc)
            w = am[t - 1] + g * fr[t - 1]
            vn = g - w
            ok = alive & (vn > floor)
            if c["R"] and t % c["R"] == 0 and t != P:
                hn = [vn * W[t, k] for k in range(K)]
            else:
                hn = [hc[k] - w * W[t, k] for k in range(K)]
            h = [np.where(ok, hn[k], zero).astype(f32) for k in range(K)]
            alive = ok
    return out.reshape(n, P * K)


# ---- seeded random cases ----

FUZZ_SEED, FUZZ_COUNT = 23, 36
FUZZ_PERIODS = [2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 24]
FUZZ_PATHS = [63, 64, 65, 255, 256, 257, 1000, 2047, 2998]
FUZZ_FIRST = [0, 1, 255, (1 << 32) - 300, (1 << 32), (1 << 45) + 12345, (1 << 62) - 7000]
FUZZ_ROWS = [37, 2048, 2049]  # a table of one or two rows has too few distinct paths to size a schedule on


def _random_weights(rng, K, zero_ok):
    w = rng.dirichlet(np.ones(K))
    if zero_ok and rng.integers(4) == 0:
        w[int(rng.integers(K))] = 0.0
    w = (w / w.sum()).astype(f32)
    w[int(np.argmax(w))] += f32(1.0 - float(w.astype(np.float64).sum()))  # the sum within 1e-6 of 1
    return tuple(float(x) for x in w)


def fuzz_draw():
    """The FUZZ_COUNT cases as the fixed numpy seed draws them, without their schedules."""
    rng = np.random.default_rng(FUZZ_SEED)
    out = []
    for i in range(FUZZ_COUNT):
        mode = ("table", "gauss")[int(rng.integers(2))]
        K = int(rng.integers(1, 5))
        P = int(rng.choice(FUZZ_PERIODS))
        cap = float(rng.choice([1.0, 1000.0, 12345.678, 1e9]))
        n_bins = int(rng.choice([0, 1, 7, 100]))
        varying = bool(rng.integers(2))
        c = dict(i=i, family="portfolio_cashflow_kernel", mode=mode, T=int(rng.choice(FUZZ_ROWS)), K=K,
                 extreme=False, exact="flag" if rng.integers(4) == 0 else None, kind=None, capital=cap, varying=varying, id=f"glide#{i}",
                 seed=int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2)), first=int(rng.choice(FUZZ_FIRST)),
                 n=int(rng.choice(FUZZ_PATHS)) + int(rng.integers(0, 3)), P=P,
                 hist=(n_bins, 0.0, float(f32(cap * 4.0)), float(f32(cap))))
        c["weights"] = _random_weights(rng, K, K > 1)
        c["R"] = int(rng.choice([0, 1, 2, 3, 5, P, P + 1]))
        n_changes = int(rng.integers(0, 7))
        after = sorted(set(int(x) for x in rng.integers(1, P + 3, n_changes)))
        c["changes"] = tuple((t, _random_weights(rng, K, K > 1)) for t in after)
        if mode == "table":
            c["assets"] = rng.normal(0.6, 4.3, (c["T"], K)).astype(f32)
        else:
            g = rng.normal(0.0, 1.0, (K, K + 2))
            sd = rng.choice([0.5, 2.0, 4.3], K)
            corr = g @ g.T
            corr /= np.sqrt(np.outer(np.diag(corr), np.diag(corr)))
            c["pf"] = ([float(x) for x in rng.choice([0.0, 0.5, -0.25, 2.0], K)], np.linalg.cholesky(sd[:, None] * corr * sd[None, :]).astype(f32))
        c["contributions_only"] = bool(varying and rng.integers(4) == 0)
        out.append(c)
    return out


def fuzz_finish(oracle, c):
    """The case with its schedule (sized_schedule); `depletes`: whether the schedule takes anything out."""
    c = dict(c)
    only_in = c.pop("contributions_only")
    shape = dict(c, kind=M.DIV_FAST if only_in else None)
    c["schedule"] = sized_schedule(oracle, shape)
    c["depletes"] = not only_in
    return c


def fuzz_cases(oracle):
    for c in fuzz_draw():
        yield fuzz_finish(oracle, c)


def brief(c):
    return {k: (v if not isinstance(v, np.ndarray) else v.shape) for k, v in c.items() if k not in ("table", "assets", "pf")}
