"""Seeded random cases of smmc_engine_simulate_portfolio_cashflow_regimes (the helper of
tests/test_portfolio_cashflow_regimes_fuzz_cpu.py and tests/test_portfolio_cashflow_regimes_fuzz_gpu.py, in the style of
tests/portfolio_cashflow_stationary_fuzz.py).  Every field comes from a generator of this module's own: any 64-bit seed,
path ids up to 2^62, sizes on both sides of a wave and a chunk, capitals from 1e-3 to 1e9, K = 1 .. 4 with a weight of
exactly 0 now and then, two random laws per case (means, deviations and a random correlation matrix each, small enough for
the divide rule's bounds), P <= 64, any R (0, 1, 8, P and P + 1 among them), 0 to 1000 buckets, the IEEE-divide flag in a
quarter of the cases, four forms of schedule, and the three probabilities: 0 and 65536 now and then, else any value, half of
them small (long sojourns).

Against a vacuous fuzz the schedule is sized from the case's own first 256 paths (finish), as there."""
import numpy as np

import feature_fuzz as F
import portfolio_cashflow_blocks_fuzz as BF
import portfolio_cashflow_blocks_reference as B
import portfolio_cashflow_reference as pcref
import portfolio_cashflow_regimes_reference as Q
import portfolio_reference as pref

f32 = np.float32
SEED, COUNT = 31, 40
PATHS = BF.PATHS
FORMS = BF.FORMS


def _q16(rng):
    pick = int(rng.integers(6))
    return int(rng.choice([0, Q.ONE])) if pick == 0 else int(rng.integers(0, 8192)) if pick < 3 else int(rng.integers(0, Q.ONE + 1))


def _law(rng, K):
    means = rng.uniform(-2.0, 1.5, K)
    stds = rng.uniform(0.5, 4.0, K)  # row sums of |L| stay below 8: 100 + mean - 7 * 8 > 0, the divide rule has its bounds
    g = rng.normal(size=(K, K + 2))
    c = g @ g.T
    d = np.sqrt(np.diag(c))
    return tuple(float(f32(x)) for x in means), pref.factor_of(stds, c / d[:, None] / d[None, :])


def draw():
    """The COUNT cases as the module's fixed numpy seed draws them, without the schedule's scale: cheap, so a test can take
    case i alone and finish() it."""
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(COUNT):
        cap = float(rng.choice(F.CAPITALS))
        n_bins = int(rng.choice(F.BINS))
        K = int(rng.integers(1, 5))
        P = int(rng.integers(1, 65))
        c = dict(i=i, K=K, P=P, prob=((_q16(rng), _q16(rng)), _q16(rng)), exact=bool(rng.integers(4) == 0), capital=cap,
                 id=f"portfolio_cashflow_regimes#{i}", seed=int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2)), first=int(rng.choice(F.FIRST)),
                 n=int(rng.choice(PATHS)) + int(rng.integers(0, 3)), form=str(rng.choice(FORMS, p=[0.3, 0.2, 0.35, 0.15])),
                 hist=(n_bins, 0.0, float(f32(cap * float(rng.choice([2.0, 20.0])))), float(f32(cap * float(rng.choice([0.9, 1.0, 1.5]))))))
        w = rng.dirichlet(np.ones(K))
        if K > 1 and rng.integers(3) == 0:
            w[int(rng.integers(K))] = 0.0  # a weight of exactly 0
        w = (w / w.sum()).astype(f32)
        w[int(np.argmax(w))] += f32(1.0 - float(w.astype(np.float64).sum()))  # the sum within 1e-6 of 1
        c["weights"] = tuple(float(x) for x in w)
        c["R"] = int(rng.choice([0, 1, 5, 8, 12, P, P + 1]))
        (m0, f0), (m1, f1) = _law(rng, K), _law(rng, K)
        c["means"], c["factors"] = (m0, m1), (f0, f1)
        c["shape"] = dict(share=float(rng.choice([0.3, 0.5, 0.7])), floor=float(rng.choice([0.0, 0.0, 1e-5, 0.1])),
                          ramp=(float(rng.choice([0.5, 1.1])), float(rng.choice([1.5, 2.5]))), lead=int(rng.integers(0, P)),
                          fractions=bool(rng.integers(2)))
        out.append(c)
    return out


def multipliers(oracle, c, n=None):
    return Q.multipliers_of(oracle, c["means"], c["factors"], c["n"] if n is None else n, c["P"], c["prob"], c["seed"], c["first"])


def finish(oracle, c):
    """The case with its schedule (keyword arguments of simulate and of the call): the drawn shape sized on the case's
    first 256 paths, by the block fuzz's procedure on these paths."""
    c, shape = dict(c), c["shape"]
    P, cap = c["P"], c["capital"]
    a = multipliers(oracle, c, min(c["n"], 256))
    m = max(float(np.median(pcref.simulate(a, c["weights"], 0, capital=cap)["final"])) / cap, 1e-3)
    r = m ** (1.0 / P) - 1.0
    level = cap * m * r / (m - 1.0) if abs(m - 1.0) > 1e-9 else cap / P  # exhausts the median path at the end of the run
    if c["form"] == "amount":
        kw = dict(amount=float(f32(level)), floor=float(f32(shape["floor"] * cap)))
    elif c["form"] == "fraction":
        kw = dict(fraction=0.03, floor=float(f32(np.median(pcref.simulate(a, c["weights"], 0, fraction=0.03, capital=cap)["final"]))))
    elif c["form"] == "varying":
        lead = shape["lead"]
        kw = dict(amounts=np.concatenate([np.full(lead, -0.02 * cap), np.linspace(*shape["ramp"], P - lead) * level]).astype(f32),
                  floor=float(f32(shape["floor"] * cap)))
        if shape["fractions"]:
            kw["fractions"] = np.concatenate([np.zeros(lead), np.full(P - lead, 0.004)]).astype(f32)
    else:
        kw = dict(amounts=(-np.linspace(0.03, 0.001, P) * cap).astype(f32))
    if c["form"] != "contributions":
        def depleted(f):
            return float((pcref.simulate(a, c["weights"], c["R"], capital=cap, **B._resized(kw, f))["ruin_period"] > 0).mean())
        lo, hi = 0.0, 8.0
        if depleted(lo) < shape["share"] <= depleted(hi):
            for _ in range(30):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if depleted(mid) < shape["share"] else (lo, mid)
            kw = B._resized(kw, hi)
    c["schedule"] = kw
    del c["shape"]
    return c


def cases(oracle):
    """The COUNT finished cases."""
    for c in draw():
        yield finish(oracle, c)


def reference(oracle, c):
    """The restatement of a finished case: portfolio_cashflow_reference.simulate on the regime multipliers."""
    return pcref.simulate(multipliers(oracle, c), c["weights"], c["R"], capital=c["capital"], **c["schedule"])


def instantiation(c):
    """(K, varying schedule): with the divide the launch takes, which of the 16 kernels a case runs."""
    return c["K"], "amounts" in c["schedule"] or "fractions" in c["schedule"]


def brief(c):
    return {k: v for k, v in F.brief(c).items() if k not in ("schedule", "factors")}
