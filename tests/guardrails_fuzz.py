"""Seeded random cases of smmc_engine_simulate_guardrails (the helper of tests/test_guardrails_fuzz_cpu.py and
tests/test_guardrails_fuzz_gpu.py, modelled on tests/real_cashflow_fuzz.py): any 64-bit seed, path ids up to 2^62, sizes
on both sides of a wave, a chunk and a Philox block, capitals from 1e-3 to 1e9, K = 1 .. 4 with a weight of exactly 0 now
and then, any R and E (0, 1, P and P + 1 among them), joint tables of 1, 2, 37, 2048 and 2049 rows, random Gaussian laws,
0 to 1000 buckets, the IEEE-divide flag (which changes nothing) in a quarter of the cases, and rules within the contract:
cut and raise factors of exactly 1 and far from it, an index below and above 1, open and shut clamps, open and closed
bands.  A case is a dict in the form of tests/guardrails_reference.py's, carrying its own inputs and its rule, so that
reference() restates it.

Against a vacuous fuzz the rule is sized from the case's own first 256 paths (guardrails_reference.sized_rule): the amount
from their median growth, the floor and the bands from quantiles the case draws.  tests/test_guardrails_fuzz_cpu.py
asserts that most cases cut some paths and not all, and deplete some and not all."""
import numpy as np

import feature_fuzz as F
import guardrails_reference as G

f32 = np.float32
SEED, COUNT = 19, 36
PERIODS = [1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 100, 360, 361]
PATHS = [1, 63, 64, 65, 255, 256, 257, 1000, 2047, 4100]  # at most a few thousand


def draw():
    """The COUNT cases as the module's fixed numpy seed draws them, without the rule: everything here is cheap, so a test
    can take case i alone and finish() it."""
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(COUNT):
        mode = ("table", "gauss")[int(rng.integers(2))]
        cap = float(rng.choice(F.CAPITALS))
        n_bins = int(rng.choice(F.BINS))
        K = int(rng.integers(1, 5))
        P = int(rng.choice(PERIODS))
        c = dict(i=i, mode=mode, T=int(rng.choice(F.ROWS, p=[0.1, 0.15, 0.25, 0.25, 0.25])), K=K, extreme=False,
                 exact=bool(rng.integers(4) == 0), capital=cap, id=f"guardrails#{i}",
                 seed=int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2)), first=int(rng.choice(F.FIRST)),
                 n=int(rng.choice(PATHS, p=[0.05] + [0.95 / 9] * 9)) + int(rng.integers(0, 3)), P=P,
                 hist=(n_bins, 0.0, float(f32(cap * float(rng.choice([2.0, 20.0])))), float(f32(cap * float(rng.choice([0.9, 1.0, 1.5]))))))
        w = rng.dirichlet(np.ones(K))
        if K > 1 and rng.integers(3) == 0:
            w[int(rng.integers(K))] = 0.0  # a weight of exactly 0
        w = (w / w.sum()).astype(f32)
        w[int(np.argmax(w))] += f32(1.0 - float(w.astype(np.float64).sum()))  # the sum within 1e-6 of 1
        c["weights"] = tuple(float(x) for x in w)
        c["R"] = int(rng.choice([0, 1, 5, 12, P, P + 1]))
        c["E"] = int(rng.choice([0, 1, 2, 3, 12, P, P + 1], p=[0.05, 0.25, 0.2, 0.2, 0.2, 0.05, 0.05]))
        if mode == "table":
            c["assets"] = rng.normal(0.6, 4.3, (c["T"], K)).astype(f32)
        else:  # random means and the Cholesky factor of a random covariance matrix
            g = rng.normal(0.0, 1.0, (K, K + 2))
            sd = rng.choice([0.5, 2.0, 4.3], K)
            corr = g @ g.T
            corr /= np.sqrt(np.outer(np.diag(corr), np.diag(corr)))
            c["pf"] = ([float(x) for x in rng.choice([0.0, 0.5, -0.25, 2.0], K)], np.linalg.cholesky(sd[:, None] * corr * sd[None, :]).astype(f32))
        lo = float(rng.choice([0.0, 0.2, 0.35, 0.5]))
        c["shape"] = dict(bands=(lo, float(rng.choice([lo, 0.65, 0.8, 1.0]) if lo < 0.65 else lo)), open_upper=bool(rng.integers(6) == 0),
                          cut=float(rng.choice([1.0, 0.9, 0.75, 0.25])), raise_=float(rng.choice([1.0, 1.1, 1.25, 3.0])),
                          index=float(rng.choice([1.0, 1.02, 0.97, 1.3])), amount_min=float(rng.choice([0.0, 0.5, 0.8, 1.0])),
                          amount_max=float(rng.choice([1.0, 1.5, 4.0, np.inf])), floor=float(rng.choice([0.0, 0.1, 0.25, 0.5])))
        out.append(c)
    return out


def finish(oracle, c):
    """The case with its rule: the drawn shape sized on the case's first 256 paths."""
    c, shape = dict(c), dict(c["shape"])
    open_upper = shape.pop("open_upper")
    rule = G.sized_rule(oracle, c, shape, head=256)
    if open_upper:
        rule["upper"] = G.INF
    if shape["bands"][0] == 0.0:
        rule["lower"] = 0.0
    c["rule"] = rule
    del c["shape"]
    return c


def cases(oracle):
    """The COUNT finished cases."""
    for c in draw():
        yield finish(oracle, c)


def within_the_contract(r):
    """The bounds the comments of smmc_guardrails state, on the binary32 values the library is given."""
    g = {k: (v if k == "review_every" else f32(v)) for k, v in r.items()}
    return bool(g["amount"] > 0 and np.isfinite(g["amount"]) and g["index"] > 0 and np.isfinite(g["index"]) and 0 <= g["lower"] <= g["upper"]
                and 0 < g["cut"] <= 1 and 1 <= g["raise_"] and np.isfinite(g["raise_"]) and 0 <= g["amount_min"] <= g["amount"] <= g["amount_max"]
                and g["floor"] >= 0 and np.isfinite(g["floor"]) and g["review_every"] >= 0)


brief = F.brief
