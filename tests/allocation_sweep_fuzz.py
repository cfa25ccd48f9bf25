"""Seeded random allocation sweeps (the helper of tests/test_allocation_sweep_fuzz_gpu.py and its _cpu twin), in the manner
of tests/feature_fuzz.py: any 64-bit seed, path ids up to 2^62, sizes on both sides of a wave, a chunk and a Philox block,
joint tables of 2, 37, 2048 and 2049 rows or a random Gaussian law, K = 1 .. 4 assets, S = 1 .. 8 scenarios with random
weights (now and then one of exactly 0), R, amounts, fractions and floors, 0 to 100 buckets, the IEEE divide asked for in
a quarter of the cases.  A case carries its own inputs; reference() restates it with
tests/portfolio_cashflow_reference.py on the multipliers of tests/portfolio_reference.py.

Against a vacuous fuzz the amounts are sized from the case's own paths: around the constant amount that exhausts the
median path of scenario 0's allocation at the end of the run.  tests/test_allocation_sweep_fuzz_cpu.py asserts, on the
restatement alone, that at most a quarter of the cases have every path depleted in every scenario or none in any."""
import numpy as np

import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

f32 = np.float32
FIRST = [0, 1, 255, (1 << 32) - 300, (1 << 32), (1 << 45) + 12345, (1 << 62) - 7000]
PATHS = [1, 63, 64, 65, 255, 256, 257, 1000, 2047, 4100]
PERIODS = [1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 100, 360]
ROWS = [2, 37, 2048, 2049]
BINS = [0, 7, 100]
SEED, COUNT = 18, 32  # the numpy seed of the draw and the number of cases: the reference work stays under about 30 s


def _weights(rng, K):
    w = rng.dirichlet(np.ones(K))
    if K > 1 and rng.integers(3) == 0:
        w[int(rng.integers(K))] = 0.0  # a weight of exactly 0
    w = (w / w.sum()).astype(f32)
    w[int(np.argmax(w))] += f32(1.0 - float(w.astype(np.float64).sum()))  # the sum within 1e-6 of 1
    return tuple(float(x) for x in w)


def multipliers(oracle, c):
    if c["mode"] == "table":
        return pref.table_multipliers(oracle, c["assets"], c["seed"], c["first"], c["n"], c["P"])
    return pref.gauss_multipliers(oracle, c["law"][0], c["law"][1], c["seed"], c["first"], c["n"], c["P"])


def reference(oracle, c):
    """One portfolio_cashflow_reference.simulate per scenario of the case."""
    a = multipliers(oracle, c)
    return [pcref.simulate(a, w, R, amount=am, fraction=fr, floor=fl, capital=c["capital"]) for w, R, am, fr, fl in c["scenarios"]]


def cases(oracle):
    rng = np.random.default_rng(SEED)
    for i in range(COUNT):
        K, S, P = int(rng.integers(1, 5)), int(rng.integers(1, 9)), int(rng.choice(PERIODS))
        cap = float(rng.choice([1000.0, 12345.678, 1.0]))
        c = dict(i=i, id=f"allocation_sweep#{i}", mode=("table", "gauss")[int(rng.integers(2))], K=K, S=S, P=P, capital=cap,
                 seed=int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2)), first=int(rng.choice(FIRST)),
                 n=int(rng.choice(PATHS, p=[0.05] + [0.95 / 9] * 9)) + int(rng.integers(0, 3)), exact=bool(rng.integers(4) == 0),
                 hist=(int(rng.choice(BINS)), 0.0, float(f32(cap * float(rng.choice([2.0, 20.0])))), float(f32(cap * float(rng.choice([0.9, 1.0, 1.5]))))))
        if c["mode"] == "table":
            c["assets"] = rng.normal(0.6, 4.3, (int(rng.choice(ROWS)), K)).astype(f32)
        else:  # random means and a random valid Cholesky factor: that of a random covariance matrix
            g = rng.normal(0.0, 1.0, (K, K + 2))
            sd = rng.choice([0.5, 2.0, 4.3], K)
            corr = g @ g.T
            corr /= np.sqrt(np.outer(np.diag(corr), np.diag(corr)))
            c["law"] = ([float(x) for x in rng.choice([0.0, 0.5, -0.25, 2.0], K)], np.linalg.cholesky(sd[:, None] * corr * sd[None, :]).astype(f32))
        weights = [_weights(rng, K) for _ in range(S)]
        head = multipliers(oracle, dict(c, n=min(c["n"], 256)))
        m = float(np.median(pcref.simulate(head, weights[0], 0, capital=cap)["final"])) / cap
        level = cap / P if abs(m - 1.0) < 1e-6 else cap * m * (m ** (1.0 / P) - 1.0) / (m - 1.0)
        am = level * (0.7 + 0.6 * rng.permutation(S) / max(S - 1, 1))
        if S > 2:
            am[rng.integers(S)] *= -0.1  # one scenario pays in
        floor = float(f32(cap * float(rng.choice([0.0, 1e-5, 0.05]))))
        c["scenarios"] = [(weights[s], int(rng.choice([0, 1, 5, 12, P, P + 1])), float(f32(am[s])), float(rng.choice([0.0, 0.002])),
                           float(f32(floor * (1 + s % 2)))) for s in range(S)]
        yield c


def vacuous(ref):
    """Every path depleted in every scenario, or none in any."""
    shares = [float((r["ruin_period"] > 0).mean()) for r in ref]
    return all(s == 0.0 for s in shares) or all(s == 1.0 for s in shares)
