"""Seeded random cases of smmc_engine_simulate_real_cashflow (the helper of tests/test_real_cashflow_fuzz_cpu.py and
tests/test_real_cashflow_fuzz_gpu.py, as tests/feature_fuzz.py is of its families): any 64-bit seed, path ids up to 2^62,
sizes on both sides of a wave, a chunk and a Philox block, capitals from 1e-3 to 1e9, K = 1 .. 3 with a weight of exactly 0
now and then, any R, joint tables of 1, 2, 37, 2048 and 2049 rows whose last column is an inflation series of its own
mean and spread (0 % and deflation included), random Gaussian laws of K + 1 series, 0 to 1000 buckets, the IEEE divide
asked for in a quarter of the cases, constant and per-period schedules with contributions among the withdrawals.  A case
is a dict in the form of tests/real_cashflow_matrix.py's, carrying its own inputs, so that its reference() restates it.

Against a vacuous fuzz the amounts are sized from the case's own paths: near the real amount that exhausts the median path
at the end of the run, then scaled by bisection on the restatement until about half of the first 256 paths are depleted
(tests/feature_fuzz.py: _sized).  tests/test_real_cashflow_fuzz_cpu.py asserts that at most a quarter of the cases have
every or no path depleted."""
import numpy as np

import feature_fuzz as F
import feature_matrix as M
import real_cashflow_matrix as RM
import real_cashflow_reference as ref

f32 = np.float32
SEED, COUNT = 18, 40
PERIODS = [1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 100, 360, 361]


def _sized(oracle, c, sched):
    head = dict(c, n=min(c["n"], 256))
    lo, hi = 0.02, 50.0
    for _ in range(8):
        mid = float(np.sqrt(lo * hi))
        share = float((RM.reference(oracle, dict(head, schedule=F._scaled(sched, mid)))["ruin_period"] > 0).mean())
        if share < 0.5:
            lo = mid
        else:
            hi = mid
    return F._scaled(sched, float(np.sqrt(lo * hi)))


def draw():
    """The COUNT cases as the module's fixed numpy seed draws them, without the schedule: everything here is cheap, so a
    test can take case i alone and finish() it."""
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(COUNT):
        mode = ("table", "gauss")[int(rng.integers(2))]
        cap = float(rng.choice(F.CAPITALS))
        n_bins = int(rng.choice(F.BINS))
        K = int(rng.integers(1, 4))
        P = int(rng.choice(PERIODS))
        c = dict(family=RM.FAMILY, i=i, mode=mode, T=int(rng.choice(F.ROWS, p=[0.1, 0.15, 0.25, 0.25, 0.25])), K=K, extreme=False, kind=None,
                 exact="flag" if rng.integers(4) == 0 else None, capital=cap, id=f"real_cashflow#{i}",
                 seed=int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2)), first=int(rng.choice(F.FIRST)),
                 n=int(rng.choice(F.PATHS, p=[0.05] + [0.95 / 9] * 9)) + int(rng.integers(0, 3)), P=P,
                 hist=(n_bins, 0.0, float(f32(cap * float(rng.choice([2.0, 20.0])))), float(f32(cap * float(rng.choice([0.9, 1.0, 1.5]))))))
        w = rng.dirichlet(np.ones(K))
        if K > 1 and rng.integers(3) == 0:
            w[int(rng.integers(K))] = 0.0  # a weight of exactly 0
        w = (w / w.sum()).astype(f32)
        w[int(np.argmax(w))] += f32(1.0 - float(w.astype(np.float64).sum()))  # the sum within 1e-6 of 1
        c["weights"] = tuple(float(x) for x in w)
        c["R"] = int(rng.choice([0, 1, 5, 12, P, P + 1]))
        inflation = (float(rng.choice([0.0, 0.25, 1.0, -0.2])), float(rng.choice([0.0, 0.1, 0.4])))
        if mode == "table":
            t = rng.normal(0.6, 4.3, (c["T"], K + 1))
            t[:, K] = inflation[0] + inflation[1] * (0.5 * t[:, 0] / 4.3 + rng.normal(0.0, 1.0, c["T"]))  # correlated with asset 0
            c["assets"] = t.astype(f32)
        else:  # random means and the Cholesky factor of a random covariance matrix; the last series is inflation
            g = rng.normal(0.0, 1.0, (K + 1, K + 3))
            sd = np.append(rng.choice([0.5, 2.0, 4.3], K), inflation[1])
            corr = g @ g.T
            corr /= np.sqrt(np.outer(np.diag(corr), np.diag(corr)))
            means = [float(x) for x in rng.choice([0.0, 0.5, -0.25, 2.0], K)] + [inflation[0]]
            factor = np.linalg.cholesky(sd[:, None] * corr * sd[None, :] + np.diag([0.0] * K + [1e-30])).astype(f32)
            c["pf"] = (means, factor)
        c["varying"] = bool(rng.integers(2))
        # the schedule's shape, relative to the level that finish() works out from the case's own paths
        shape = dict(level=float(rng.uniform(0.8, 1.25)), floor=float(f32(cap * float(rng.choice([0.0, 1e-5, 0.05])))))
        if not c["varying"]:
            shape["fraction"] = float(rng.choice([0.0, 0.0, 0.003]))
        else:
            am = rng.uniform(0.3, 1.8, P)
            am[rng.random(P) < 0.2] *= -0.5  # contributions among the withdrawals
            shape["amounts"], shape["fractions"] = am, rng.choice([0.0, 0.002, 0.01], P).astype(f32)
        c["shape"] = shape
        out.append(c)
    return out


def finish(oracle, c):
    """The case with its schedule: the drawn shape at the real amount that exhausts the median path at the end of the run,
    then sized so that about half of the first 256 paths are depleted."""
    c, shape = dict(c), c["shape"]
    P, cap = c["P"], c["capital"]
    with np.errstate(all="ignore"):
        m = float(np.nanmedian(ref.simulate(RM.multipliers(oracle, dict(c, n=min(c["n"], 256))), c["weights"], 0, capital=cap)["final_real"]
                               .astype(np.float64))) / cap
    level = M._level(m if np.isfinite(m) and m > 0 else 1.0, P, cap) * shape["level"]
    if not c["varying"]:
        sched = dict(amount=float(f32(level)), fraction=shape["fraction"], floor=shape["floor"])
    else:
        sched = dict(amounts=(level * shape["amounts"]).astype(f32), fractions=shape["fractions"], floor=shape["floor"])
    c["schedule"] = _sized(oracle, c, sched)
    del c["shape"]
    return c


def cases(oracle):
    """The COUNT finished cases."""
    for c in draw():
        yield finish(oracle, c)


def vacuous(want):
    share = float((want["ruin_period"] > 0).mean())
    return share == 0.0 or share == 1.0


brief = F.brief
