"""Seeded random cases of the seven feature entry points (the helper of tests/test_feature_fuzz_gpu.py, as _cases is of
tests/test_fuzz_gpu.py): any 64-bit seed, path ids up to 2^62, sizes on both sides of a wave, a chunk and a Philox block,
capitals from 1e-3 to 1e9, Gaussian laws with std 0, tables of 1, 2, 37, 2048 and 2049 rows, 0 to 1000 buckets, the IEEE
divide asked for in a quarter of the cases, and each feature's own arguments.  A case is a dict in the form of
tests/feature_matrix.py's, carrying its own inputs, so that feature_matrix.reference() restates it.

Arguments the header refuses are not drawn: P = 0 is refused by checkpoints (a checkpoint lies in 1 .. P), cash flows,
sweeps, excursions and portfolio cash flows, and drawn for blocks and portfolios; a checkpoint set holds at most
8192 / n_bins periods (SMMC_MAX_CHECKPOINT_BINS), a sweep at most 8192 counters (SMMC_MAX_SWEEP_COUNTERS).

Against a vacuous fuzz the schedules and levels are sized from the case's own paths: a constant amount near the one that
exhausts the median path at the end of the run (feature_matrix._level), levels at the 30th percentile of the paths' lows
and the 70th of their peaks.  tests/test_feature_fuzz_cpu.py asserts, on the restatement alone, that at most a quarter of
a function's cases have every or no path depleted (no path ever below, none reaching)."""
import numpy as np

import feature_matrix as M

f32 = np.float32
FIRST = [0, 1, 255, (1 << 32) - 300, (1 << 32), (1 << 45) + 12345, (1 << 62) - 7000]
PATHS = [1, 63, 64, 65, 255, 256, 257, 1000, 2047, 4100]
PERIODS = [1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 100, 360, 361, 500]
CAPITALS = [1.0, 1000.0, 12345.678, 1e-3, 1e9]
ROWS = [1, 2, 37, 2048, 2049]
BINS = [0, 1, 7, 100, 1000]
# (numpy seed, cases) of each test function; the counts keep a function's reference work under about 30 s
PLAN = {"checkpoints_kernel": (11, 40), "cashflow_kernel": (12, 40), "cashflow_sweep_kernel": (13, 30), "excursions_kernel": (14, 40),
        "blocks_kernel": (15, 40), "portfolio_kernel": (16, 30), "portfolio_cashflow_kernel": (17, 30)}
P_ZERO = ("blocks_kernel", "portfolio_kernel")  # the entry points that accept n_periods = 0


def _common(rng, family, i):
    mode = "table" if family == "blocks_kernel" else ("table", "gauss")[int(rng.integers(2))]
    periods = ([0] if family in P_ZERO else []) + PERIODS
    cap = float(rng.choice(CAPITALS))
    n_bins = int(rng.choice(BINS))
    exact = bool(rng.integers(4) == 0)
    c = dict(family=family, i=i, mode=mode, T=int(rng.choice(ROWS, p=[0.1, 0.15, 0.25, 0.25, 0.25])), K=1, S=1, L=1, varying=False, extreme=False, kind=None,
             exact="flag" if exact else None, read=None, capital=cap, id=f"{family}#{i}",
             seed=int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2)), first=int(rng.choice(FIRST)),
             n=int(rng.choice(PATHS, p=[0.05] + [0.95 / 9] * 9)) + int(rng.integers(0, 3)), P=int(rng.choice(periods)),
             law=(float(rng.choice([0.0, 0.5, -0.25, 2.0])), float(rng.choice([0.0, 0.83333, 4.3, 1e-3], p=[0.125, 0.25, 0.5, 0.125]))),
             hist=(n_bins, 0.0, float(f32(cap * float(rng.choice([2.0, 20.0])))), float(f32(cap * float(rng.choice([0.9, 1.0, 1.5]))))))
    if mode == "table":
        c["table"] = rng.normal(0.6, 4.3, c["T"]).astype(f32)
    return c


def _portfolio(rng, c):
    K = c["K"] = int(rng.integers(1, 5))
    w = rng.dirichlet(np.ones(K))
    if K > 1 and rng.integers(3) == 0:
        w[int(rng.integers(K))] = 0.0  # a weight of exactly 0
    w = (w / w.sum()).astype(f32)
    w[int(np.argmax(w))] += f32(1.0 - float(w.astype(np.float64).sum()))  # the sum within 1e-6 of 1
    c["weights"] = tuple(float(x) for x in w)
    c["R"] = int(rng.choice([0, 1, 5, 12, max(c["P"], 1), c["P"] + 1]))
    if c["mode"] == "table":
        c["assets"] = rng.normal(0.6, 4.3, (c["T"], K)).astype(f32)
    else:  # random means and a random valid Cholesky factor: that of a random covariance matrix
        g = rng.normal(0.0, 1.0, (K, K + 2))
        sd = rng.choice([0.5, 2.0, 4.3], K)
        corr = g @ g.T
        corr /= np.sqrt(np.outer(np.diag(corr), np.diag(corr)))
        c["pf"] = ([float(x) for x in rng.choice([0.0, 0.5, -0.25, 2.0], K)],
                   np.linalg.cholesky(sd[:, None] * corr * sd[None, :]).astype(f32))
    return c


def _scaled(sched, x):
    if isinstance(sched, list):
        return [(float(f32(a * x)), fr, fl) for a, fr, fl in sched]
    return {k: ((v * f32(x)).astype(f32) if k == "amounts" else float(f32(v * x)) if k == "amount" else v) for k, v in sched.items()}


def _sized(oracle, c, sched):
    """The schedule with its amounts scaled so that about half of the case's first 256 paths are depleted: eight
    bisection steps on the restatement (the degenerate cases -- one path, std 0, one table row -- stay all or none)."""
    head = dict(c, n=min(c["n"], 256))
    lo, hi = 0.02, 50.0
    for _ in range(8):
        mid = float(np.sqrt(lo * hi))
        share = M.depleted_share(M.reference(oracle, dict(head, schedule=_scaled(sched, mid))))
        if float(np.median(share)) < 0.5:
            lo = mid
        else:
            hi = mid
    return _scaled(sched, float(np.sqrt(lo * hi)))


def _flows(rng, oracle, c):
    """The schedule of a cash-flow case, sized from its own capital and median growth (the module's docstring)."""
    P, cap = c["P"], c["capital"]
    level = M._level(M.median_growth(oracle, c), P, cap) * float(rng.uniform(0.8, 1.25))
    floor = float(f32(cap * float(rng.choice([0.0, 1e-5, 0.05]))))
    if c["family"] == "cashflow_sweep_kernel":
        S = c["S"] = int(rng.integers(1, 9))
        am = level * (0.9 + 0.2 * rng.permutation(S) / max(S - 1, 1))
        if S > 2:
            am[rng.integers(S)] *= -0.1  # one scenario pays in
        return [(float(f32(am[s])), float(rng.choice([0.0, 0.002])), float(f32(floor * (1 + s % 2)))) for s in range(S)]
    c["varying"] = bool(rng.integers(2))
    if not c["varying"]:
        return dict(amount=float(f32(level)), fraction=float(rng.choice([0.0, 0.0, 0.003])), floor=floor)
    am = level * rng.uniform(0.3, 1.8, P)
    am[rng.random(P) < 0.2] *= -0.5  # contributions among the withdrawals
    return dict(amounts=am.astype(f32), fractions=rng.choice([0.0, 0.002, 0.01], P).astype(f32), floor=floor)


def cases(oracle, family):
    """The cases of a family's test function, drawn from its fixed numpy seed."""
    seed, count = PLAN[family]
    rng = np.random.default_rng(seed)
    for i in range(count):
        c = _common(rng, family, i)
        P = c["P"]
        if family == "checkpoints_kernel":
            k = int(rng.integers(1, min(P, 64, 8192 // max(c["hist"][0], 1)) + 1))
            c["periods"] = sorted(int(x) for x in rng.choice(np.arange(1, P + 1), size=k, replace=False))
        elif family == "excursions_kernel":
            traj = M.trajectories(oracle, c)
            with np.errstate(all="ignore"):
                c["levels"] = (float(np.percentile(traj.min(axis=1), 30.0).astype(f32)), float(np.percentile(traj.max(axis=1), 70.0).astype(f32)))
        elif family == "blocks_kernel":
            c["L"] = int(rng.choice([1, 2, 3, 12, max(P, 1), P + 1, c["T"], c["T"] + 1]))
        elif family in ("portfolio_kernel", "portfolio_cashflow_kernel"):
            _portfolio(rng, c)
        if family == "cashflow_sweep_kernel" and c["hist"][0] == 1000:  # 8 * (P + 1 + 1000) may pass the counter budget
            c["hist"] = (100,) + c["hist"][1:]
        if family in ("cashflow_kernel", "cashflow_sweep_kernel", "portfolio_cashflow_kernel"):
            c["schedule"] = _sized(oracle, c, _flows(rng, oracle, c))
        yield c


def vacuous(ref):
    """Whether a cash-flow reference has every path or no path depleted; a sweep: every path in every scenario, or none
    in any (scenarios that part ways -- all depleted in one, none in its neighbour -- tell a kernel's scenarios apart)."""
    share = M.depleted_share(ref)
    share = share if isinstance(share, list) else [share]
    return all(s == 0.0 for s in share) or all(s == 1.0 for s in share)


def brief(c):
    return {k: (v if not isinstance(v, np.ndarray) else v.shape) for k, v in c.items() if k not in ("table", "assets", "pf")}
