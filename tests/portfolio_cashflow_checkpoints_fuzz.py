"""Seeded random requests of smmc_engine_simulate_portfolio_cashflow_checkpoints (the helper of
tests/test_portfolio_cashflow_checkpoints_gpu.py; tests/test_portfolio_cashflow_checkpoints_cpu.py checks the generator
alone).  A case is a portfolio cash-flow case of tests/feature_fuzz.py -- drawn with its own pieces, nothing there is
edited: any 64-bit seed, path ids up to 2^62, sizes on both sides of a wave, a chunk and a Philox block, K = 1 .. 4 with
now and then a weight of exactly 0, R in 0, 1, 5, 12, P and P + 1, a constant or a per-period schedule sized so that
about half of the case's paths are depleted, 0 to 1000 buckets, the IEEE divide asked for in a quarter of the cases --
with a random checkpoint set: 1 to min(P, 64, 8192 / n_bins) distinct periods (SMMC_MAX_CHECKPOINTS,
SMMC_MAX_CHECKPOINT_BINS), sorted.  reference() restates a case with tests/portfolio_cashflow_reference.py, columns
included."""
import numpy as np

import feature_fuzz as F
import feature_matrix as M
import portfolio_cashflow_reference as pcref

PARENT = "portfolio_cashflow_kernel"
SEED, COUNT = 19, 24  # the numpy seed of the draw and the number of cases: the reference work stays under about 30 s


def cases(oracle):
    rng = np.random.default_rng(SEED)
    for i in range(COUNT):
        c = F._common(rng, PARENT, i)
        c["id"] = f"portfolio_cashflow_checkpoints#{i}"
        F._portfolio(rng, c)
        c["schedule"] = F._sized(oracle, c, F._flows(rng, oracle, c))
        P = c["P"]
        k = int(rng.integers(1, min(P, 64, 8192 // max(c["hist"][0], 1)) + 1))
        c["periods"] = tuple(sorted(int(x) for x in rng.choice(np.arange(1, P + 1), size=k, replace=False)))
        yield c


def reference(oracle, c):
    """portfolio_cashflow_reference.simulate's dict of the case with `values` [n, P + 1]."""
    return pcref.simulate(M.portfolio_multipliers(oracle, c), M.weights(c), M.rebalance(c), capital=c["capital"], columns=True,
                          **c["schedule"])


def vacuous(ref):
    """Every path depleted, or none."""
    share = float((ref["ruin_period"] > 0).mean())
    return share == 0.0 or share == 1.0
