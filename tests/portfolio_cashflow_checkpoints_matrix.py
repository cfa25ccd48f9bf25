"""The ledger of portfolio_cashflow_checkpoints_kernel's instantiations, in the manner of tests/real_cashflow_matrix.py
(it uses the helpers of tests/feature_matrix.py and edits nothing there): one row per compiled combination of <kMode,
kExactDiv, kDense, K, kVarying> -- three rungs of the mode ladder, two divides, K = 1 .. 4, constant or per-period
schedule: 48 -- with ONE request each that makes the host choose it through
smmc_engine_simulate_portfolio_cashflow_checkpoints.  tests/test_portfolio_cashflow_checkpoints_cpu.py compares ROWS with
the compiled symbol names; tests/test_portfolio_cashflow_checkpoints_gpu.py runs every row against reference().

The new family is chosen by the rule that chooses portfolio_cashflow_kernel (mode, table length, divide kind, K,
schedule form), so a row is the parent's row of tests/feature_matrix.py -- its shapes (64 kW 2 + 37 paths, 9 periods for
dense tables and 5 otherwise, tables of 2048 and 2049 rows), laws, weights, R = 2 and schedule -- under the new family's
name, with feature_matrix.checkpoints_of() as its periods: (1, 4, 8, 9) or (1, 4, 5), the first period, a block boundary
of either draw width and the last period."""
import feature_matrix as M
import portfolio_cashflow_reference as pcref

FAMILY = "portfolio_cashflow_checkpoints_kernel"
PARENT = "portfolio_cashflow_kernel"
SIGNATURE = M.SIGNATURES[PARENT]
DIV_FAST, DIV_EXACT = M.DIV_FAST, M.DIV_EXACT


def mangled(args):
    """The template-argument list of an instantiation as it appears in the kernel's symbol."""
    return "I" + "".join(f"L{t}{int(v)}E" for t, v in zip(SIGNATURE, args)) + "E"


def _row(parent):
    c = dict(parent)  # family stays the parent's: feature_matrix's helpers choose the portfolio's inputs by it
    c["id"] = "portfolio_cashflow_checkpoints" + mangled(c["args"]) + ("-extreme" if c["extreme"] else "")
    c["periods"] = tuple(M.checkpoints_of(parent))
    return c


ROWS = [_row(c) for c in M.rows_of(PARENT, M.ROWS)]
EXTREME = [_row(c) for c in M.rows_of(PARENT, M.EXTREME)]
CASES = ROWS + EXTREME


def reference(oracle, c):
    """portfolio_cashflow_reference.simulate's dict with `values` [n, P + 1] (column p: the paths' values after period p)
    and `args`: (R, the schedule's keyword arguments)."""
    sched = M.schedule(c, None if "schedule" in c else M.median_growth(oracle, c))
    R = M.rebalance(c)
    out = pcref.simulate(M.portfolio_multipliers(oracle, c), M.weights(c), R, capital=c["capital"], columns=True, **sched)
    out["args"] = (R, sched)
    return out
