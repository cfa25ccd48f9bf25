"""ctypes binding of the C ABI in include/smmc.h (libsmmc_hip.so).

There is no fallback: if the HIP library is missing or fails to load, importing the
engine raises.  Nothing here touches oracle/.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libsmmc_hip.so")
# Development only: tools/variant_build.sh writes experimental builds under _build/ (never over the
# product library) and the A/B tools point this at them.
if os.environ.get("SMMC_LIB"):
    import sys as _sys
    LIB_PATH = os.path.abspath(os.environ["SMMC_LIB"])
    print(f"stock_market_monte_carlo_amd: DEVELOPMENT library {LIB_PATH} (SMMC_LIB)", file=_sys.stderr)

ABI_VERSION = 4
MODE_TABLE = 0
MODE_GAUSSIAN = 1
FLAG_EXACT_DIV = 1
FLAG_STREAM_V2 = 2  # counter stream v2 (round 1's) instead of v3
FLAG_QUIET = 8
FLAG_HOST_NOPIN = 16  # simulate_to_host: never page-lock host_final for the call
FLAG_STREAM_REF = 4  # the reference CPU engine's own stream: per-path mt19937 + libstdc++ Lemire map (table mode)
CHUNK = 256
MAX_TABLE = 16384
MAX_BINS = 4096
MAX_RANKS = 8
MAX_CHECKPOINTS = 64
MAX_CHECKPOINT_BINS = 8192  # largest n_checkpoints * n_bins of one simulate_checkpoints call
MAX_CASHFLOW_PERIODS = 4096  # largest n_periods of a simulate_cashflow call
MAX_SWEEP = 8  # most scenarios of a simulate_cashflow_sweep or simulate_allocation_sweep call
MAX_SWEEP_COUNTERS = 8192  # largest n_scenarios * (n_periods + 1 + n_bins) of one
MAX_EXCURSION_PERIODS = 4096  # largest n_periods of a simulate_excursions call
MAX_ASSETS = 4  # most assets of a simulate_portfolio call
MAX_GLIDE_CHANGES = 512  # most changes of target weights of a simulate_glide call


class Sim(C.Structure):
    """smmc_sim"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mode", C.c_int32),
        ("seed", C.c_uint64),
        ("first_path", C.c_uint64),
        ("n_paths", C.c_uint64),
        ("n_periods", C.c_uint32),
        ("initial_capital", C.c_float),
        ("gauss_mean", C.c_float),
        ("gauss_std", C.c_float),
        ("n_bins", C.c_uint32),
        ("hist_lo", C.c_float),
        ("hist_hi", C.c_float),
        ("below_threshold", C.c_float),
        ("flags", C.c_uint32),
    ]


class Stats(C.Structure):
    """smmc_stats (header of the packed record; n_bins uint64 counts follow)"""
    _fields_ = [
        ("count", C.c_uint64),
        ("below", C.c_uint64),
        ("underflow", C.c_uint64),
        ("overflow", C.c_uint64),
        ("sum", C.c_double),
        ("sumsq", C.c_double),
        ("min", C.c_float),
        ("max", C.c_float),
        ("n_bins", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class Cashflow(C.Structure):
    """smmc_cashflow"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("amount", C.c_float),
        ("fraction", C.c_float),
        ("amounts", C.c_void_p),
        ("fractions", C.c_void_p),
        ("floor", C.c_float),
    ]


class Excursions(C.Structure):
    """smmc_excursions"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("lower", C.c_float),
        ("target", C.c_float),
        ("drawdown_threshold", C.c_float),
    ]


class Blocks(C.Structure):
    """smmc_blocks"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("block_len", C.c_uint32),
        ("kind", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


BLOCKS_CIRCULAR = 0


class Stationary(C.Structure):
    """smmc_stationary"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("renew_q16", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


RENEW_Q16_ONE = 65536


class Regimes(C.Structure):
    """smmc_regimes"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("mean", C.c_float * 2),
        ("std", C.c_float * 2),
        ("leave_q16", C.c_uint32 * 2),
        ("start1_q16", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


REGIME_Q16_ONE = 65536


class PortfolioRegimes(C.Structure):
    """smmc_portfolio_regimes"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("leave_q16", C.c_uint32 * 2),
        ("start1_q16", C.c_uint32),
        ("means", (C.c_float * 4) * 2),
        ("factor", (C.c_float * 16) * 2),
        ("reserved", C.c_uint32 * 2),
    ]


class Portfolio(C.Structure):
    """smmc_portfolio"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_assets", C.c_uint32),
        ("rebalance_every", C.c_uint32),
        ("reserved", C.c_uint32),
        ("weights", C.c_float * MAX_ASSETS),
        ("means", C.c_float * MAX_ASSETS),
        ("factor", C.c_float * (MAX_ASSETS * MAX_ASSETS)),
    ]


class PortfolioOutputs(C.Structure):
    """smmc_portfolio_outputs"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("final", C.c_void_p),
        ("holdings", C.c_void_p),
        ("stats", C.c_void_p),
    ]


class PortfolioCashflowOutputs(C.Structure):
    """smmc_portfolio_cashflow_outputs"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("final", C.c_void_p),
        ("holdings", C.c_void_p),
        ("paid", C.c_void_p),
        ("ruin_period", C.c_void_p),
        ("stats", C.c_void_p),
        ("depleted_at", C.c_void_p),
    ]


class RealCashflowOutputs(C.Structure):
    """smmc_real_cashflow_outputs"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("final", C.c_void_p),
        ("final_real", C.c_void_p),
        ("index", C.c_void_p),
        ("holdings", C.c_void_p),
        ("paid", C.c_void_p),
        ("ruin_period", C.c_void_p),
        ("stats", C.c_void_p),
        ("depleted_at", C.c_void_p),
    ]


class Glide(C.Structure):
    """smmc_glide"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_changes", C.c_uint32),
        ("after", C.POINTER(C.c_uint32)),
        ("weights", C.POINTER(C.c_float)),
    ]


class Guardrails(C.Structure):
    """smmc_guardrails"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("review_every", C.c_uint32),
        ("amount", C.c_float),
        ("index", C.c_float),
        ("upper", C.c_float),
        ("lower", C.c_float),
        ("cut", C.c_float),
        ("raise_", C.c_float),
        ("amount_min", C.c_float),
        ("amount_max", C.c_float),
        ("floor", C.c_float),
    ]


# the pointer fields of smmc_guardrails_outputs, in the order of the structure
GUARDRAILS_OUTPUTS = ("final", "holdings", "paid", "ruin_period", "stats", "depleted_at", "amount_last", "amount_lowest",
                      "cuts", "raises", "cuts_at", "raises_at")


class GuardrailsOutputs(C.Structure):
    """smmc_guardrails_outputs"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(name, C.c_void_p) for name in GUARDRAILS_OUTPUTS]


class AllocationSweepOutputs(C.Structure):
    """smmc_allocation_sweep_outputs"""
    _fields_ = PortfolioCashflowOutputs._fields_  # the same pointers, scenario-major


# the pointer fields of smmc_excursion_outputs, in the order of the structure
EXCURSION_OUTPUTS = ("final", "peak", "low", "drawdown", "drawdown_period", "underwater", "first_below", "first_reach",
                     "stats", "drawdown_stats", "first_below_at", "first_reach_at")


class ExcursionOutputs(C.Structure):
    """smmc_excursion_outputs"""
    _fields_ = [("struct_size", C.c_uint32)] + [(name, C.c_void_p) for name in EXCURSION_OUTPUTS]


# every symbol include/smmc.h declares: (name, restype, argtypes)
DIV_FAST, DIV_EXACT, DIV_CHECKED = 0, 1, 2  # smmc_engine_divide_kind
MERGE_HOST, MERGE_RCCL = 0, 1  # smmc_group_create

SYMBOLS = [
    ("smmc_update_fund", C.c_float, [C.c_float, C.c_float]),
    ("smmc_many_updates", None, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("smmc_abi_version", C.c_int, []),
    ("smmc_build_digest", C.c_char_p, []),
    ("smmc_vector_add", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]),
    ("smmc_last_error", C.c_char_p, []),
    ("smmc_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("smmc_engine_create", C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("smmc_engine_destroy", None, [C.c_void_p]),
    ("smmc_engine_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("smmc_engine_get_stream", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("smmc_engine_wait_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("smmc_engine_release_to_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("smmc_engine_set_progress", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_set_table", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("smmc_engine_simulate", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_keepdata", C.c_int, [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_void_p]),
    ("smmc_engine_sync", C.c_int, [C.c_void_p]),
    ("smmc_engine_simulate_checkpoints", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_checkpoints_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_cashflow", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Cashflow), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_cashflow_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Cashflow), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_cashflow_divide_kind", C.c_int, [C.c_void_p, C.POINTER(Sim), C.POINTER(Cashflow)]),
    ("smmc_engine_simulate_cashflow_sweep", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Cashflow), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_cashflow_sweep_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Cashflow), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_cashflow_sweep_divide_kind", C.c_int, [C.c_void_p, C.POINTER(Sim), C.POINTER(Cashflow), C.c_uint32]),
    ("smmc_engine_simulate_excursions", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Excursions), C.POINTER(ExcursionOutputs)]),
    ("smmc_engine_simulate_excursions_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Excursions), C.POINTER(ExcursionOutputs)]),
    ("smmc_engine_simulate_blocks", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Blocks), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_blocks_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Blocks), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats),
      C.c_void_p]),
    ("smmc_engine_blocks_divide_kind", C.c_int, [C.c_void_p, C.POINTER(Sim), C.POINTER(Blocks)]),
    ("smmc_engine_simulate_stationary", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Stationary), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_stationary_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Stationary), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats),
      C.c_void_p]),
    ("smmc_engine_stationary_divide_kind", C.c_int, [C.c_void_p, C.POINTER(Sim), C.POINTER(Stationary)]),
    ("smmc_engine_simulate_regimes", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Regimes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_engine_simulate_regimes_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Regimes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats),
      C.c_void_p]),
    ("smmc_engine_regimes_divide_kind", C.c_int, [C.c_void_p, C.POINTER(Sim), C.POINTER(Regimes)]),
    ("smmc_engine_set_asset_table", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("smmc_engine_simulate_portfolio", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(PortfolioOutputs)]),
    ("smmc_engine_simulate_portfolio_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(PortfolioOutputs)]),
    ("smmc_engine_portfolio_divide_kind", C.c_int, [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio)]),
    ("smmc_engine_simulate_portfolio_cashflow", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_simulate_portfolio_cashflow_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_portfolio_cashflow_divide_kind", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow)]),
    ("smmc_engine_simulate_portfolio_cashflow_blocks", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Blocks), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_simulate_portfolio_cashflow_blocks_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Blocks), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_portfolio_cashflow_blocks_divide_kind", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Blocks)]),
    ("smmc_engine_simulate_portfolio_cashflow_stationary", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Stationary), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_simulate_portfolio_cashflow_stationary_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Stationary), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_portfolio_cashflow_stationary_divide_kind", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Stationary)]),
    ("smmc_engine_simulate_portfolio_cashflow_regimes", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(PortfolioRegimes), C.POINTER(Cashflow), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_simulate_portfolio_cashflow_regimes_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(PortfolioRegimes), C.POINTER(Cashflow), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_portfolio_cashflow_regimes_divide_kind", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(PortfolioRegimes), C.POINTER(Cashflow)]),
    ("smmc_engine_simulate_portfolio_cashflow_checkpoints", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.c_void_p, C.c_uint32,
      C.POINTER(PortfolioCashflowOutputs), C.c_void_p]),
    ("smmc_engine_simulate_portfolio_cashflow_checkpoints_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.c_void_p, C.c_uint32,
      C.POINTER(PortfolioCashflowOutputs), C.c_void_p]),
    ("smmc_engine_simulate_allocation_sweep", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.c_uint32, C.POINTER(AllocationSweepOutputs)]),
    ("smmc_engine_simulate_allocation_sweep_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.c_uint32, C.POINTER(AllocationSweepOutputs)]),
    ("smmc_engine_allocation_sweep_divide_kind", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.c_uint32]),
    ("smmc_engine_simulate_real_cashflow", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(RealCashflowOutputs)]),
    ("smmc_engine_simulate_real_cashflow_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(RealCashflowOutputs)]),
    ("smmc_engine_real_cashflow_divide_kind", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow)]),
    ("smmc_engine_simulate_guardrails", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Guardrails), C.POINTER(GuardrailsOutputs)]),
    ("smmc_engine_simulate_guardrails_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Guardrails), C.POINTER(GuardrailsOutputs)]),
    ("smmc_engine_simulate_glide", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Glide), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_simulate_glide_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Glide), C.POINTER(PortfolioCashflowOutputs)]),
    ("smmc_engine_glide_divide_kind", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.POINTER(Portfolio), C.POINTER(Cashflow), C.POINTER(Glide)]),
    ("smmc_engine_simulate_to_host", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats), C.c_void_p]),
    ("smmc_engine_prepare_host", C.c_int, [C.c_void_p, C.c_uint64]),
    ("smmc_host_register", C.c_int, [C.c_void_p, C.c_uint64]),
    ("smmc_host_unregister", C.c_int, [C.c_void_p]),
    ("smmc_group_prepare_host", C.c_int, [C.c_void_p, C.c_uint64]),
    ("smmc_engine_simulate_keepdata_to_host", C.c_int, [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_void_p]),
    ("smmc_engine_values_stats", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_uint32, C.c_float, C.c_float, C.c_void_p]),
    ("smmc_engine_order_statistics", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("smmc_engine_quartiles", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("smmc_engine_reduce_mean_host", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    ("smmc_engine_host_values_summary", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.c_uint32, C.c_float, C.c_float, C.POINTER(Stats),
      C.c_void_p, C.c_void_p]),
    ("smmc_engine_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("smmc_engine_kernel_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    ("smmc_engine_kernel_clock", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("smmc_engine_selftest", C.c_int,
     [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("smmc_engine_selftest_draws", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("smmc_engine_geometry", C.c_int,
     [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("smmc_engine_divide_kind", C.c_int, [C.c_void_p, C.POINTER(Sim), C.c_int]),
    ("smmc_engine_paths_form", C.c_int, [C.c_void_p, C.POINTER(Sim)]),
    ("smmc_set_uniform_hi", C.c_int, [C.c_int]),
    ("smmc_group_create", C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("smmc_group_destroy", None, [C.c_void_p]),
    ("smmc_group_size", C.c_int, [C.c_void_p]),
    ("smmc_group_set_table", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("smmc_group_set_progress", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("smmc_group_simulate", C.c_int,
     [C.c_void_p, C.POINTER(Sim), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats), C.c_void_p]),
    ("smmc_group_shard", C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("smmc_group_device_record", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("smmc_group_timings", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("smmc_stats_bytes", C.c_uint64, [C.c_uint32]),
    ("smmc_stats_merge", C.c_int, [C.c_void_p, C.c_void_p]),
]

_lib = None


class SmmcError(RuntimeError):
    pass


def lib():
    """Loads libsmmc_hip.so once.  Raises if it is missing: there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SmmcError(
                f"{LIB_PATH} is missing: build it with `python -m stock_market_monte_carlo_amd.build` "
                "(hipcc, gfx950).  This package has no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm wheels carry their own libamdhip64
        # (soname libamdhip64.so.7, the one our library asks for).  Loading torch first
        # makes the dynamic linker hand that copy to libsmmc_hip.so, so streams and
        # device pointers can cross between the two; the other order would map a
        # second runtime (/opt/rocm) that cannot see the device.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if L.smmc_abi_version() != ABI_VERSION:
            raise SmmcError(f"libsmmc_hip.so has ABI {L.smmc_abi_version()}, binding expects {ABI_VERSION}")
        _check_digest(L)
        _lib = L
    return _lib


def build_digest():
    """The digest the loaded library carries (smmc_build_digest)."""
    return lib().smmc_build_digest().decode()


def _check_digest(L):
    """The library must have been built from the sources that lie beside it: its embedded digest (flags + content
    of every source and header, build.source_digest()) against the tree's.  A stale product library is an error;
    a development library (SMMC_LIB) only a loud warning.  Without the sources (a copied .so) there is nothing
    to compare with and nothing is claimed."""
    import sys
    from . import build
    if not os.path.isdir(build.CSRC):
        return
    have, want = L.smmc_build_digest().decode(), build.source_digest()
    if have == want:
        return
    msg = (f"{LIB_PATH} was built from other sources or flags than this tree holds (library {have[:16]}..., sources "
           f"{want[:16]}...): rebuild it with `python -m stock_market_monte_carlo_amd.build`")
    if os.environ.get("SMMC_LIB"):
        print(f"stock_market_monte_carlo_amd: WARNING: {msg}", file=sys.stderr)
        return
    raise SmmcError("stale library: " + msg)


def check(rc):
    if rc != 0:
        raise SmmcError(f"smmc error {rc}: {lib().smmc_last_error().decode(errors='replace')}")
