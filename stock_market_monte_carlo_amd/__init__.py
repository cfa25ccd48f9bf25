"""MI355X-native Monte-Carlo returns engine: a drop-in for the Monte-Carlo path of
matthijsvk/stock_market_monte_carlo (src/simulations.{cpp,cu}).  See DESIGN.md."""
from ._lib import BLOCKS_CIRCULAR, MAX_ASSETS, MAX_CASHFLOW_PERIODS, MAX_EXCURSION_PERIODS, MAX_GLIDE_CHANGES, MAX_SWEEP, MAX_SWEEP_COUNTERS, MODE_GAUSSIAN, MODE_TABLE, SmmcError  # noqa: F401
from .engine import (AllocationSweepResult, CashflowResult, Engine, ExcursionResult, Fan, Group, GuardrailsResult, PortfolioCashflowResult, PortfolioResult, RealCashflowResult, Stats, SweepResult, cholesky_factor, fan, glide_linear, many_updates, mc_simulations, mc_simulations_gpu,  # noqa: F401
                     mc_simulations_gpu_reduceBlock, mc_simulations_keepdata, read_historical_returns,
                     reduce_mean_gpu, update_count_below_min, update_fund, update_mean_std, update_quartiles,
                     vector_add_gpu)
from .stationary import renew_q16_of, simulate_stationary, simulate_stationary_raw, simulate_stationary_to_host, stationary_divide_kind  # noqa: F401
from .regimes import make_regimes, regimes_divide_kind, simulate_regimes, simulate_regimes_raw, simulate_regimes_to_host  # noqa: F401
from .regimes import (make_portfolio_regimes, portfolio_cashflow_regimes_divide_kind, simulate_portfolio_cashflow_regimes,  # noqa: F401
                      simulate_portfolio_cashflow_regimes_raw, simulate_portfolio_cashflow_regimes_to_host)
