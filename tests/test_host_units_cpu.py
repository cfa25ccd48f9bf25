"""The host units' shared statements, by their source text (no compiler): the run of a wave-walk entry -- device,
accumulator lease, wiring, launch, folds -- is stated once, in csrc/smmc_host.h (host_wave_walk_run), and what only
host units share stays out of csrc/smmc_internal.h, which is part of the kernels' source digest."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
# smmc_capi.cpp defines engine_acc_lease and uses it in its own entries; smmc_blocks.cpp was left alone on purpose: its
# enqueue is smmc_capi.cpp's enqueue_simulation with another kernel (chunk statistics, the _to_host pipeline), no wave walk
LEASE_UNITS = {"smmc_capi.cpp", "smmc_blocks.cpp"}


def _code(name):
    """The file without its comments."""
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_wave_walk_run_is_stated_once():
    units = sorted(u for u in os.listdir(CSRC) if u.endswith(".cpp"))
    assert {"smmc_cashflow.cpp", "smmc_sweep.cpp", "smmc_excursions.cpp", "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp",
            "smmc_real_cashflow.cpp", "smmc_allocation_sweep.cpp"} <= set(units)
    assert {u for u in units if "engine_acc_lease(" in _code(u)} == LEASE_UNITS
    host = _code("smmc_host.h")
    for once in ("engine_acc_lease(e, &lease)", "launch_finalize_depleted(", "if (w.grid)", "out->reserved != 0", "finalize_queued();"):
        assert host.count(once) == 1, once
    for u in units:
        if u not in LEASE_UNITS:
            code = _code(u)
            assert "launch_finalize" not in code and "finalize_queued" not in code and "ZeroLease" not in code, u
            assert not re.search(r"\bout->reserved\b", code), u
            assert "host_timed_launch" not in code, u


def test_the_kernels_header_holds_nothing_of_the_host_side():
    code = _code("smmc_internal.h")
    for name in ("host_fail", "EngineView", "HostPiece", "DeviceGuard"):
        assert name not in code, name
    assert '#include "smmc_internal.h"' in _code("smmc_host.h")
