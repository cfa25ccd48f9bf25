"""Portfolio cash flows without a GPU: the restatement of the contract (tests/portfolio_cashflow_reference.py) against
the two restatements it must agree with -- tests/cashflow_reference.py for one asset of weight 1, tests/
portfolio_reference.py for zero flows --, its prefix property, the sizing of the schedules that run on the device, a
live path with a negative holding; the entry points declared, exported and bound; every argument error include/smmc.h
lists as SMMC_ERR_INVALID with a text and without a launch, from all three entries, the divide rule's answers and the
accumulator lease after a failed launch (csrc/smmc_portfolio_cashflow.cpp + the library's other host units over
tests/cpp/fake_hip.cpp, driven by tests/cpp/portfolio_cashflow_args.cpp, built with -fsanitize=address,undefined and run
directly).

Not reachable, with the reason: "asset table, depletion counters and histogram beyond the device's LDS".  The largest
request the other checks let through is 5461 rows of 3 assets (padded to 4 words), 4097 depletion counters and 4096
buckets, 118 KiB with the partials; an engine assumes 128 KiB at the least and the check keeps 2 KiB back, so the
refusal guards a device smaller than any the library runs on."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cashflow_reference as cref
import portfolio_cashflow_reference as ref
import portfolio_reference as pref
from stock_market_monte_carlo_amd._lib import PortfolioCashflowOutputs  # noqa: F401  the contract restated here is this feature's: without it the module has no subject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_portfolio_cashflow", "smmc_engine_simulate_portfolio_cashflow_to_host",
         "smmc_engine_portfolio_cashflow_divide_kind")
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [37, 2500])
@pytest.mark.parametrize("name", ref.SCHEDULES)
def test_one_asset_with_weight_one_is_the_cash_flow_on_that_column(oracle, T, name):
    """final, paid, ruin_period and depleted_at of tests/cashflow_reference.py on the column's returns, for every R."""
    shape, P, n = "t%d" % T, 41, ref.n_paths("t")
    table = ref.asset_table(T, 1)
    rows = pref.row_indices(oracle, T, ref.SEED, ref.FIRST_PATH, n, P)
    kw = ref.schedules(oracle, shape, 1, (1.0,))[name]
    sched = dict(amount=kw.get("amounts", kw.get("amount", 0.0)), fraction=kw.get("fractions", kw.get("fraction", 0.0)),
                 floor=kw.get("floor", 0.0))
    final, paid, ruin, depleted_at = cref.simulate(table[rows, 0], capital=ref.CAPITAL, **sched)
    assert 0 < depleted_at[0] < n
    for R in ref.REBALANCE:
        got = ref.reference(oracle, shape, 1, (1.0,), R, name, P)
        assert np.array_equal(_bits(got["final"]), _bits(final)) and np.array_equal(_bits(got["holdings"][0]), _bits(final)), R
        assert np.array_equal(_bits(got["paid"]), _bits(paid)) and np.array_equal(got["ruin_period"], ruin), R
        assert np.array_equal(got["depleted_at"], depleted_at), R


@pytest.mark.parametrize("shape,K", [("t37", 3), ("t2500", 2), ("gauss", 4)])
@pytest.mark.parametrize("R", [0, 5, 12])
def test_zero_flows_are_the_plain_portfolio(oracle, shape, K, R):
    n, P = ref.n_paths(shape), ref.longest(shape)
    a = ref.multipliers(oracle, shape, K, n, P)
    values, holdings = pref.simulate(a, ref.WEIGHTS[K], R)
    assert np.isfinite(values).all() and (values > 0).all()
    got = ref.simulate(a, ref.WEIGHTS[K], R)
    assert np.array_equal(_bits(got["final"]), _bits(values[:, P])) and np.array_equal(_bits(got["holdings"]), _bits(holdings))
    assert not got["paid"].any() and not got["ruin_period"].any() and got["depleted_at"][0] == n


@pytest.mark.parametrize("shape,K", [("t37", 3), ("gauss", 2)])
@pytest.mark.parametrize("name", ["amount", "varying"])
def test_the_final_value_does_not_depend_on_n_periods(oracle, shape, K, name):
    """Column p of the longest run is the final value of a run of p periods (whose last period never rebalances), and so
    are paid and ruin_period up to there."""
    n, P, R = 70, ref.longest(shape), 5
    a = ref.multipliers(oracle, shape, K, ref.n_paths(shape), P)[:n]
    kw = ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name]
    long = ref.simulate(a, ref.WEIGHTS[K], R, columns=True, **kw)
    for p in range(1, P + 1):
        short = ref.simulate(a[:, :p], ref.WEIGHTS[K], R, **ref.cut(kw, p))
        assert np.array_equal(_bits(short["final"]), _bits(long["values"][:, p])), p
        assert np.array_equal(short["ruin_period"], np.where(long["ruin_period"] <= p, long["ruin_period"], 0)), p


def _device_cases():
    for shape, K in ref.SHAPES:
        yield shape, K, ref.WEIGHTS[K]
    yield ref.ZERO_WEIGHT + (ref.WEIGHTS_WITH_ZERO[ref.ZERO_WEIGHT[1]],)


@pytest.mark.parametrize("shape,K,weights", list(_device_cases()))
def test_the_schedules_run_on_the_device_deplete_a_good_part_of_the_paths_and_not_all(oracle, shape, K, weights):
    n, P = ref.n_paths(shape), ref.longest(shape)
    for name in ref.SCHEDULES:
        for R in ref.REBALANCE:
            got = ref.reference(oracle, shape, K, weights, R, name, P)
            depleted = 1.0 - got["depleted_at"][0] / n
            assert int(got["depleted_at"].sum()) == n and 0.10 <= depleted <= 0.90, (shape, K, name, R, depleted)
            alive = got["ruin_period"] == 0
            assert (got["final"][alive] > 0).all() and not got["final"][~alive].any() and not got["holdings"][:, ~alive].any()
    kw = ref.schedules(oracle, shape, K, weights)["varying"]
    assert (kw["amounts"][:10] < 0).all() and (kw["amounts"][10:] > 0).all()  # contributions first, then withdrawals


@pytest.mark.parametrize("shape,K", [("t37", 2), ("gauss", 4)])
def test_buy_and_hold_with_long_withdrawals_ends_with_a_negative_holding_on_a_live_path(oracle, shape, K):
    """The contract does not clamp a holding: the value alone decides depletion."""
    got = ref.reference(oracle, shape, K, ref.WEIGHTS[K], 0, "amount", ref.longest(shape))
    live_negative = (got["ruin_period"] == 0) & (got["holdings"] < 0).any(axis=0)
    assert live_negative.any() and (got["final"][live_negative] > 0).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound():
    from stock_market_monte_carlo_amd import _lib, build
    import stock_market_monte_carlo_amd as S
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    build.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert ctypes.sizeof(_lib.PortfolioCashflowOutputs) == 56 and ctypes.sizeof(_lib.Cashflow) == 40
    assert "smmc_portfolio_cashflow.cpp" in build.SOURCES  # part of the build digest
    for name in ("simulate_portfolio_cashflow", "simulate_portfolio_cashflow_raw", "simulate_portfolio_cashflow_to_host",
                 "portfolio_cashflow_divide_kind"):
        assert hasattr(S.Engine, name), name
    r = S.PortfolioCashflowResult(4, 2, depleted_at=np.array([1, 2, 1], dtype=np.uint64), n_assets=2)
    assert np.array_equal(r.survival(), [1.0, 0.5, 0.25]) and r.holdings is None


def test_only_the_new_unit_refers_to_the_new_launch_symbols(tmp_path):
    """csrc/smmc_cashflow.cpp and csrc/smmc_portfolio.cpp lend their checks and gain no undefined symbol of the new kernel:
    the existing host-only programs link them against their own launch stubs."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    seen = {}
    for unit in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp"):
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        seen[unit] = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
    for unit in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_portfolio.cpp"):
        assert "portfolio_cashflow" not in seen[unit], (unit, seen[unit])
    assert "launch_portfolio_cashflow" in seen["smmc_portfolio_cashflow.cpp"]
    assert "launch_portfolio(" not in seen["smmc_portfolio_cashflow.cpp"] and "launch_cashflow(" not in seen["smmc_portfolio_cashflow.cpp"]


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/portfolio_cashflow_args.cpp over the fake HIP runtime, under AddressSanitizer and UBSan: {case: tuple of
    ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("pfcf") / "portfolio_cashflow_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "portfolio_cashflow_launch_stub.cpp",
                                                            "portfolio_cashflow_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "portfolio_cashflow_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out, text, last = {}, {}, None
    for line in r.stdout.splitlines():
        if line.startswith("#") and last:
            text[last] = line[1:].strip()
            continue
        parts = line.split()
        if len(parts) >= 2 and all(re.fullmatch(r"-?\d+", x) for x in parts[1:]):
            out[parts[0]] = tuple(int(x) for x in parts[1:])
            last = parts[0]
    out["_text"] = text
    return out


# case -> a word its error text must hold
INVALID = {"engine_null": "engine", "sim_null": "sim", "sim_struct_size_wrong": "struct_size", "portfolio_null": "smmc_portfolio",
           "portfolio_struct_size_wrong": "struct_size", "no_assets": "n_assets", "five_assets": "n_assets",
           "reserved_not_zero": "reserved", "weight_negative": "weights[0]", "weight_nan": "weights[0]",
           "weight_infinite": "weights[1]", "weight_beyond_assets": "weights[2]", "weights_do_not_sum_to_one": "sum",
           "table_mode_without_asset_table": "set_asset_table", "asset_table_of_other_width": "columns",
           "gaussian_fields_in_table_mode": "table mode", "mean_nan": "means[1]", "factor_infinite": "factor[1][0]",
           "factor_above_diagonal": "factor[0][1]", "factor_beyond_assets": "factor[2][2]", "mean_beyond_assets": "means[3]",
           "diagonal_negative": "diagonal", "stream_ref": "REF", "stream_v2": "V2", "n_bins_above_max": "n_bins",
           "histogram_range_empty": "histogram", "unknown_mode": "mode",
           "cashflow_null": "cf", "cashflow_struct_size_wrong": "smmc_cashflow.struct_size", "no_periods": "n_periods",
           "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS", "floor_negative": "floor", "floor_nan": "floor",
           "amount_infinite": "amount", "fraction_nan": "fraction", "amounts_entry_nan": "amounts[200]",
           "fractions_entry_infinite": "fractions[359]"}
CALL_ONLY = {"outputs_null": "smmc_portfolio_cashflow_outputs", "outputs_struct_size_wrong": "struct_size",
             "outputs_reserved_not_zero": "reserved", "paths_per_workgroup": "shard"}
DEVICE_ONLY = {"paid_misaligned": "4-byte", "depleted_at_misaligned": "8-byte"}


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    assert INVALID[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry,case", [(e, c) for e in ("device", "to_host") for c in sorted(CALL_ONLY)]
                         + [("device", c) for c in sorted(DEVICE_ONLY)])
def test_errors_of_the_two_simulating_entries(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)
    assert {**CALL_ONLY, **DEVICE_ONLY}[case] in args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", ["valid_table", "valid_gaussian", "valid_buy_and_hold", "valid_varying", "valid_largest",
                                  "valid_no_outputs"])
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result.  The
    table-mode requests run on an engine that has no single-series table."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_and_no_error(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)


FAST, EXACT = 0, 1
KINDS = {
    # required: schedules that take nothing out
    "zero_flows_table": FAST, "contributions_table": FAST, "contributions_varying_table": FAST,
    "contributions_varying_zero_fractions": FAST, "contributions_gaussian_36": FAST, "contributions_gaussian_360": EXACT,
    "contributions_too_large": EXACT, "one_withdrawal_among_contributions": EXACT,
    # wanted: one constant amount, fraction 0, a floor above 0 where a rebalance happens
    "withdrawal_floor_rebalanced": FAST, "withdrawal_floor_gaussian_36": FAST, "withdrawal_floor_gaussian_360": EXACT,
    "withdrawal_no_floor_rebalanced": EXACT, "withdrawal_no_floor_buy_and_hold": FAST,
    "withdrawal_no_floor_rebalance_never_reached": FAST, "withdrawal_tiny_amount": EXACT, "withdrawal_tiny_floor": EXACT,
    "withdrawal_zero_weight": FAST, "withdrawal_tiny_weight": EXACT,
    # unproven: the IEEE divide
    "fraction": EXACT, "amount_and_fraction": EXACT, "varying_withdrawals": EXACT, "exact_flag": EXACT,
    "table_doubling_360": EXACT, "table_doubling_36": FAST, "gaussian_may_go_negative": EXACT, "no_capital": EXACT}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_rule(args_report, case):
    """The fast divide only where the header's rule proves every product inside its domain; never the checked form."""
    assert args_report["kind:" + case] == (KINDS[case],)


def test_a_launch_is_given_the_form_the_rule_names(args_report):
    assert args_report["ran:fast"] == (-2, 0) and args_report["ran:exact"] == (-2, 1)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    """A call whose launch fails after it has counted into the engine's accumulator (buckets and depletion counters): the
    record of the next call, a plain simulate with buckets, is that call's alone."""
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 40, 56)


def test_the_product_does_not_touch_the_oracle():
    text = open(os.path.join(CSRC, "smmc_portfolio_cashflow.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text
