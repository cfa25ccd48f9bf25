"""Allocation sweeps without a GPU: the scenario sets that run on the device (tests/allocation_sweep_reference.py), checked
on the restatement alone so that no device case is vacuous; the entry points declared, exported and bound; every argument
error include/smmc.h lists as SMMC_ERR_INVALID with a text and without a launch, from all three entries where it applies,
the divide rule's answers, the padding a launch is given and the accumulator lease after a failed launch
(csrc/smmc_allocation_sweep.cpp + the library's other host units over tests/cpp/fake_hip.cpp, driven by
tests/cpp/allocation_sweep_args.cpp, built with -fsanitize=address,undefined and run directly); and the ledger of the
compiled instantiations of allocation_sweep_kernel, each with a request that reaches it.

A set of ONE scenario cannot both deplete no path and deplete a share inside (0.05, 0.95): the S = 1 cases run the level
amount and are held to the second condition; every larger set is held to both.

Not reachable, with the reason: "asset table, counters and partials beyond the device's LDS".  The largest request the
other checks let through is 4096 rows of 4 assets (64 KiB), SMMC_MAX_SWEEP_COUNTERS counters (32 KiB) and 8 x 4 partials,
98 KiB; an engine assumes 128 KiB at the least and the check keeps 2 KiB back, so the refusal guards a device smaller than
any the library runs on."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import allocation_sweep_reference as ref
from stock_market_monte_carlo_amd._lib import AllocationSweepOutputs  # noqa: F401  without the feature the module has no subject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_allocation_sweep", "smmc_engine_simulate_allocation_sweep_to_host",
         "smmc_engine_allocation_sweep_divide_kind")


# ---- the scenario sets of the device tests, on the restatement alone ------------------------------------------------

def _shares(oracle, shape, K, P, scenarios, n=2000):
    return [float((ref.reference(oracle, shape, K, P, sc)["ruin_period"][:n] > 0).mean()) for sc in scenarios]


def test_every_device_set_has_a_scenario_that_depletes_nothing_and_one_that_depletes_a_good_part(oracle):
    for tag, shape, K, P, scenarios in ref.device_sets(oracle):
        shares = _shares(oracle, shape, K, P, scenarios, 255 if P > 360 else 2000)
        assert any(x == 0.0 for x in shares), (tag, shares)
        assert any(0.05 < x < 0.95 for x in shares), (tag, shares)


def test_the_single_scenario_cases_deplete_a_good_part(oracle):
    for shape, K, P, S, n in ref.PARITY_CASES:
        if S == 1:
            (share,) = _shares(oracle, shape, K, P, ref.uniform_set(oracle, shape, K, P, 1))
            assert 0.05 < share < 0.95, (shape, K, P, share)


@pytest.mark.parametrize("shape,K", ref.MIXED_CASES)
def test_the_mixed_set_differs_in_everything_and_weights_alone_part_two_scenarios(oracle, shape, K):
    mixed = ref.mixed_set(oracle, shape, K, 360)
    assert len(mixed) == 8 and {sc[1] for sc in mixed} == {0, 1, 5, 12}
    assert len({sc[0] for sc in mixed}) == 8 and any(0.0 in sc[0] for sc in mixed)  # one allocation has a zero weight
    assert len({sc[2] for sc in mixed}) > 4 and len({sc[3] for sc in mixed}) == 3 and len({sc[4] for sc in mixed}) == 3
    assert mixed[0][1:] == mixed[7][1:] and mixed[0][0] != mixed[7][0]  # the same R, flow and floor on other weights
    a, b = (ref.reference(oracle, shape, K, 360, mixed[i])["ruin_period"][:4099] for i in (0, 7))
    assert (a != b).any()
    c = ref.reference(oracle, shape, K, 360, mixed[4])["ruin_period"][:4099]  # floor 300 against floor 0.01
    assert (a != c).any()


def test_the_restatement_is_the_single_strategy_restatement(oracle):
    import portfolio_cashflow_reference as pcref
    scenarios = ref.mixed_set(oracle, "t37", 3, 360)[:3]
    a = ref.draws(oracle, "t37", 3, 360)[:300]
    for got, (w, R, am, fr, fl) in zip(ref.simulate(a, scenarios), scenarios):
        want = pcref.simulate(a, w, R, amount=am, fraction=fr, floor=fl)
        assert all(np.array_equal(got[k], want[k]) for k in want)


def test_the_cases_cover_what_the_issue_names():
    for shape in ref.SHAPES:
        mine = [c for c in ref.PARITY_CASES if c[0] == shape]
        assert {(P, S) for _, _, P, S, _ in mine} == {(P, S) for P in (7, 360) for S in (1, 3, 4, 5, 8)}
    assert {c[1] for c in ref.PARITY_CASES} == {1, 2, 3, 4} and {c[4] for c in ref.PARITY_CASES} == set(ref.PATHS)
    assert {n for _, _, _, S, n in ref.PARITY_CASES if S == 8} >= {4099, ref.N_MAX}
    assert ref.PATHS == [1, 255, 4099, 2 * 4099 + 1] and ref.FIRST_PATH == 2 ** 32 - 100 and ref.BINS == 64


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
    assert ctypes.sizeof(_lib.AllocationSweepOutputs) == 56
    assert "smmc_allocation_sweep.cpp" in build.SOURCES  # part of the build digest
    for name in ("make_allocation_sweep", "simulate_allocation_sweep", "simulate_allocation_sweep_raw",
                 "simulate_allocation_sweep_to_host", "allocation_sweep_divide_kind"):
        assert hasattr(S.Engine, name), name


def test_make_allocation_sweep_broadcasts_scalars():
    import stock_market_monte_carlo_amd as S
    pfs, cfs, w, every, am, fr, fl = S.Engine.make_allocation_sweep([[1, 0], [.8, .2], [.6, .4]], 12, [4.0, 5.0, 6.0], floors=0.01)
    assert w.shape == (3, 2) and list(every) == [12, 12, 12] and list(am) == [4.0, 5.0, 6.0] and not fr.any()
    assert [pfs[s].rebalance_every for s in range(3)] == [12, 12, 12] and [pfs[s].n_assets for s in range(3)] == [2, 2, 2]
    assert pfs[1].weights[0] == np.float32(0.8) and cfs[2].amount == 6.0 and cfs[0].floor == np.float32(0.01)
    assert list(S.Engine.make_allocation_sweep([[1.0]] * 2, [0, 5])[3]) == [0, 5]
    with pytest.raises(ValueError):
        S.Engine.make_allocation_sweep([[1, 0], [.8, .2]], amounts=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        S.Engine.make_allocation_sweep([1.0, 0.0])


def test_the_result_object_without_a_device():
    import stock_market_monte_carlo_amd as S
    dep = np.array([[4, 0, 0], [3, 1, 0], [1, 1, 2]], dtype=np.uint64)
    r = S.AllocationSweepResult(4, 2, np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), depleted_at=dep,
                                n_assets=2)
    assert isinstance(r, S.SweepResult) and r.holdings is None
    assert np.array_equal(r.survival(), [[1, 1, 1], [1, .75, .75], [1, .75, .25]]) and np.array_equal(r.depleted_share(), [0, .25, .75])
    assert r.surviving(0.75) == [0, 1] and r.surviving(0.2) == [0, 1, 2] and r.surviving(1.0) == [0]


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """The units that lend their checks gain no undefined symbol of the new kernel: the existing host-only programs link them
    against their own launch stubs."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    seen = {}
    for unit in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", "smmc_allocation_sweep.cpp"):
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        seen[unit] = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
    for unit in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp"):
        assert "allocation_sweep" not in seen[unit], (unit, seen[unit])
    mine = seen["smmc_allocation_sweep.cpp"]
    assert "launch_allocation_sweep" in mine and "smmc_engine_portfolio_cashflow_divide_kind" in mine
    assert "launch_portfolio_cashflow" not in mine and "launch_cashflow_sweep" not in mine and "launch_portfolio(" not in mine


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/allocation_sweep_args.cpp over the fake HIP runtime, under AddressSanitizer and UBSan: {case: tuple of
    ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("alsw") / "allocation_sweep_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", "smmc_allocation_sweep.cpp",
                                           "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "sweep_launch_stub.cpp", "excursions_launch_stub.cpp",
                                                            "blocks_launch_stub.cpp", "portfolio_launch_stub.cpp",
                                                            "portfolio_cashflow_launch_stub.cpp", "allocation_sweep_launch_stub.cpp",
                                                            "allocation_sweep_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "allocation_sweep_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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


# case -> words its error text must hold
INVALID = {"pfs_null": ["pfs"], "cfs_null": ["cfs"], "no_scenarios": ["n_scenarios"], "nine_scenarios": ["SMMC_MAX_SWEEP"],
           "scenario_with_amounts": ["cfs[5]", "arrays"], "scenario_with_fractions": ["cfs[2]", "arrays"],
           "law_n_assets_differs": ["pfs[6]", "n_assets"], "law_means_differ": ["pfs[3]", "means"],
           "law_factor_differs": ["pfs[7]", "factor"], "law_means_differ_in_sign_of_zero": ["pfs[2]", "means"],
           "engine_null": ["engine"], "sim_null": ["sim"], "sim_struct_size_wrong": ["struct_size"],
           "portfolio_struct_size_wrong": ["struct_size"], "no_assets": ["n_assets"], "reserved_not_zero": ["reserved"],
           "weight_negative": ["weights[0]"], "weight_nan": ["weights[1]"], "weights_do_not_sum_to_one": ["sum"],
           "table_mode_without_asset_table": ["set_asset_table"], "asset_table_of_other_width": ["columns"],
           "gaussian_fields_in_table_mode": ["table mode"], "factor_above_diagonal": ["factor[0][1]"], "stream_ref": ["REF"],
           "stream_v2": ["V2"], "n_bins_above_max": ["n_bins"], "histogram_range_empty": ["histogram"], "unknown_mode": ["mode"],
           "cashflow_struct_size_wrong": ["smmc_cashflow.struct_size"], "no_periods": ["n_periods"],
           "too_many_periods": ["SMMC_MAX_CASHFLOW_PERIODS"], "floor_negative": ["floor"], "floor_nan": ["floor"],
           "amount_infinite": ["amount"], "fraction_nan": ["fraction"]}
CALL_ONLY = {"outputs_null": "smmc_allocation_sweep_outputs", "outputs_struct_size_wrong": "struct_size",
             "outputs_reserved_not_zero": "reserved", "paths_per_workgroup": "shard",
             "counter_cap_8_x_1000_64_bins": "SMMC_MAX_SWEEP_COUNTERS", "counter_cap_2_x_max_periods": "SMMC_MAX_SWEEP_COUNTERS"}
DEVICE_ONLY = {"holdings_misaligned": "4-byte", "depleted_at_misaligned": "8-byte"}
VALID = ["valid_8_gaussian", "valid_8_table", "valid_5", "valid_4", "valid_3", "valid_1", "valid_no_outputs",
         "valid_7_x_1000_64_bins", "valid_8_x_1000_no_stats", "valid_1_x_max_periods"]


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    for word in INVALID[case]:
        assert word in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry,case", [(e, c) for e in ("device", "to_host") for c in sorted(CALL_ONLY)]
                         + [("device", c) for c in sorted(DEVICE_ONLY)])
def test_errors_of_the_two_simulating_entries(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)
    assert {**CALL_ONLY, **DEVICE_ONLY}[case] in args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", VALID)
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_and_no_error(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)


FAST, EXACT = 0, 1
KINDS = {"each_of_the_eight_alone": FAST, "all_fast_table": FAST, "all_fast_gaussian_36": FAST, "gaussian_360": EXACT,
         "exact_flag": EXACT, "one_exact_among_eight": EXACT, "last_exact": EXACT, "single_fast": FAST, "single_exact": EXACT}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_rule(args_report, case):
    """FAST if and only if the single call's rule says FAST for every scenario; never the checked form."""
    assert args_report["kind:" + case] == (KINDS[case],)


def test_a_launch_is_given_the_form_the_rule_names(args_report):
    assert args_report["ran:fast"] == (-2, 0) and args_report["ran:exact"] == (-2, 1)


@pytest.mark.parametrize("S,width", [(1, 4), (3, 4), (4, 4), (5, 8), (8, 8)])
def test_the_padded_scenarios_are_copies_of_the_last_real_one(args_report, S, width):
    assert args_report[f"padding:{S}"] == (-2, 1, 1, width)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1)


def test_sizes_of_the_structures_and_constants(args_report):
    from stock_market_monte_carlo_amd import _lib
    assert args_report["sizes"] == (ctypes.sizeof(_lib.Sim), ctypes.sizeof(_lib.Portfolio), ctypes.sizeof(_lib.Cashflow),
                                    ctypes.sizeof(_lib.AllocationSweepOutputs)) == (72, 112, 40, 56)
    assert args_report["constants"] == (_lib.MAX_SWEEP, 8192, 4)


def test_the_product_does_not_touch_the_oracle():
    text = open(os.path.join(CSRC, "smmc_allocation_sweep.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text


# ---- the ledger: every compiled instantiation of allocation_sweep_kernel, with a request that reaches it --------------

# (mode, exact_div, dense, K, width) -> (shape, K, P, S, exact_div flag): mode 1 = Gaussian, 0 = table; t37 is a dense table
# (eight draws per block), t2500 a wide one (four); the uniform set of S scenarios at P = 9 (dense) or 5 periods is FAST by
# the rule (tests/test_allocation_sweep_gpu.py asserts it before it runs the row), the flag asks for the IEEE divide
LEDGER = {(mode, exact, dense, K, width): ("gauss" if mode else ("t37" if dense else "t2500"), K, 9 if dense else 5,
                                           3 if width == 4 else 6, bool(exact))
          for mode, dense in ((1, 0), (0, 1), (0, 0)) for exact in (0, 1) for K in (1, 2, 3, 4) for width in (4, 8)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def test_the_ledger_names_exactly_the_compiled_instantiations(asm):
    """Names only: no instruction is read."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_table as T
    prefix, symbols = T.instantiations(asm, "allocation_sweep_kernel")
    compiled = set()
    for sym in symbols:
        m = re.match(r"ILi(\d)ELb(\d)ELb(\d)ELi(\d)ELi(\d)EEE", sym[len(prefix):])
        assert m, sym
        compiled.add(tuple(int(x) for x in m.groups()))
    assert len(symbols) == len(compiled) == 48
    assert compiled == set(LEDGER), (compiled - set(LEDGER), set(LEDGER) - compiled)
    from stock_market_monte_carlo_amd import _lib  # the widths the host pads to
    assert all(1 <= row[3] <= _lib.MAX_SWEEP and row[1] == key[3] for key, row in LEDGER.items())
