"""Cash-flow schedules without a GPU: the entry points are declared, exported and bound and the ABI version and
smmc_sim are what they were; every argument error include/smmc.h lists comes back as SMMC_ERR_INVALID with a text
from both entries (csrc/smmc_cashflow.cpp + csrc/smmc_capi.cpp over tests/cpp/fake_hip.cpp, driven by
tests/cpp/cashflow_args.cpp); the divide rule's answers; survival() against a hand-made depleted_at; and the numpy
restatement of the arithmetic (tests/cashflow_reference.py) against the CPU oracle where there is no cash flow."""
import os
import re
import subprocess

import numpy as np
import pytest

import cashflow_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_cashflow", "smmc_engine_simulate_cashflow_to_host")


def test_entry_points_are_declared_exported_and_bound():
    import ctypes
    from stock_market_monte_carlo_amd import _lib, build
    import stock_market_monte_carlo_amd as S
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    build.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound and len(bound[name][2]) == 8, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert "smmc_engine_cashflow_divide_kind" in bound and len(bound["smmc_engine_cashflow_divide_kind"][2]) == 3
    m = re.search(r"#define SMMC_MAX_CASHFLOW_PERIODS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_CASHFLOW_PERIODS == S.MAX_CASHFLOW_PERIODS == 4096
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert ctypes.sizeof(_lib.Sim) == 72  # unchanged: 68 bytes of fields, 8-byte aligned
    assert "smmc_cashflow.cpp" in build.SOURCES  # part of the build digest


def test_the_engine_unit_gained_no_undefined_symbol(tmp_path):
    """csrc/smmc_capi.cpp still links against the stand-ins that predate this feature: it refers to nothing of
    csrc/smmc_cashflow.cpp or of the cash-flow kernel."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    obj = str(tmp_path / "smmc_capi.o")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, "smmc_capi.cpp"), "-o", obj])
    undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
    assert "cashflow" not in undefined and "finalize_depleted" not in undefined, undefined


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/cashflow_args.cpp over the fake HIP runtime: {case: (return code, length of the error text)}."""
    exe = str(tmp_path_factory.mktemp("cf") / "cashflow_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "cashflow_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cashflow_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and not line.startswith("#"):
            out[parts[0]] = (int(parts[1]), int(parts[2]))
    return out


INVALID = ["cf_null", "struct_size_wrong", "n_periods_zero", "n_periods_above_max", "floor_negative", "floor_infinite",
           "floor_nan", "amount_nan", "fraction_infinite", "amounts_entry_infinite", "fractions_entry_nan", "stream_ref",
           "stream_v2", "table_mode_without_table", "n_bins_above_max", "histogram_range_empty", "engine_null"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", INVALID)
def test_argument_errors_are_invalid_with_a_text(args_report, entry, case):
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -1, (entry, case, rc)  # SMMC_ERR_INVALID
    assert text_len > 0


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", ["valid_constant", "valid_arrays", "valid_max_periods"])
def test_a_valid_request_passes_the_argument_checks(args_report, entry, case):
    """The host-only build then stops at its missing kernel: an error of its own (SMMC_ERR_HIP), not
    SMMC_ERR_INVALID and not a result."""
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"][:2] == (72, 40)  # smmc_sim as before; smmc_cashflow as _lib.Cashflow lays it out
    import ctypes
    from stock_market_monte_carlo_amd import _lib
    assert ctypes.sizeof(_lib.Cashflow) == 40


FAST, EXACT = 0, 1
DIVIDE = {"zero_flow": FAST, "fraction_only_floor_0": FAST, "amount_floor_0": EXACT, "amount_floor_cent": FAST,
          "collapse_floor_cent": FAST, "fraction_half_floor_0": EXACT, "fraction_negative": EXACT,
          "fraction_above_one": EXACT, "contribution": FAST, "contribution_huge": EXACT, "tiny_floor": EXACT,
          "exact_flag": EXACT, "table": FAST}


@pytest.mark.parametrize("case", sorted(DIVIDE))
def test_the_divide_rule(args_report, case):
    """The fast divide only where the header's rule proves every live product inside its domain: a floor (or
    nothing but contributions and fractions below 1) below, fractions in [0, 1] and the contributions above."""
    assert args_report["divide:" + case][0] == DIVIDE[case]


def test_survival_from_a_hand_made_depleted_at():
    from stock_market_monte_carlo_amd import CashflowResult
    r = CashflowResult(10, 4, depleted_at=np.array([4, 1, 0, 3, 2], dtype=np.uint64))
    assert np.allclose(r.survival(), [1.0, 0.9, 0.9, 0.6, 0.4])
    assert r.survival().size == 5 and r.survival()[-1] == pytest.approx(4 / 10)  # what is left = never depleted
    none = CashflowResult(5, 2, depleted_at=np.array([5, 0, 0], dtype=np.uint64))
    assert (none.survival() == 1.0).all()
    with pytest.raises(ValueError):
        CashflowResult(5, 2).survival()


@pytest.mark.parametrize("mode,table_key", [(1, "none"), (0, "bundled")])
def test_the_restatement_without_cash_flow_is_the_oracle(oracle, table, mode, table_key):
    """300 x 360: with amount = fraction = 0 and floor 0 the numpy restatement gives the oracle engine's final
    values bit for bit, nothing is paid and nobody is depleted."""
    n, P = 300, 360
    R = ref.returns(oracle, mode, table if mode == 0 else None, n, P)
    v, paid, ruin, dep = ref.simulate(R, 0.0, 0.0, 0.0)
    p = oracle.make_params(mode, P, n, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL,
                           table=table if mode == 0 else None)
    want = oracle.counter_mc(p)["final"]
    assert np.array_equal(v.view(np.uint32), want.view(np.uint32))
    assert not paid.any() and not ruin.any() and dep[0] == n and dep.sum() == n


def test_the_restatement_depletes_and_pays_as_stated(oracle):
    """A hand-checkable path: returns of 0 %, capital 100, 30 out per period, floor 0.01: 70, 40, 10, then the
    fourth withdrawal does not fit: the path pays the 10 that are left and is depleted at period 4."""
    R = np.zeros((1, 6), dtype=np.float32)
    v, paid, ruin, dep = ref.simulate(R, 30.0, 0.0, 0.01, capital=100.0)
    assert v[0] == 0.0 and paid[0] == 100.0 and ruin[0] == 4 and list(dep) == [0, 0, 0, 0, 1, 0, 0]
    # contributions keep a path alive but never bring a depleted one back
    am = np.array([60.0, 60.0, -500.0, -500.0, 0.0, 0.0], dtype=np.float32)
    v, paid, ruin, dep = ref.simulate(R, am, 0.0, 0.01, capital=100.0)
    assert v[0] == 0.0 and paid[0] == 100.0 and ruin[0] == 2
    v, paid, ruin, dep = ref.simulate(R, -am, 0.0, 0.01, capital=100.0)   # pays in 120, then takes out 1000
    assert ruin[0] == 3 and paid[0] == np.float32(-120.0 + 220.0) and v[0] == 0.0
