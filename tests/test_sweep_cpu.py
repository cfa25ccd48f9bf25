"""Cash-flow sweeps without a GPU: the entry points are declared, exported and bound, the constants agree between the
header and Python, the ABI version and smmc_sim are what they were; every refusal include/smmc.h lists comes back as
SMMC_ERR_INVALID with a text and without a launch from the entries it applies to (csrc/smmc_sweep.cpp +
csrc/smmc_cashflow.cpp + csrc/smmc_capi.cpp over tests/cpp/fake_hip.cpp, driven by tests/cpp/sweep_args.cpp); the
divide rule; SweepResult on hand-made counts; and the monotonicity property of include/smmc.h on the numpy
restatement (tests/cashflow_reference.py), with the depletion shares the amount sets were chosen by.

Not reachable, with the reason: "tables and counters beyond the device's LDS".  The largest request the other checks
let through is a 16384-entry table (64 KiB) with SMMC_MAX_SWEEP_COUNTERS counters (32 KiB) and 64 wave partials
(3.5 KiB); an engine assumes 128 KiB at the least."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cashflow_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = {"smmc_engine_simulate_cashflow_sweep": 9, "smmc_engine_simulate_cashflow_sweep_to_host": 9,
         "smmc_engine_cashflow_sweep_divide_kind": 4}
# the issue's amount sets: 360 periods and 7 periods, capital 1000, floor 0.01
AMOUNTS = {360: (0.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 12.0), 7: (0.0, 100.0, 130.0, 145.0, 160.0, 200.0, 400.0, 1001.0)}
# depleted shares of the first 2000 paths, by the restatement
SHARES = {("gaussian", 360): (0, 0, 0, 0, 0.009, 0.547, 1, 1), ("table", 360): (0, 0.009, 0.078, 0.246, 0.435, 0.634, 0.878, 0.989),
          ("table3001", 360): (0, 0.002, 0.013, 0.075, 0.177, 0.357, 0.708, 0.983),
          ("gaussian", 7): (0, 0, 0, 0.346, 1, 1, 1, 1), ("table", 7): (0, 0, 0.063, 0.502, 0.917, 1, 1, 1),
          ("table3001", 7): (0, 0, 0.038, 0.422, 0.917, 1, 1, 1)}


def test_entry_points_are_declared_exported_and_bound():
    from stock_market_monte_carlo_amd import _lib, build
    import stock_market_monte_carlo_amd as S
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    build.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for name, n_args in NAMES.items():
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound and len(bound[name][2]) == n_args, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    m = re.search(r"#define SMMC_MAX_SWEEP (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_SWEEP == S.MAX_SWEEP == 8
    m = re.search(r"#define SMMC_MAX_SWEEP_COUNTERS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_SWEEP_COUNTERS == S.MAX_SWEEP_COUNTERS == 8192
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert ctypes.sizeof(_lib.Sim) == 72 and ctypes.sizeof(_lib.Cashflow) == 40  # unchanged
    assert "smmc_sweep.cpp" in build.SOURCES  # part of the build digest
    for name in ("simulate_cashflow_sweep", "simulate_cashflow_sweep_raw", "simulate_cashflow_sweep_to_host", "cashflow_sweep_divide_kind"):
        assert hasattr(S.Engine, name), name
    assert S.SweepResult


def test_the_other_host_units_gained_no_undefined_symbol(tmp_path):
    """csrc/smmc_capi.cpp and csrc/smmc_cashflow.cpp still link against the stand-ins that predate this feature."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for unit in ("smmc_capi.cpp", "smmc_cashflow.cpp"):
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        assert "sweep" not in undefined, (unit, undefined)


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/sweep_args.cpp over the fake HIP runtime: {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("sw") / "sweep_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_sweep.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "sweep_launch_stub.cpp", "sweep_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sweep_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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
INVALID = {"scenarios_null": "scenarios", "no_scenarios": "n_scenarios", "nine_scenarios": "SMMC_MAX_SWEEP",
           "scenario_with_amounts": "scenarios[5]", "scenario_with_fractions": "scenarios[2]", "struct_size_wrong": "struct_size",
           "floor_negative": "floor", "floor_infinite": "floor", "floor_nan": "floor", "amount_nan": "amount",
           "fraction_infinite": "fraction", "n_periods_zero": "n_periods", "n_periods_above_max": "SMMC_MAX_CASHFLOW_PERIODS",
           "stream_ref": "REF", "stream_v2": "V2", "table_mode_without_table": "table", "n_bins_above_max": "n_bins",
           "histogram_range_empty": "hist", "engine_null": "engine", "sim_struct_size_wrong": "struct_size"}
CALL_ONLY = {"counter_cap_8_x_1000_64_bins": "SMMC_MAX_SWEEP_COUNTERS", "counter_cap_2_x_max_periods": "SMMC_MAX_SWEEP_COUNTERS",
             "paths_per_workgroup": "shard"}
DEVICE_ONLY = {"final_misaligned": "aligned", "depleted_at_misaligned": "aligned"}


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    assert INVALID[case].lower() in args_report["_text"][f"{entry}:{case}"].lower(), args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry,case", [(e, c) for e in ("device", "to_host") for c in sorted(CALL_ONLY)]
                         + [("device", c) for c in sorted(DEVICE_ONLY)])
def test_errors_of_the_simulating_entries(args_report, entry, case):
    """The counter cap: S = 8, P = 1000, 64 buckets needs 8 x 1065 = 8520 > 8192 counters."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)
    assert {**CALL_ONLY, **DEVICE_ONLY}[case] in args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", ["valid_8", "valid_3", "valid_1", "valid_5_table", "valid_7_x_1000_64_bins", "valid_8_x_1000_no_stats",
                                  "valid_1_x_max_periods"])
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result.  S = 7
    at P = 1000 with 64 buckets (7455 counters) passes where S = 8 is refused; so does S = 8 without the record."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1, (entry, case, rc)


FAST, EXACT = 0, 1
KINDS = {"all_fast": FAST, "all_fast_table": FAST, "exact_flag": EXACT, "one_exact_among_eight": EXACT, "last_exact": EXACT,
         "single_fast": FAST, "single_exact": EXACT, "mixed_all_fast": FAST}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_rule(args_report, case):
    """FAST if and only if the single call's rule says FAST for every scenario; the exact flag gives EXACT."""
    assert args_report["kind:" + case] == (KINDS[case],)


def test_sizes_and_constants_of_the_header(args_report):
    assert args_report["sizes"] == (72, 40) and args_report["constants"] == (8, 8192, 4)


def test_the_product_does_not_touch_the_reference_of_its_tests():
    text = open(os.path.join(CSRC, "smmc_sweep.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "cashflow_reference" not in text
    assert "log2" not in text and "host_multiplier_bounds" not in text  # the divide rule is stated once, in smmc_cashflow.cpp


# ---- SweepResult ----------------------------------------------------------------------------------------------------------

def _result(depleted_at, amounts):
    from stock_market_monte_carlo_amd import SweepResult
    am = np.asarray(amounts, dtype=np.float32)
    d = np.asarray(depleted_at, dtype=np.uint64)
    return SweepResult(int(d[0].sum()), d.shape[1] - 1, am, np.zeros_like(am), np.zeros_like(am), depleted_at=d)


def test_sweep_result_from_hand_made_counts():
    from stock_market_monte_carlo_amd import CashflowResult, SweepResult
    dep = [[10, 0, 0, 0, 0], [9, 0, 1, 0, 0], [4, 1, 0, 3, 2], [0, 5, 5, 0, 0]]
    r = _result(dep, [1.0, 2.0, 3.0, 4.0])
    s = r.survival()
    assert s.shape == (4, 5)
    assert np.allclose(s, [[1, 1, 1, 1, 1], [1, 1, 0.9, 0.9, 0.9], [1.0, 0.9, 0.9, 0.6, 0.4], [1, 0.5, 0, 0, 0]])
    for row, d in zip(s, dep):
        assert np.array_equal(row, CashflowResult(10, 4, depleted_at=np.array(d, dtype=np.uint64)).survival())
    assert np.allclose(r.depleted_share(), [0.0, 0.1, 0.6, 1.0])
    assert r.highest_surviving(0.95) == 0 and r.highest_surviving(0.9) == 1 and r.highest_surviving(0.4) == 2
    assert r.highest_surviving(0.0) == 3 and r.highest_surviving(1.0) == 0
    # the largest AMOUNT counts, not the position
    shuffled = _result([dep[2], dep[0], dep[3], dep[1]], [3.0, 1.0, 4.0, 2.0])
    assert shuffled.highest_surviving(0.9) == 3 and shuffled.highest_surviving(0.95) == 1
    assert _result([dep[3]], [4.0]).highest_surviving(0.5) is None
    with pytest.raises(ValueError):
        SweepResult(5, 2, np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)).survival()
    with pytest.raises(ValueError):
        SweepResult(5, 2, np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)).depleted_share()


def test_make_sweep_broadcasts_scalars():
    from stock_market_monte_carlo_amd import Engine
    cfs, am, fr, fl = Engine.make_sweep([1.0, 2.0, 3.0], 0.004, floors=[0.0, 0.01, 0.02])
    assert len(cfs) == 3 and list(am) == [1.0, 2.0, 3.0] and list(fr) == [np.float32(0.004)] * 3
    assert [c.struct_size for c in cfs] == [40] * 3 and [c.floor for c in cfs] == [0.0, np.float32(0.01), np.float32(0.02)]
    assert all(c.amounts is None and c.fractions is None for c in cfs)
    assert len(Engine.make_sweep(5.0)[0]) == 1
    with pytest.raises(ValueError):
        Engine.make_sweep([1.0, 2.0, 3.0], [0.1, 0.2])


# ---- monotonicity, on the restatement -------------------------------------------------------------------------------

def _mode(name):
    return (1, "none") if name == "gaussian" else (0, "bundled" if name == "table" else "big")


@pytest.mark.parametrize("P", [360, 7])
@pytest.mark.parametrize("mode_name", ["gaussian", "table", "table3001"])
def test_monotone_in_the_amount_on_the_restatement(oracle, mode_name, P):
    """Equal floor, fraction 0, amounts ascending: on every path the final value does not rise and the period of
    depletion does not get later ("never" counting as latest) from one scenario to the next; and the amount sets do what
    they were chosen for: one scenario depletes nobody, one some but not all, and those stated as 1 everybody."""
    n = 2000
    mode, key = _mode(mode_name)
    R = ref.cached_returns(oracle, mode, key, n, P)
    runs = [ref.simulate(R, a, 0.0, ref.FLOOR) for a in AMOUNTS[P]]
    shares = [float((ruin > 0).mean()) for _, _, ruin, _ in runs]
    print(mode_name, P, shares)
    assert shares == pytest.approx(SHARES[(mode_name, P)], abs=0.00051)  # the stated shares have three decimals
    assert any(s == 0.0 for s in shares) and any(0.0 < s < 1.0 for s in shares)
    assert all(s == 1.0 for s, stated in zip(shares, SHARES[(mode_name, P)]) if stated == 1)
    if (mode_name, P) == ("gaussian", 360):
        assert 0.0 < shares[4] < 1.0 and 0.0 < shares[5] < 1.0  # 5.0 and 6.0
    latest = lambda ruin: np.where(ruin == 0, P + 1, ruin)  # noqa: E731
    for (va, _, ra, _), (vb, _, rb, _) in zip(runs, runs[1:]):
        assert (vb <= va).all() and (latest(rb) <= latest(ra)).all()
