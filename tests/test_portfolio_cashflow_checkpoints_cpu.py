"""Portfolio cash-flow checkpoints without a GPU: what a record is, on the restatement alone
(tests/portfolio_cashflow_reference.py with columns=True); the entry points declared, exported and bound; which units
refer to which symbols; every argument error include/smmc.h lists as SMMC_ERR_INVALID with a text and without a launch,
the two budgets on both sides of their edges, no paths, the divide form a launch is given, the growth of the partial
array and the accumulator lease after a failed launch (csrc/smmc_portfolio_cashflow_checkpoints.cpp + the library's other
host units over tests/cpp/fake_hip.cpp, driven by tests/cpp/portfolio_cashflow_checkpoints_args.cpp, built with
-fsanitize=address,undefined and run directly); the ledger of the 48 instantiations against the kernels as they compile
now, none with scratch (the kernels' metadata; no instruction is looked at); the fuzz generator alone."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import feature_matrix as M
import portfolio_cashflow_checkpoints_fuzz as fuzz
import portfolio_cashflow_checkpoints_matrix as CM
import portfolio_cashflow_reference as ref
from stock_market_monte_carlo_amd.engine import PortfolioCashflowCheckpointsResult  # noqa: F401  without it the module has no subject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
UNIT = "smmc_portfolio_cashflow_checkpoints.cpp"
NAMES = ("smmc_engine_simulate_portfolio_cashflow_checkpoints", "smmc_engine_simulate_portfolio_cashflow_checkpoints_to_host")
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,K", ref.SHAPES)
def test_the_named_schedules_deplete_a_good_part_of_the_paths_and_not_all(oracle, shape, K):
    """The parent's own check, on the reference alone: no checkpoint test can pass on all-live or all-dead paths."""
    n, P = ref.n_paths(shape), ref.longest(shape)
    for name in ref.SCHEDULES:
        for R in (0, 5):
            got = ref.reference(oracle, shape, K, ref.WEIGHTS[K], R, name, P)
            assert 0.10 <= 1.0 - got["depleted_at"][0] / n <= 0.90, (shape, K, name, R)


@pytest.mark.parametrize("shape,K", [("t37", 3), ("t2500", 2), ("gauss", 4)])
@pytest.mark.parametrize("name", ref.SCHEDULES)
def test_a_record_is_the_statistics_of_a_column(oracle, shape, K, name):
    """Column p holds vn of the live paths and 0 from a path's depletion on; the last column is the final values; with
    below_threshold == floor == FLOOR the count below the threshold at p is the paths depleted at or before p."""
    n, P, R = ref.n_paths(shape), ref.longest(shape), 5
    a = ref.multipliers(oracle, shape, K, n, P)
    kw = dict(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name])
    if name != "fraction":  # that one is depleted by its own, high floor
        kw["floor"] = ref.FLOOR
    floor = f32(kw["floor"])
    got = ref.simulate(a, ref.WEIGHTS[K], R, columns=True, **kw)
    values, ruin = got["values"], got["ruin_period"]
    assert values.shape == (n, P + 1) and np.array_equal(_bits(values[:, P]), _bits(got["final"]))
    gone = np.cumsum(got["depleted_at"]) - got["depleted_at"][0]
    assert 0 < gone[P] < n
    for p in range(1, P + 1):
        dead = (ruin > 0) & (ruin <= p)
        assert not values[dead, p].any() and (values[~dead, p] > floor).all(), p
        st, _ = oracle.values_stats(values[:, p], float(floor), 0, 0.0, 1.0)
        assert st.count == n and st.below == int(dead.sum()) == int(gone[p]), p
    # the last column's record is the final record
    last, lh = oracle.values_stats(values[:, P], ref.BELOW, ref.BINS, ref.LO, ref.HI)
    fin, fh = oracle.values_stats(got["final"], ref.BELOW, ref.BINS, ref.LO, ref.HI)
    assert (last.count, last.below, last.underflow, last.overflow, last.min, last.max, last.sum, last.sumsq) == \
        (fin.count, fin.below, fin.underflow, fin.overflow, fin.min, fin.max, fin.sum, fin.sumsq) and np.array_equal(lh, fh)


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
        assert name in bound and len(bound[name][2]) == 8, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert not re.search(r"portfolio_cashflow_checkpoints_divide_kind", hdr + exported)  # the parent's answers for this call
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert ctypes.sizeof(_lib.PortfolioCashflowOutputs) == 56
    assert UNIT in build.SOURCES  # part of the build digest
    for name in ("simulate_portfolio_cashflow_checkpoints", "simulate_portfolio_cashflow_checkpoints_raw",
                 "simulate_portfolio_cashflow_checkpoints_to_host"):
        assert hasattr(S.Engine, name), name


def test_the_result_class():
    from stock_market_monte_carlo_amd.engine import PortfolioCashflowResult, Stats
    r = PortfolioCashflowCheckpointsResult(4, 3, depleted_at=np.array([1, 2, 0, 1], dtype=np.uint64), n_assets=2,
                                           periods=np.array([1, 3], dtype=np.uint32))
    assert isinstance(r, PortfolioCashflowResult) and np.array_equal(r.survival(), [1.0, 0.5, 0.5, 0.25])
    assert np.array_equal(r.depleted_by(), [0.5, 0.75])
    with pytest.raises(ValueError):
        PortfolioCashflowCheckpointsResult(4, 3, periods=np.array([1], dtype=np.uint32)).depleted_by()
    # fan(): two records of four values each in four buckets over [0, 4)
    mk = lambda hist: Stats(count=4, below=0, underflow=0, overflow=0, sum=0.0, sumsq=0.0, min=0.0, max=0.0,  # noqa: E731
                            hist=np.array(hist, dtype=np.uint64), hist_lo=0.0, hist_hi=4.0)
    r.checkpoints = [mk([4, 0, 0, 0]), mk([0, 0, 2, 2])]
    fan = r.fan([0.5])
    assert fan.values.shape == (2, 1) and fan.values[0, 0] == pytest.approx(0.5) and fan.values[1, 0] == pytest.approx(3.0)


def _undefined(tmp_path, unit):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    obj = str(tmp_path / (unit + ".o"))
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
    return subprocess.check_output(["nm", "-u", "-C", obj]).decode()


def test_which_unit_refers_to_which_symbols(tmp_path):
    """smmc_capi.cpp lends its checkpoint checks and calls into no feature unit; the new unit borrows from its parents and
    refers to nothing of the real-cash-flow, excursion or block-bootstrap units; the other wave-walk units gain no
    reference to a checkpoint fold through the shared run."""
    capi = _undefined(tmp_path, "smmc_capi.cpp")
    for word in ("portfolio", "cashflow", "sweep", "excursion", "blocks", "asset_table"):
        assert word not in capi, (word, capi)
    new = _undefined(tmp_path, UNIT)
    for word in ("real_cashflow", "excursion", "blocks"):
        assert word not in new, (word, new)
    for word in ("launch_portfolio_cashflow_checkpoints(", "portfolio_cashflow_checkpoints_lds_bytes(", "launch_finalize_checkpoints(",
                 "launch_finalize(", "launch_finalize_depleted(", "host_check_checkpoint_args(", "portfolio_check(", "cashflow_check_schedule(",
                 "portfolio_launch_args(", "cashflow_stage_schedule(", "host_wave_walk_grid(", "host_outputs_to_host(", "engine_ext(",
                 "smmc_engine_portfolio_cashflow_divide_kind"):
        assert word in new, word
    assert "launch_portfolio_cashflow(" not in new and "launch_checkpoints(" not in new
    for unit in ("smmc_cashflow.cpp", "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", "smmc_real_cashflow.cpp"):
        assert "checkpoint" not in _undefined(tmp_path, unit), unit
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, UNIT)).read())
    for word in ("launch_finalize", "finalize_queued", "ZeroLease", "host_timed_launch", "engine_acc_lease(", "out->reserved"):
        assert word not in code, word
    assert "host_wave_walk_run(" in code and "portfolio_cashflow_checkpoints_lds_bytes(" in code
    assert "orc_" not in code and "smmc_oracle" not in code and "_reference" not in code


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/portfolio_cashflow_checkpoints_args.cpp over the fake HIP runtime, under AddressSanitizer and UBSan:
    {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("pfcc") / "portfolio_cashflow_checkpoints_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", UNIT, "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "portfolio_cashflow_launch_stub.cpp",
                                                            "portfolio_cashflow_checkpoints_launch_stub.cpp",
                                                            "portfolio_cashflow_checkpoints_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "portfolio_cashflow_checkpoints_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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
           "five_assets": "n_assets", "weights_do_not_sum_to_one": "sum", "table_mode_without_asset_table": "set_asset_table",
           "gaussian_fields_in_table_mode": "table mode", "factor_above_diagonal": "factor[0][1]", "stream_ref": "REF",
           "stream_v2": "V2", "n_bins_above_max": "n_bins", "cashflow_null": "cf", "cashflow_struct_size_wrong": "smmc_cashflow.struct_size",
           "no_periods": "n_periods", "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS", "floor_negative": "floor",
           "amount_infinite": "amount", "amounts_entry_nan": "amounts[200]", "outputs_null": "smmc_portfolio_cashflow_outputs",
           "outputs_struct_size_wrong": "struct_size", "outputs_reserved_not_zero": "reserved", "paths_per_workgroup": "shard",
           # what smmc_engine_simulate_checkpoints refuses about the checkpoint arguments
           "periods_null": "periods is NULL", "records_null": "records pointer is NULL", "no_checkpoints": "n_checkpoints is 0",
           "too_many_checkpoints": "SMMC_MAX_CHECKPOINTS", "period_zero": "periods[1] is 0", "period_above_n_periods": "above n_periods",
           "periods_not_increasing": "strictly increasing", "periods_decreasing": "strictly increasing",
           # the two budgets
           "bucket_budget_over": "64 * 129 exceeds SMMC_MAX_CHECKPOINT_BINS", "lds_budget_over": "bytes of LDS"}
DEVICE_ONLY = {"paid_misaligned": "4-byte", "depleted_at_misaligned": "8-byte", "records_misaligned": "records pointer must be 8-byte"}


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    assert INVALID[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("case", sorted(DEVICE_ONLY))
def test_alignment_errors_of_the_device_entry(args_report, case):
    rc, text_len, launches = args_report[f"device:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0
    assert DEVICE_ONLY[case] in args_report["_text"][f"device:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_the_lds_refusal_names_both_numbers(args_report, entry):
    """4096 rows x 4 words, 4097 depletion counters, 3 x 3907 buckets (padded to 8 bytes) and four partials of 56 bytes."""
    need = (16384 + 4097 + 3 * 3907 + 1) // 2 * 2 * 4 + 4 * 56
    assert need == 129032 and need + 2048 > 128 * 1024 >= need - 8 + 2048
    text = args_report["_text"][f"{entry}:lds_budget_over"]
    assert str(need) in text and str(128 * 1024) in text, text


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", ["valid_table", "valid_gaussian", "valid_varying", "valid_no_buckets", "valid_no_parent_outputs",
                                  "bucket_budget_at", "lds_budget_at"])
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result -- the
    requests AT the two budgets among them."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_no_error_and_empty_records(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)
    assert args_report[f"empty:{entry}"] == (1, 1)  # thirty empty records with n_bins set, and the empty final record


def test_a_launch_is_given_the_form_the_parents_rule_names(args_report):
    """(return code, the launch's form, the parent's divide kind) and (n, periods[0], periods[n] == 0xffffffff)."""
    assert args_report["ran:fast"] == (-2, 0, 0) and args_report["ran:exact"] == (-2, 1, 1)
    assert args_report["ran:arguments"] == (30, 12, 1)


def test_the_partial_array_grows_with_checkpoints_times_grid(args_report):
    """One checkpoint on one workgroup, then 64 on every workgroup the engine launches, then three again: the launch stub
    writes all n x grid entries of the array it is given, under AddressSanitizer."""
    assert args_report["grow:partials"] == (-2, -2, -2, 1, 64, 3)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    """A call whose launch fails after it has counted into the three regions of the engine's accumulator queues no fold;
    the record of the next call, a plain simulate whose bucket copies span the whole accumulator, is that call's alone."""
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1, 0)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 40, 56)


# ---- the ledger and the kernels as they compile now -------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def test_the_ledger_names_exactly_the_compiled_instantiations(asm):
    import isa_table as T
    prefix, symbols = T.instantiations(asm, CM.FAMILY)
    compiled = []
    for sym in symbols:
        m = re.match(r"(I(?:L[a-z]\d+E)+E)Ev", sym[len(prefix):])
        assert m, sym
        compiled.append(m.group(1))
    ledger = [CM.mangled(c["args"]) for c in CM.ROWS]
    assert len(compiled) == len(set(compiled)) == len(ledger) == len(set(ledger)) == 48
    assert sorted(compiled) == sorted(ledger)
    assert len({c["id"] for c in CM.CASES}) == len(CM.CASES) == 50
    for c in CM.CASES:  # a row's request is the one its arguments say
        a, dense = c["args"], c["mode"] == "table" and c["T"] <= 2048
        assert a[0] == (M.MODE_GAUSSIAN if c["mode"] == "gauss" else M.MODE_TABLE) and a[2] == dense, c["id"]
        assert a[1] == (c["kind"] == M.DIV_EXACT) == (c["exact"] is not None) and a[3] == c["K"] and a[4] == c["varying"], c["id"]
        assert c["P"] == (9 if dense else 5) and c["n"] == 64 * (8 if c["mode"] == "gauss" else 4) * 2 + 37, c["id"]
        assert c["periods"][0] == 1 and c["periods"][-1] == c["P"] and list(c["periods"]) == sorted(set(c["periods"])), c["id"]
    # the parent's family is what it was
    _, parent = T.instantiations(asm, CM.PARENT)
    assert len(parent) == 48


def test_no_instantiation_uses_scratch(asm):
    """The kernels' metadata in the emitted assembly: private segment 0 for each of the 48."""
    import isa_table as T
    lines = open(asm).read().splitlines()
    prefix, symbols = T.instantiations(asm, CM.FAMILY)
    assert len(symbols) == 48
    for sym in symbols:
        sizes = [int(m.group(1)) for l in lines for m in [re.match(r"\s*\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", l)] if m]
        assert sizes == [0], (sym, sizes)


def test_the_ledgers_rows_deplete_part_of_their_paths(oracle):
    """No row is vacuous, but the twelve per-period FAST rows, which tests/feature_matrix.py confines to contributions (the
    only per-period schedules the parent's rule proves): every record of theirs holds live paths alone."""
    for c in CM.ROWS:
        want = CM.reference(oracle, c)
        share = float((want["ruin_period"] > 0).mean())
        if c["varying"] and c["kind"] == M.DIV_FAST:
            assert share == 0.0, c["id"]
        else:
            assert 0.05 < share < 0.95, (c["id"], share)
        assert want["values"].shape == (c["n"], c["P"] + 1)


# ---- the fuzz generator ---------------------------------------------------------------------------------------------------

def test_the_fuzz_generator(oracle):
    from stock_market_monte_carlo_amd import _lib
    cases = list(fuzz.cases(oracle))
    assert len(cases) == fuzz.COUNT and 20 <= fuzz.COUNT <= 30
    assert [c["periods"] for c in cases] == [c["periods"] for c in fuzz.cases(oracle)]  # seeded
    vacuous = 0
    for c in cases:
        per = c["periods"]
        assert 1 <= len(per) <= _lib.MAX_CHECKPOINTS and len(per) * c["hist"][0] <= _lib.MAX_CHECKPOINT_BINS, c["id"]
        assert list(per) == sorted(set(per)) and per[0] >= 1 and per[-1] <= c["P"], c["id"]
        assert 1 <= c["K"] <= 4 and 0 <= c["first"] <= 1 << 62 and 0 <= c["seed"] < 1 << 64, c["id"]
        vacuous += fuzz.vacuous(fuzz.reference(oracle, c))
    assert vacuous <= fuzz.COUNT // 4
    assert {c["K"] for c in cases} == {1, 2, 3, 4} and {c["mode"] for c in cases} == {"table", "gauss"}
    assert {bool(c["varying"]) for c in cases} == {False, True} and any(c["exact"] for c in cases) and any(c["hist"][0] == 0 for c in cases)
    assert any(len(c["periods"]) == 1 for c in cases) and any(len(c["periods"]) > 8 for c in cases)
    assert any(c["first"] >= 1 << 45 for c in cases)
