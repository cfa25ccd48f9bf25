"""Block-bootstrap plans (include/smmc.h, smmc_engine_simulate_portfolio_cashflow_blocks) without a GPU: the restatement
(tests/portfolio_cashflow_blocks_reference.py) against the restatements it is composed of -- block length 1 is the parent's
reference, one asset without flows is tests/blocks_reference.py, a block longer than the run is one run of consecutive rows
from the parent's first row --, the sizing of the schedules that run on the device, the proof that every reviewed edge of
the kernel's row walk occurs among the device cases, the entry points declared, exported and bound, every argument error as
SMMC_ERR_INVALID with a text and without a launch and the divide rule equal to the parent's over a grid of requests
(csrc/smmc_portfolio_cashflow_blocks.cpp + the library's other host units over tests/cpp/fake_hip.cpp, driven by
tests/cpp/portfolio_cashflow_blocks_args.cpp, a stand-alone program built with -fsanitize=address,undefined and run
directly), the LDS formula of smmc_internal.h stated once more, and the kernel's 32 instantiations as compiled.

Not reachable, with the reason: "asset table with its circular extension, depletion counters and histogram beyond the
device's LDS".  The largest request the other checks let through is 5461 + 7 rows of 3 assets (padded to 4 words), 4097
depletion counters and 4096 buckets, 118 KiB with the partials; an engine assumes 128 KiB at the least and the check keeps
2 KiB back, so the refusal guards a device smaller than any the library runs on (as the parent's).

On the commit before this feature the tests of the feature itself fail -- the entry points declared, exported and bound,
the LDS formula, the new unit's symbols, everything the args program reports, the 32-row ledger and the reads of a
period --, because the symbols, the unit and the kernel do not exist; the tests of the restatement alone (the identities,
the rows, the sizing of the schedules, the edges among the device cases) pass there too: they test the reference."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import blocks_reference as bref
import portfolio_cashflow_blocks_reference as B
import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_portfolio_cashflow_blocks", "smmc_engine_simulate_portfolio_cashflow_blocks_to_host",
         "smmc_engine_portfolio_cashflow_blocks_divide_kind")
KERNEL = "portfolio_cashflow_blocks_kernel"
f32 = np.float32


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,K", [(37, 1), (37, 3), (2500, 2)])
def test_block_length_one_is_the_parents_reference(oracle, T, K):
    """The same rows, the same scale of the schedules, so the same outputs, for every schedule, R and P."""
    shape, w = "t%d" % T, B.WEIGHTS[K]
    assert B.N == pcref.n_paths(shape) and B.LONGEST == pcref.longest(shape)
    assert _same(B.multipliers(oracle, T, K, 1), pcref.multipliers(oracle, shape, K, B.N, B.LONGEST))
    for name in B.SCHEDULES:
        for R in (0, 5):
            for P in (9, B.LONGEST):
                got, want = B.reference(oracle, T, K, w, R, name, P, 1), pcref.reference(oracle, shape, K, w, R, name, P)
                assert set(got) == set(want) and all(_same(got[k], want[k]) for k in want), (name, R, P)


@pytest.mark.parametrize("T", [37, 2500, 5])
@pytest.mark.parametrize("L", [3, 12, 64])
def test_one_asset_without_flows_is_the_block_bootstrap_of_that_column(oracle, T, L):
    """Identity 2 on the references: blocks_reference.finals_bulk (the oracle's update_fund on the oracle's block starts)."""
    column = B.asset_table(T, 1)
    P = B.LONGEST
    want = bref.finals_bulk(oracle, column[:, 0], B.SEED, B.FIRST_PATH, B.N, P, L, B.CAPITAL)
    assert np.isfinite(want).all() and (want > 0).all()
    for R in (0, 5):
        got = pcref.simulate(B.multipliers(oracle, T, 1, L), (1.0,), R)
        assert _same(got["final"], want) and _same(got["holdings"][0], want), R
        assert not got["paid"].any() and not got["ruin_period"].any()


@pytest.mark.parametrize("T,K", [(37, 3), (2500, 2)])
def test_zero_flows_are_the_block_bootstrap_of_the_plain_portfolio(oracle, T, K):
    """Identity 3: there is no device sibling, the reference states it."""
    for L in (3, 12):
        a = B.multipliers(oracle, T, K, L)
        for R in (0, 5):
            values, holdings = pref.simulate(a, B.WEIGHTS[K], R)
            got = pcref.simulate(a, B.WEIGHTS[K], R)
            assert _same(got["final"], values[:, B.LONGEST]) and _same(got["holdings"], holdings), (L, R)


@pytest.mark.parametrize("T", [37, 2500, 5, 1])
def test_a_block_as_long_as_the_run_is_consecutive_rows_from_the_parents_first_row(oracle, T):
    first = pref.row_indices(oracle, T, B.SEED, B.FIRST_PATH, B.N, 1)[:, 0]
    for P, L in ((B.LONGEST, B.LONGEST), (B.LONGEST, 64), (9, 40)):
        r = B.rows(oracle, T, B.N, P, L)
        assert np.array_equal(r, (first[:, None] + np.arange(P)[None, :]) % T), (P, L)
    # and no new random numbers: the starts over P periods are the parent's rows over ceil(P / L) periods
    s = B.starts(oracle, T, B.N, 14)
    assert np.array_equal(s, pref.row_indices(oracle, T, B.SEED, B.FIRST_PATH, B.N, 14))
    assert np.array_equal(B.rows(oracle, T, B.N, B.LONGEST, 3)[:, ::3], s)


def _device_weights():
    for T, K in B.TABLES:
        yield T, K, B.WEIGHTS[K]
    yield B.ZERO_WEIGHT + (B.WEIGHTS_WITH_ZERO[B.ZERO_WEIGHT[1]],)


@pytest.mark.parametrize("T,K,weights", [c for c in _device_weights() if c[0] != 1])
def test_the_schedules_run_on_the_device_deplete_a_good_part_of_the_paths_and_not_all(oracle, T, K, weights):
    """Every schedule at the longest P, for every block length and R that run on the device.  The table of one row is
    exempt: all its paths are one path, so every schedule depletes none or all (asserted below)."""
    for L in B.BLOCK_LENS + [5]:
        for name in B.SCHEDULES:
            for R in B.REBALANCE:
                got = B.reference(oracle, T, K, weights, R, name, B.LONGEST, L)
                depleted = 1.0 - got["depleted_at"][0] / B.N
                assert int(got["depleted_at"].sum()) == B.N and 0.10 <= depleted <= 0.90, (T, K, L, name, R, depleted)
                alive = got["ruin_period"] == 0
                assert (got["final"][alive] > 0).all() and not got["final"][~alive].any() and not got["holdings"][:, ~alive].any()


def test_the_table_of_one_row_has_one_path(oracle):
    for L in (1, 9):
        for name in B.SCHEDULES:
            got = B.reference(oracle, 1, 1, (1.0,), 5, name, B.LONGEST, L)
            assert len(set(got["final"].tolist())) == 1 and int(got["depleted_at"].max()) == B.N


def test_every_reviewed_edge_of_the_row_walk_occurs_among_the_device_cases(oracle):
    """A tail segment (a block's last 1 .. 7 periods), a block cut by P, n_rows < 8, L > n_rows, a wrap past the table's end
    inside a segment and between segments, a segment that begins off a multiple of 8 with a varying schedule, and a rebalance
    inside a block and on a block's boundary."""
    for T, K in B.TABLES:
        cases = list(B.device_cases(T))
        assert any(L % 8 in range(1, 8) and P >= L for L, P, R, _ in cases)                      # the tail of a whole block
        assert {L % 8 for L, P, R, _ in cases if P >= L} >= {0, 1, 3, 4}                         # tails of 1, 3, 4; none
        assert any(P > L and P % L for L, P, R, _ in cases)                                      # the last block cut by P
        assert any(L > P for L, P, R, _ in cases) and (T > 64 or any(L > T for L, P, R, _ in cases))  # L > n_rows: the short tables
        assert any(name == "varying" and L % 8 and P > L for L, P, R, name in cases)             # schedule read off a multiple of 8
        assert any(R and L > R and any(t % R == 0 and t % L for t in range(1, P)) for L, P, R, _ in cases)       # inside a block
        assert any(R and any(t % R == 0 and t % L == 0 for t in range(1, P)) for L, P, R, _ in cases)            # on a boundary
        assert (12, B.LONGEST, 12, "amount") in cases and (5, B.LONGEST, 12, "varying") in cases
        # the wrap: some path's run passes the table's last row inside its first segment, and, for a block of more than
        # 8 periods, in a later one
        for L in (9, 40):
            s = B.starts(oracle, T, B.N, -(-B.LONGEST // L))
            assert (s + min(L, 8) - 1 >= T).any() and (s < T).all(), (T, L)
            assert (s + 8 >= T).any(), (T, L)                                  # the address wraps between two segments
        assert T > 64 or (((B.starts(oracle, T, B.N, 2) + 8) % T + 7) >= T).any(), T   # L = 40: and inside a later segment
    assert any(T < 8 for T, _ in B.TABLES) and any(T == 1 for T, _ in B.TABLES) and any(T > 2048 for T, _ in B.TABLES)
    assert B.FIRST_PATH < (1 << 32) < B.FIRST_PATH + B.N and B.N == 64 * 4 * 2 + 37


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
    assert ctypes.sizeof(_lib.PortfolioCashflowOutputs) == 56 and ctypes.sizeof(_lib.Cashflow) == 40 and ctypes.sizeof(_lib.Blocks) == 16
    assert "smmc_portfolio_cashflow_blocks.cpp" in build.SOURCES  # part of the build digest
    for name in ("simulate_portfolio_cashflow_blocks", "simulate_portfolio_cashflow_blocks_raw", "simulate_portfolio_cashflow_blocks_to_host",
                 "portfolio_cashflow_blocks_divide_kind"):
        assert hasattr(S.Engine, name), name


def test_the_lds_need_is_the_formula_of_smmc_internal_h():
    """[(n_rows + 7) rows of 1, 2 or 4 words][n_periods + 1 depletion counters][n_bins buckets][pad to 8 bytes][one 56-byte
    partial for each of the four waves], asked of the library itself (a host function of the kernels' unit)."""
    from stock_market_monte_carlo_amd import build
    build.build()
    lib = ctypes.CDLL(build.LIB)
    fn = lib._ZN4smmc35portfolio_cashflow_blocks_lds_bytesEjjjj
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_uint32] * 4
    text = open(os.path.join(CSRC, "smmc_internal.h")).read()
    assert re.search(r"portfolio_cashflow_blocks_rows\(uint32_t n_rows\) \{ return n_rows \+ 7u; \}", text)
    for n_rows, K, P, bins in ((1, 1, 1, 0), (5, 2, 41, 64), (37, 3, 41, 64), (37, 4, 40, 63), (2500, 2, 360, 100), (4096, 4, 4096, 4096)):
        words = (n_rows + 7) * {1: 1, 2: 2, 3: 4, 4: 4}[K] + P + 1 + bins
        assert fn(n_rows, K, P, bins) == (words + 1) // 2 * 8 + 4 * 56, (n_rows, K, P, bins)


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """The units that lend their checks gain no undefined symbol of the new kernel, and the new unit none of a parent's
    launch: the existing host-only programs link the former against their own launch stubs."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    units = [u for u in sorted(os.listdir(CSRC)) if u.endswith(".cpp")]
    assert "smmc_portfolio_cashflow_blocks.cpp" in units
    for unit in units:
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        if unit == "smmc_portfolio_cashflow_blocks.cpp":
            assert "launch_portfolio_cashflow_blocks" in undefined and "portfolio_cashflow_blocks_lds_bytes" in undefined
            assert "blocks_check" in undefined and "smmc_engine_portfolio_cashflow_divide_kind" in undefined
            for other in ("launch_portfolio_cashflow(", "launch_portfolio(", "launch_cashflow(", "launch_blocks("):
                assert other not in undefined, other
        else:
            assert "portfolio_cashflow_blocks" not in undefined, (unit, undefined)
    text = open(os.path.join(CSRC, "smmc_portfolio_cashflow_blocks.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text
    assert "host_wave_walk_run(" in text and "host_outputs_struct_to_host(" in text and "static " not in text  # no state of its own


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/portfolio_cashflow_blocks_args.cpp over the fake HIP runtime, a stand-alone executable under
    AddressSanitizer and UBSan: {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("pfcfb") / "portfolio_cashflow_blocks_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", "smmc_portfolio_cashflow_blocks.cpp",
                                           "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "portfolio_cashflow_launch_stub.cpp",
                                                            "portfolio_cashflow_blocks_launch_stub.cpp",
                                                            "portfolio_cashflow_blocks_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "portfolio_cashflow_blocks_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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
           "gaussian_fields_in_table_mode": "table mode", "mean_nan": "means[1]", "factor_above_diagonal": "factor[0][1]",
           "diagonal_negative": "diagonal", "stream_ref": "REF", "stream_v2": "V2", "n_bins_above_max": "n_bins",
           "histogram_range_empty": "histogram", "unknown_mode": "mode",
           "cashflow_null": "cf", "cashflow_struct_size_wrong": "smmc_cashflow.struct_size", "no_periods": "n_periods",
           "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS", "floor_negative": "floor", "floor_nan": "floor",
           "amount_infinite": "amount", "fraction_nan": "fraction", "amounts_entry_nan": "amounts[200]",
           "fractions_entry_infinite": "fractions[359]",
           "gaussian_mode": "SMMC_MODE_TABLE", "blocks_null": "smmc_blocks", "blocks_struct_size_wrong": "smmc_blocks.struct_size",
           "block_len_zero": "block_len", "blocks_kind_unknown": "SMMC_BLOCKS_CIRCULAR", "blocks_reserved_not_zero": "smmc_blocks.reserved"}
CALL_ONLY = {"outputs_null": "smmc_portfolio_cashflow_outputs", "outputs_struct_size_wrong": "struct_size",
             "outputs_reserved_not_zero": "reserved", "paths_per_workgroup": "shard"}
DEVICE_ONLY = {"paid_misaligned": "4-byte", "depleted_at_misaligned": "8-byte"}
VALID = ["valid_table", "valid_block_len_one", "valid_block_len_largest", "valid_exact_div_flag", "valid_buy_and_hold", "valid_varying",
         "valid_largest", "valid_no_outputs"]


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
@pytest.mark.parametrize("case", VALID)
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result; the one
    launch is this kernel's, never the parent's."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_and_no_error(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)


def test_every_case_of_the_args_program_is_claimed(args_report):
    want = {f"{e}:{c}" for e in ("device", "to_host", "divide_kind") for c in INVALID}
    want |= {f"{e}:{c}" for e in ("device", "to_host") for c in list(CALL_ONLY) + VALID + ["valid_no_paths"]}
    want |= {f"device:{c}" for c in DEVICE_ONLY}
    assert {k for k in args_report if k.startswith(("device:", "to_host:", "divide_kind:"))} == want


FAST, EXACT = 0, 1
KINDS = {"zero_flows": FAST, "contributions": FAST, "contributions_varying": FAST, "contributions_too_large": EXACT,
         "withdrawal_floor_rebalanced": FAST, "withdrawal_no_floor_rebalanced": EXACT, "withdrawal_no_floor_buy_and_hold": FAST,
         "withdrawal_tiny_floor": EXACT, "fraction": EXACT, "varying_withdrawals": EXACT, "exact_flag": EXACT,
         "table_doubling_360": EXACT, "table_doubling_36": FAST}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_rule_is_the_parents_for_every_block_length(args_report, case):
    for L in (1, 3, 12, 360, 5000):
        assert args_report[f"kind:{case}:{L}"] == (KINDS[case], KINDS[case]), (case, L)
    assert len([k for k in args_report if k.startswith("kind:")]) == 5 * len(KINDS)


def test_a_launch_is_given_the_form_the_rule_names_and_the_block_length(args_report):
    assert args_report["ran:fast"] == (-2, 0, 12) and args_report["ran:exact"] == (-2, 1, 77) and args_report["ran:exact_flag"] == (-2, 1, 77)


@pytest.mark.parametrize("what", ["rc", "plan", "sim", "outputs", "nothing_asked"])
def test_the_launch_is_given_what_the_request_says(args_report, what):
    assert args_report["staged:" + what] == (1,)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 40, 16, 56)


# ---- the kernels as they compile now --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def test_thirty_two_instantiations_none_with_scratch(asm):
    """(exact | fast divide) x (dense | four-draw table) x K = 1 .. 4 x (constant | varying schedule); private segment 0 and
    no scratch instruction."""
    import isa_loops as L
    import isa_table as T
    lines = open(asm).read().splitlines()
    prefix, symbols = T.instantiations(asm, KERNEL)
    got = sorted(re.match(r"(I(?:L[a-z]\d+E)+E)Ev", s[len(prefix):]).group(1) for s in symbols)
    want = sorted(f"ILb{x}ELb{d}ELi{K}ELb{v}EE" for x in (0, 1) for d in (0, 1) for K in (1, 2, 3, 4) for v in (0, 1))
    assert got == want and len(got) == 32
    for sym in symbols:
        sizes = [int(m.group(1)) for l in lines for m in [re.match(r"\s*\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", l)] if m]
        assert sizes == [0], (sym, sizes)
        assert not any(l.split()[0].startswith("scratch_") for l in L.kernel_body(lines, sym) if l.strip() and l.strip()[0] not in ";."), sym


def test_a_period_reads_its_row_with_one_lds_read_at_a_constant_offset(asm):
    """The segment's eight reads and the tail's seven: ds_read_b32 / b64 / b128 for K = 1, 2, 3 .. 4, the period in the
    offset field (multiples of the row's bytes up to seven rows)."""
    import isa_loops as L
    lines = open(asm).read().splitlines()
    for K, op, row in ((1, "ds_read_b32", 4), (2, "ds_read_b64", 8), (3, "ds_read_b128", 16), (4, "ds_read_b128", 16)):
        body = L.kernel_body(lines, f"{KERNEL}ILb1ELb1ELi{K}ELb0EE")
        reads = [l for l in body if l.split() and l.split()[0] in (op, op.replace("_b32", "2_b32"))]
        offsets = {int(m.group(1)) for l in reads for m in [re.search(r"offset:(\d+)", l)] if m}
        assert offsets >= {row * j for j in range(1, 8)} or (K == 1 and any("ds_read2_b32" in l for l in reads)), (K, sorted(offsets))
        assert len(reads) >= 8, (K, len(reads))


def test_the_committed_listing_is_of_the_kernels_as_they_compile(asm):
    """profiles/portfolio_cashflow_blocks/isa.txt names every instantiation with the fingerprint it has now."""
    import isa_loop_count as I
    import isa_table as T
    listing = open(os.path.join(ROOT, "profiles", "portfolio_cashflow_blocks", "isa.txt")).read()
    prefix, symbols = T.instantiations(asm, KERNEL)
    assert len(symbols) == 32
    for sym in symbols:
        variant = sym[len(prefix):]
        assert f"{KERNEL}{variant}:" in listing and f"fingerprint {I.fingerprint(asm, variant, KERNEL)[:16]}" in listing, variant
        assert re.search(re.escape(f"{KERNEL}{variant}:") + r".* private_segment 0 ", listing), variant
