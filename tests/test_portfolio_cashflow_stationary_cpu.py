"""Stationary-bootstrap plans (include/smmc.h, smmc_engine_simulate_portfolio_cashflow_stationary) without a GPU: the
restatement (tests/portfolio_cashflow_stationary_reference.py) against the restatements it is composed of -- probability 1
is the parent's reference, probability 0 one block of the block plan's, one asset without flows is
tests/stationary_reference.py --, the sizing of the schedules that run on the device, the proof that the edges of the row
rule occur among the device cases, the entry points declared, exported and bound, every refusal with its text, the order of
refusals, the LDS refusal and the divide rule equal to the parent's (csrc/smmc_portfolio_cashflow_stationary.cpp + the
library's other host units over tests/cpp/fake_hip.cpp, driven by tests/cpp/portfolio_cashflow_stationary_args.cpp, a
stand-alone program built with -fsanitize=address,undefined and run directly), and the kernel's 32 instantiations as
compiled: none with scratch, each within the registers of the residency DESIGN.md claims.

On the commit before this feature the tests of the feature itself fail -- the symbols, the unit and the kernel do not
exist --; the tests of the restatement alone pass there too: they test the reference."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import portfolio_cashflow_blocks_reference as B
import portfolio_cashflow_reference as pcref
import portfolio_cashflow_stationary_reference as Q
import portfolio_reference as pref
import stationary_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
UNIT = "smmc_portfolio_cashflow_stationary.cpp"
NAMES = ("smmc_engine_simulate_portfolio_cashflow_stationary", "smmc_engine_simulate_portfolio_cashflow_stationary_to_host",
         "smmc_engine_portfolio_cashflow_stationary_divide_kind")
KERNEL = "portfolio_cashflow_stationary_kernel"
# DESIGN.md, "Stationary-bootstrap plans": six waves per SIMD by registers.  512 VGPRs per lane and SIMD, allocated in
# blocks of 8: six waves get floor(512 / 6 / 8) * 8 = 80 each
MAX_VGPRS = 80
f32 = np.float32


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,K", [(37, 1), (37, 3), (2500, 2)])
def test_probability_one_is_the_parents_reference(oracle, T, K):
    """Identity 1: the same rows, so the same outputs, for every schedule, R and P."""
    shape, w = "t%d" % T, Q.WEIGHTS[K]
    assert Q.N == pcref.n_paths(shape) and Q.LONGEST == pcref.longest(shape)
    assert _same(Q.multipliers(oracle, T, K, sref.ONE), pcref.multipliers(oracle, shape, K, Q.N, Q.LONGEST))
    assert np.array_equal(Q.rows(oracle, T, Q.N, Q.LONGEST, sref.ONE), pref.row_indices(oracle, T, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST))
    for name in Q.SCHEDULES:
        for R in (0, 5):
            for P in (9, Q.LONGEST):
                kw = Q.cut(Q.schedules(oracle, T, K, w, sref.ONE)[name], P)
                got = pcref.simulate(Q.multipliers(oracle, T, K, sref.ONE, P), w, R, **kw)
                want = pcref.simulate(pcref.multipliers(oracle, shape, K, Q.N, Q.LONGEST)[:, :P], w, R, **kw)
                assert set(got) == set(want) and all(_same(got[k], want[k]) for k in want), (name, R, P)


@pytest.mark.parametrize("T,K", [(37, 3), (2500, 2), (5, 2), (1, 1)])
def test_probability_zero_is_one_block_of_the_block_plan(oracle, T, K):
    """Identity 2: one run of consecutive rows from the parent's first row, which is the block plan with L >= P."""
    for P, L in ((Q.LONGEST, Q.LONGEST), (Q.LONGEST, 64), (9, 40)):
        assert np.array_equal(Q.rows(oracle, T, Q.N, P, 0), B.rows(oracle, T, Q.N, P, L)), (P, L)
    assert _same(Q.multipliers(oracle, T, K, 0), B.multipliers(oracle, T, K, 64))


@pytest.mark.parametrize("T", [37, 2500, 5])
@pytest.mark.parametrize("q", [0, 5461, 32768, sref.ONE])
def test_one_asset_without_flows_is_the_stationary_bootstrap_of_that_column(oracle, T, q):
    """Identity 3 on the references: stationary_reference.finals_bulk (the oracle's update_fund on the same indices)."""
    column = Q.asset_table(T, 1)
    want = sref.finals_bulk(oracle, column[:, 0], Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST, q, Q.CAPITAL)
    assert np.isfinite(want).all() and (want > 0).all()
    for R in (0, 5):
        got = pcref.simulate(Q.multipliers(oracle, T, 1, q), (1.0,), R)
        assert _same(got["final"], want) and _same(got["holdings"][0], want), R
        assert not got["paid"].any() and not got["ruin_period"].any()


def _device_weights():
    for T, K in Q.TABLES + Q.FOUR_DRAW_ONCE:
        yield T, K, Q.WEIGHTS[K]
    yield Q.ZERO_WEIGHT + (Q.WEIGHTS_WITH_ZERO[Q.ZERO_WEIGHT[1]],)


@pytest.mark.parametrize("T,K,weights", [c for c in _device_weights() if c[0] != 1])
def test_the_schedules_run_on_the_device_deplete_a_good_part_of_the_paths_and_not_all(oracle, T, K, weights):
    """Every schedule at the longest P, for every renewal probability and R that run on the device.  The table of one row
    is exempt: all its paths are one path."""
    for q in Q.RENEW:
        for name in Q.SCHEDULES:
            for R in Q.REBALANCE:
                got = Q.reference(oracle, T, K, weights, R, name, Q.LONGEST, q)
                depleted = 1.0 - got["depleted_at"][0] / Q.N
                assert int(got["depleted_at"].sum()) == Q.N and 0.10 <= depleted <= 0.90, (T, K, q, name, R, depleted)
                alive = got["ruin_period"] == 0
                assert (got["final"][alive] > 0).all() and not got["final"][~alive].any() and not got["holdings"][:, ~alive].any()
        for form, kw in Q.fast_schedules(oracle, T, K, weights, q).items():
            if form == "constant":
                got = pcref.simulate(Q.multipliers(oracle, T, K, q), weights, 5, **kw)
                assert 0.10 <= 1.0 - got["depleted_at"][0] / Q.N <= 0.90, (T, K, q)


def test_every_edge_of_the_row_rule_occurs_among_the_device_cases(oracle):
    """A renewal at t = 1, a run that wraps past the last row, a run that crosses a segment boundary, a rebalance inside a
    run; tails of 1 (one candidate block of a four-draw table), 7 and none; a varying schedule whose last segment is a tail;
    both sides of every comparison of field and q."""
    for T, K in Q.TABLES:
        cases = list(Q.device_cases(T))
        assert {q for q, _, _, _ in cases} == set(Q.RENEW) and {P for _, P, _, _ in cases} == set(Q.PERIODS)
        assert {P % 8 for _, P, _, _ in cases} >= {0, 1, 7} and any(P % 8 > 4 for _, P, _, _ in cases) and any(0 < P % 8 <= 4 for _, P, _, _ in cases)
        assert any(name == "varying" and P % 8 and P > 8 for _, P, _, name in cases)
        assert {(q, name) for q, _, _, name in cases} == {(q, name) for q in Q.RENEW for name in Q.SCHEDULES}
        if T == 1:
            continue
        for q in (5461, 21845, 32768):
            cand = pref.row_indices(oracle, T, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST)
            f = sref.fields(oracle, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST)
            rows = Q.rows(oracle, T, Q.N, Q.LONGEST, q)
            renewed = f < q
            assert renewed[:, 1].any() and (~renewed[:, 1]).any()                                   # a renewal at t = 1, and none
            assert (rows[:, 1][renewed[:, 1]] == cand[:, 1][renewed[:, 1]]).all()
            on = ~renewed[:, 1:]
            assert (on & (rows[:, :-1] == T - 1) & (rows[:, 1:] == 0)).any() or T > 2048 and q > 5461  # a run wraps past the last row
            assert (~renewed[:, 8]).any() and (~renewed[:, 8] & ~renewed[:, 7] & ~renewed[:, 9]).any()  # a run crosses a segment boundary
            # a rebalance inside a run: that of R settles at the end of the 1-based period R, 0-based t = R - 1, and the
            # run that holds t = R - 1 (no renewal there) reads on at t = R (no renewal there either)
            for R in (R for R in Q.REBALANCE if R > 1):
                assert R < Q.LONGEST and (~renewed[:, R - 1] & ~renewed[:, R]).any(), (T, q, R)
        # the comparison's own edge: some field equals some q - 1 or q of a neighbouring pair is not needed -- q = 1 renews only
        # on a field of 0, q = 65535 on every field but 65535: both sides of both occur
        f = sref.fields(oracle, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST)[:, 1:]
        assert (f >= 1).any() and (f < 65535).any()
    assert any(T < 8 for T, _ in Q.TABLES) and any(T == 1 for T, _ in Q.TABLES) and any(T > 2048 for T, _ in Q.TABLES)
    assert {K for T, K in Q.TABLES + Q.FOUR_DRAW_ONCE if T > 2048} == {1, 2, 3, 4} and {K for T, K in Q.TABLES if T == 37} == {1, 2, 3, 4}
    assert Q.FIRST_PATH < (1 << 32) < Q.FIRST_PATH + Q.N and Q.N == 64 * 4 * 2 + 37


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound():
    from stock_market_monte_carlo_amd import _lib, build, stationary
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    build.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert UNIT in build.SOURCES  # part of the build digest
    for name in ("simulate_portfolio_cashflow_stationary", "simulate_portfolio_cashflow_stationary_raw",
                 "simulate_portfolio_cashflow_stationary_to_host", "portfolio_cashflow_stationary_divide_kind"):
        assert callable(getattr(stationary, name)), name
    import stock_market_monte_carlo_amd as S
    assert not any("stationary" in n for n in dir(S.Engine))  # functions of an engine: Engine gains no method


def test_the_lds_need_is_the_formula_of_smmc_internal_h():
    """[n_rows rows of 1, 2 or 4 words, ONE plain copy][n_periods + 1 depletion counters][n_bins buckets][pad to 8 bytes][one
    56-byte partial for each of the four waves], asked of the library itself; the parent's table-mode need."""
    from stock_market_monte_carlo_amd import build
    build.build()
    lib = ctypes.CDLL(build.LIB)
    fn = lib._ZN4smmc38portfolio_cashflow_geometric_lds_bytesEjjjj
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_uint32] * 4
    parent = lib._ZN4smmc28portfolio_cashflow_lds_bytesEijjjj
    parent.restype, parent.argtypes = ctypes.c_size_t, [ctypes.c_int32] + [ctypes.c_uint32] * 4
    for n_rows, K, P, bins in ((1, 1, 1, 0), (5, 2, 41, 64), (37, 3, 41, 64), (37, 4, 40, 63), (2500, 2, 360, 100), (4096, 4, 4096, 4096)):
        words = n_rows * {1: 1, 2: 2, 3: 4, 4: 4}[K] + P + 1 + bins
        assert fn(n_rows, K, P, bins) == (words + 1) // 2 * 8 + 4 * 56 == parent(0, n_rows, K, P, bins), (n_rows, K, P, bins)
    text = open(os.path.join(CSRC, UNIT)).read()
    assert text.count("portfolio_cashflow_geometric_lds_bytes(") == 1  # the need is stated once on the host side


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """The units that lend their checks gain no undefined symbol of the new kernel, and the new unit none of a parent's
    launch: the existing host-only programs link the former against their own launch stubs."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    units = [u for u in sorted(os.listdir(CSRC)) if u.endswith(".cpp")]
    assert UNIT in units
    for unit in units:
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        if unit == UNIT:
            assert "launch_portfolio_cashflow_geometric" in undefined and "portfolio_cashflow_geometric_lds_bytes" in undefined
            assert "smmc_engine_portfolio_cashflow_divide_kind" in undefined and "stationary" not in undefined  # tests/test_stationary_cpu.py
            for other in ("launch_portfolio_cashflow(", "launch_portfolio(", "launch_cashflow(", "launch_stationary(", "launch_blocks(",
                          "launch_portfolio_cashflow_blocks("):
                assert other not in undefined, other
        else:
            assert "portfolio_cashflow_geometric" not in undefined, (unit, undefined)
    text = open(os.path.join(CSRC, UNIT)).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text
    assert "host_wave_walk_run(" in text and "host_outputs_struct_to_host(" in text and "static " not in text  # no state of its own
    internal = open(os.path.join(CSRC, "smmc_internal.h")).read()
    assert "launch_portfolio_cashflow_geometric(" in internal and "stationary_check" not in internal  # nothing of the host side there


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/portfolio_cashflow_stationary_args.cpp over the fake HIP runtime, a stand-alone executable under
    AddressSanitizer and UBSan: {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("pfcfs") / "portfolio_cashflow_stationary_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp", "smmc_stationary.cpp",
                                           "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", UNIT, "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp", "stationary_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "portfolio_cashflow_launch_stub.cpp",
                                                            "portfolio_cashflow_stationary_launch_stub.cpp",
                                                            "portfolio_cashflow_stationary_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "portfolio_cashflow_stationary_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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


# case -> words its error text must hold (the texts of the units that lend the checks, unchanged)
INVALID = {"engine_null": "engine", "sim_null": "sim", "portfolio_null": "smmc_portfolio", "five_assets": "n_assets",
           "weights_do_not_sum_to_one": "sum", "table_mode_without_asset_table": "set_asset_table", "asset_table_of_other_width": "columns",
           "stream_ref": "REF", "stream_v2": "V2", "n_bins_above_max": "n_bins",
           "cashflow_null": "cf", "no_periods": "n_periods", "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS", "floor_negative": "floor",
           "fraction_nan": "fraction",
           "gaussian_mode": "the stationary bootstrap resamples the returns table: mode must be SMMC_MODE_TABLE",
           "stationary_null": "the smmc_stationary argument is NULL",
           "stationary_struct_size_wrong": "smmc_stationary.struct_size is 20, this library expects 16",
           "renew_above_one": "renew_q16 is 65537: the renewal probability renew_q16 / 65536 is at most 1",
           "renew_all_ones": "renew_q16 is 4294967295",
           "stationary_reserved0_not_zero": "smmc_stationary.reserved is {1, 0}, it must be 0",
           "stationary_reserved1_not_zero": "smmc_stationary.reserved is {0, 7}, it must be 0",
           # the order: portfolio, schedule, stationary argument (its NULL and struct_size, the mode, the stream, q, reserved)
           "order_portfolio_first": "n_assets", "order_schedule_before_stationary": "floor",
           "order_stationary_struct_before_mode": "the smmc_stationary argument is NULL", "order_portfolios_stream_before_the_mode": "portfolios support counter stream v3 only"}
CALL_ONLY = {"outputs_null": "smmc_portfolio_cashflow_outputs", "outputs_struct_size_wrong": "struct_size",
             "outputs_reserved_not_zero": "reserved", "order_stationary_before_outputs": "renew_q16", "paths_per_workgroup": "shard",
             "lds_too_small": "asset table, depletion counters and histogram need"}
DEVICE_ONLY = {"paid_misaligned": "4-byte", "depleted_at_misaligned": "8-byte"}
VALID = ["valid_table", "valid_never", "valid_always", "valid_exact_div_flag", "valid_varying", "valid_largest", "valid_no_outputs"]


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_their_text_in_their_order_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    assert INVALID[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry,case", [(e, c) for e in ("device", "to_host") for c in sorted(CALL_ONLY)]
                         + [("device", c) for c in sorted(DEVICE_ONLY)])
def test_errors_of_the_two_simulating_entries(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)
    assert {**CALL_ONLY, **DEVICE_ONLY}[case] in args_report["_text"][f"{entry}:{case}"]


def test_the_lds_refusal_names_both_numbers(args_report):
    for entry in ("device", "to_host"):
        m = re.search(r"need (\d+) bytes of LDS, device allows (\d+)", args_report["_text"][f"{entry}:lds_too_small"])
        assert m and int(m.group(1)) > (1 << 20) > int(m.group(2)) > 0


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
KINDS = {"zero_flows": FAST, "contributions": FAST, "contributions_varying": FAST, "withdrawal_floor_rebalanced": FAST,
         "withdrawal_no_floor_rebalanced": EXACT, "withdrawal_no_floor_buy_and_hold": FAST, "fraction": EXACT, "varying_withdrawals": EXACT,
         "exact_flag": EXACT}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_rule_is_the_parents_for_every_renewal_probability(args_report, case):
    for q in (0, 1, 5461, 65535, 65536):
        assert args_report[f"kind:{case}:{q}"] == (KINDS[case], KINDS[case]), (case, q)
    assert len([k for k in args_report if k.startswith("kind:")]) == 5 * len(KINDS)


def test_a_launch_is_given_the_form_the_rule_names_and_the_renewal_probability(args_report):
    assert args_report["ran:fast"] == (-2, 0, 12) and args_report["ran:exact"] == (-2, 1, 77) and args_report["ran:exact_flag"] == (-2, 1, 77)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 40, 16, 56)


# ---- the kernels as they compile now --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def test_thirty_two_instantiations_none_with_scratch_each_within_the_registers_of_six_waves(asm):
    """(exact | fast divide) x (dense | four-draw table) x K = 1 .. 4 x (constant | varying schedule); private segment 0, no
    scratch instruction, and at most MAX_VGPRS vector registers."""
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
        vgprs = [int(m.group(1)) for l in lines for m in [re.match(r"\s*\.set " + re.escape(sym) + r"\.num_vgpr, (\d+)", l)] if m]
        assert len(vgprs) == 1 and 0 < vgprs[0] <= MAX_VGPRS, (sym, vgprs)


def test_the_committed_listing_is_of_the_kernels_as_they_compile(asm):
    """profiles/portfolio_cashflow_stationary/isa.txt names every instantiation with the fingerprint it has now."""
    import isa_loop_count as I
    import isa_table as T
    listing = open(os.path.join(ROOT, "profiles", "portfolio_cashflow_stationary", "isa.txt")).read()
    prefix, symbols = T.instantiations(asm, KERNEL)
    assert len(symbols) == 32
    for sym in symbols:
        variant = sym[len(prefix):]
        assert f"{KERNEL}{variant}:" in listing and f"fingerprint {I.fingerprint(asm, variant, KERNEL)[:16]}" in listing, variant
        m = re.search(re.escape(f"{KERNEL}{variant}:") + r" vgpr (\d+) .* private_segment 0 ", listing)
        assert m and int(m.group(1)) <= MAX_VGPRS, variant
