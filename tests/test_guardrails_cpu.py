"""The guardrails contract (include/smmc.h, smmc_engine_simulate_guardrails) without a GPU: the three identities that tie
the numpy restatement (tests/guardrails_reference.py) to restatements of calls that already exist, the proof that no case
run on the device is vacuous, the C ABI, the argument checks and staging of csrc/smmc_guardrails.cpp (tests/cpp/
guardrails_args.cpp, a stand-alone program under AddressSanitizer and UBSan) and the kernel's instantiations as compiled.

On the commit before this feature every test here fails: neither the module's subject nor the symbols exist."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cashflow_reference as cref
import guardrails_reference as G
import portfolio_cashflow_reference as pcref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_guardrails", "smmc_engine_simulate_guardrails_to_host")
f32 = np.float32
ALL_CASES = G.CASES + G.EDGES
IDS = [c["id"] for c in ALL_CASES]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _shared_equal(got, parent, tag):
    for key in G.SHARED:
        assert _same(got[key], parent[key]), (tag, key)


def _untouched(out, amount, tag):
    a0 = f32(amount)
    assert (out["amount_last"] == a0).all() and (out["amount_lowest"] == a0).all(), tag
    assert not out["cuts"].any() and not out["raises"].any() and not out["cuts_at"].any() and not out["raises_at"].any(), tag


# ---- the identities ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_identity_1_without_a_review_or_with_a_neutral_rule_it_is_the_parent_with_a_constant_amount(oracle, c):
    a, w, r = G.multipliers(oracle, c), G.weights(c), G.rule(oracle, c)
    parent = pcref.simulate(a, w, c["R"], amount=r["amount"], floor=r["floor"], capital=c["capital"])
    assert 0 < int(parent["depleted_at"][0]) < c["n"]
    never = dict(r, review_every=0)
    neutral = G.make_rule(r["amount"], c["E"], cut=1.0, raise_=1.0, index=1.0, floor=r["floor"])  # bands and clamps open
    neutral_in_bands = dict(neutral, upper=r["upper"], lower=r["lower"])  # cuts and raises happen and change nothing
    for name, rule in (("never", never), ("neutral", neutral)):
        got = G.simulate(a, w, c["R"], rule, capital=c["capital"])
        _shared_equal(got, parent, (c["id"], name))
        _untouched(got, r["amount"], (c["id"], name))
    got = G.simulate(a, w, c["R"], neutral_in_bands, capital=c["capital"])
    _shared_equal(got, parent, (c["id"], "neutral in bands"))
    assert got["cuts"].any() and got["raises"].any() and (got["amount_last"] == f32(r["amount"])).all()


@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_identity_2_with_open_bands_the_amount_is_a_schedule_and_the_call_is_the_parent_with_that_array(oracle, c):
    a, w, r = G.multipliers(oracle, c), G.weights(c), G.rule(oracle, c)
    P = c["P"]
    for E in (c["E"], 1, 3):
        rule = G.make_rule(r["amount"], E, index=1.02, cut=r["cut"], raise_=r["raise_"], floor=r["floor"])
        amounts = G.indexed_amounts(rule, P)
        passed = [sum(1 for s in range(1, t) if s % E == 0) for t in range(1, P + 1)]  # reviews before period t
        want = [f32(r["amount"])]
        for t in range(1, P):
            want.append(f32(want[-1] * f32(1.02)) if passed[t] > passed[t - 1] else want[-1])
        assert _same(amounts, np.array(want, f32)) and amounts[-1] > amounts[0]
        parent = pcref.simulate(a, w, c["R"], amounts=amounts, floor=r["floor"], capital=c["capital"])
        got = G.simulate(a, w, c["R"], rule, capital=c["capital"])
        _shared_equal(got, parent, (c["id"], E))
        assert 0 < int(parent["depleted_at"][0]) < c["n"]
        assert not got["cuts"].any() and not got["raises"].any() and (got["amount_lowest"] == f32(r["amount"])).all()
        # no review at P: a path that lives to the end leaves with the amount it took in the last period
        alive = got["ruin_period"] == 0
        assert (got["amount_last"][alive] == amounts[-1]).all(), (c["id"], E)


@pytest.mark.parametrize("c", [c for c in G.CASES if c["K"] == 1], ids=[c["id"] for c in G.CASES if c["K"] == 1])
def test_identity_3_one_asset_with_weight_one_is_the_single_series_cash_flow(oracle, c):
    a, r = G.multipliers(oracle, c), G.rule(oracle, c)
    assert a.shape[2] == 1 and G.weights(c) == (1.0,)
    rule = G.make_rule(r["amount"], c["E"], index=1.02, floor=r["floor"])
    amounts = G.indexed_amounts(rule, c["P"])
    for R in (0, c["R"]):
        got = G.simulate(a, (1.0,), R, rule, capital=c["capital"])
        final, paid, ruin, dep = cref.simulate_multipliers(a[:, :, 0], amounts, 0.0, r["floor"], c["capital"])
        assert _same(got["final"], final) and _same(got["paid"], paid) and _same(got["ruin_period"], ruin) and _same(got["depleted_at"], dep)
        assert _same(got["holdings"][0], final) and 0 < int(dep[0]) < c["n"]


# ---- no case run on the device is vacuous --------------------------------------------------------------------------

@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_every_case_cuts_raises_clamps_and_depletes_part_of_its_paths(oracle, c):
    r, out, n = G.rule(oracle, c), G.reference(oracle, c), c["n"]
    cut, raised = out["cuts"] > 0, out["raises"] > 0
    assert 0 < int(cut.sum()) < n and 0 < int(raised.sum()) < n, c["id"]
    assert (cut & raised).any(), c["id"]
    assert (out["amount_last"] == f32(r["amount_min"])).any() and f32(r["amount_min"]) < f32(r["amount"]), c["id"]
    assert 0 < int((out["ruin_period"] > 0).sum()) < n, c["id"]
    assert np.count_nonzero(out["cuts_at"]) > 1, c["id"]
    # and what the device test asserts of the counts
    assert int(out["cuts_at"].sum()) == int(out["cuts"].sum()) and int(out["raises_at"].sum()) == int(out["raises"].sum())
    assert int(out["depleted_at"].sum()) == n and out["cuts_at"][0] == 0 and out["raises_at"][0] == 0
    assert (out["amount_lowest"] <= out["amount_last"]).all() and (out["amount_lowest"] >= f32(r["amount_min"])).all()


def test_the_cases_are_the_twelve_instantiations_at_the_feature_matrix_shapes():
    assert len(G.CASES) == 12 and len({(c["mode"], c["T"], c["K"]) for c in G.CASES}) == 12
    for c in G.CASES:
        dense = c["mode"] == "table" and c["T"] <= 2048
        assert c["P"] == (9 if dense else 5) and c["n"] == 64 * (8 if c["mode"] == "gauss" else 4) * 2 + 37
        assert (c["E"], c["R"]) == ((2, 4) if dense else (2, 3))
        reviews = [t for t in range(1, c["P"]) if t % c["E"] == 0]
        assert len(reviews) >= 2 and any(t % c["R"] for t in reviews)  # more than one review, one without a rebalance
        assert any(t % c["R"] == 0 for t in reviews) == dense           # with one: at P = 9 (t = 4, 8); at P = 5 R = 3 meets no review
    # a review that falls with a rebalance in the path's partial block: the edges named so, on both table forms
    for c in (c for c in G.EDGES if c["edge"] == "partial"):
        draws = 8 if c["T"] <= 2048 else 4
        assert any(t % c["E"] == 0 and t % c["R"] == 0 and t > c["P"] // draws * draws for t in range(1, c["P"])), c["id"]
    assert G.FIRST_PATH == (1 << 32) - 100


@pytest.mark.parametrize("c", G.EDGES, ids=[c["id"] for c in G.EDGES])
def test_the_edges_are_what_their_names_say(oracle, c):
    r, out = G.rule(oracle, c), G.reference(oracle, c)
    edge = c["edge"]
    assert 0 < int((out["ruin_period"] > 0).sum()) < c["n"]
    if edge == "partial":
        assert out["cuts_at"][(c["P"] - 1) // c["E"] * c["E"]] > 0 and out["cuts"].any() and out["raises"].any()
    elif edge in ("P1", "EP", "EgtP"):  # no review ever happens
        assert {"P1": c["P"] == 1, "EP": c["E"] == c["P"], "EgtP": c["E"] > c["P"]}[edge]
        _untouched(out, r["amount"], edge)
    elif edge == "E1":
        assert c["E"] == 1 and np.count_nonzero(out["cuts_at"]) == c["P"] - 1 and out["cuts_at"][c["P"]] == 0
    else:
        assert r["amount_min"] == r["amount"] == r["amount_max"] and out["cuts"].any() and out["raises"].any()
        assert (out["amount_last"] == f32(r["amount"])).all() and (out["amount_lowest"] == f32(r["amount"])).all()


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
    assert "smmc_engine_guardrails_divide_kind" not in hdr and "guardrails_divide_kind" not in exported  # one divide, the IEEE one
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert ctypes.sizeof(_lib.Guardrails) == 44 and ctypes.sizeof(_lib.GuardrailsOutputs) == 104
    assert "smmc_guardrails.cpp" in build.SOURCES  # part of the build digest
    for name in ("simulate_guardrails", "simulate_guardrails_raw", "simulate_guardrails_to_host", "make_guardrails"):
        assert hasattr(S.Engine, name), name
    gr = S.Engine.make_guardrails(4.0)
    assert (gr.review_every, gr.upper, gr.lower, gr.amount_min, gr.amount_max, gr.index) == (12, float("inf"), 0.0, 0.0, float("inf"), 1.0)
    assert (gr.cut, gr.raise_) == (float(f32(0.9)), float(f32(1.1)))
    r = S.GuardrailsResult(4, 2, depleted_at=np.array([1, 2, 1], dtype=np.uint64), n_assets=2, cuts_at=np.array([0, 1, 2], dtype=np.uint64))
    assert isinstance(r, S.PortfolioCashflowResult) and np.array_equal(r.survival(), [1.0, 0.5, 0.25])
    assert np.array_equal(r.cut_by(), [0.0, 0.25, 0.75]) and r.amount_last is None and r.cuts is None
    with pytest.raises(ValueError):
        r.ever_cut()


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """The units that lend their checks gain no undefined symbol of the new kernel, and the new unit none of a parent's
    launch: the existing host-only programs link the former against their own launch stubs."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    units = [u for u in sorted(os.listdir(CSRC)) if u.endswith(".cpp")]
    assert "smmc_guardrails.cpp" in units
    for unit in units:
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        if unit == "smmc_guardrails.cpp":
            assert "launch_guardrails" in undefined and "guardrails_lds_bytes" in undefined
            for other in ("launch_portfolio_cashflow(", "launch_portfolio(", "launch_cashflow(", "launch_real_cashflow(", "cashflow_check_schedule"):
                assert other not in undefined, other
        else:
            assert "guardrails" not in undefined, (unit, undefined)
    text = open(os.path.join(CSRC, "smmc_guardrails.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/guardrails_args.cpp over the fake HIP runtime, a stand-alone executable under AddressSanitizer and
    UBSan: {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("guardrails") / "guardrails_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_portfolio.cpp", "smmc_guardrails.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "guardrails_launch_stub.cpp",
                                                            "guardrails_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "guardrails_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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
           "portfolio_struct_size_wrong": "struct_size", "no_assets": "n_assets", "five_assets": "n_assets", "reserved_not_zero": "reserved",
           "weight_negative": "weights[0]", "weight_nan": "weights[0]", "weight_beyond_the_assets": "weights[2]",
           "weights_do_not_sum_to_one": "sum", "table_mode_without_asset_table": "set_asset_table",
           "asset_table_of_other_width": "3 columns", "gaussian_fields_in_table_mode": "table mode", "mean_nan": "means[1]",
           "factor_above_diagonal": "factor[0][1]", "diagonal_negative": "diagonal", "stream_ref": "REF", "stream_v2": "V2",
           "n_bins_above_max": "n_bins", "unknown_mode": "mode",
           "guardrails_null": "smmc_guardrails", "guardrails_struct_size_wrong": "smmc_guardrails.struct_size", "no_periods": "n_periods",
           "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS",
           "amount_zero": "amount", "amount_negative": "amount", "amount_nan": "amount", "amount_infinite": "amount",
           "index_zero": "index", "index_infinite": "index", "index_nan": "index",
           "lower_negative": "lower", "lower_above_upper": "lower <= upper", "upper_nan": "upper", "lower_nan": "lower",
           "cut_zero": "cut", "cut_above_one": "cut", "cut_nan": "cut", "raise_below_one": "raise", "raise_infinite": "raise", "raise_nan": "raise",
           "amount_min_negative": "amount_min", "amount_min_above_amount": "amount_min", "amount_max_below_amount": "amount_max",
           "amount_min_nan": "amount_min", "amount_max_nan": "amount_max",
           "floor_negative": "floor", "floor_infinite": "floor", "floor_nan": "floor",
           "outputs_null": "smmc_guardrails_outputs", "outputs_struct_size_wrong": "struct_size", "outputs_reserved_not_zero": "reserved",
           "paths_per_workgroup": "shard", "lds_too_large": "LDS"}
DEVICE_ONLY = {"amount_last_misaligned": "4-byte", "cuts_misaligned": "4-byte", "paid_misaligned": "4-byte",
               "depleted_at_misaligned": "8-byte", "raises_at_misaligned": "8-byte"}
VALID = ["valid_table", "valid_gaussian", "valid_exact_div_flag", "valid_never_reviewed", "valid_open_bounds", "valid_shut_bounds",
         "valid_most_periods", "valid_no_outputs"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    assert INVALID[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("case", sorted(DEVICE_ONLY))
def test_misaligned_device_pointers_are_refused(args_report, case):
    rc, text_len, launches = args_report[f"device:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0
    assert DEVICE_ONLY[case] in args_report["_text"][f"device:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", VALID)
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_and_no_error(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)


def test_every_case_of_the_args_program_is_claimed(args_report):
    want = {f"{e}:{c}" for e in ("device", "to_host") for c in list(INVALID) + VALID + ["valid_no_paths"]} | {f"device:{c}" for c in DEVICE_ONLY}
    assert {k for k in args_report if k.startswith(("device:", "to_host:"))} == want


@pytest.mark.parametrize("what", ["rc", "rule", "portfolio", "sim", "per_path", "counts", "nothing_asked", "one_count_array"])
def test_the_launch_is_given_what_the_request_says(args_report, what):
    assert args_report["staged:" + what] == (1,)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 44, 104)


# ---- the kernels as they compile now --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def test_twelve_instantiations_none_with_scratch(asm):
    """(Gaussian; dense table; four-draw table) x K = 1 .. 4, one divide; private segment 0 and no scratch instruction."""
    import isa_loops as L
    import isa_table as T
    lines = open(asm).read().splitlines()
    prefix, symbols = T.instantiations(asm, "guardrails_kernel")
    got = sorted(re.match(r"(I(?:L[a-z]\d+E)+E)Ev", s[len(prefix):]).group(1) for s in symbols)
    want = sorted(f"ILi{mode}ELb{dense}ELi{K}EE" for mode, dense in ((1, 0), (0, 1), (0, 0)) for K in (1, 2, 3, 4))
    assert got == want
    for sym in symbols:
        sizes = [int(m.group(1)) for l in lines for m in [re.match(r"\s*\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", l)] if m]
        assert sizes == [0], (sym, sizes)
        assert not any(l.split()[0].startswith("scratch_") for l in L.kernel_body(lines, sym) if l.strip() and l.strip()[0] not in ";."), sym


def test_the_committed_listing_is_of_the_kernels_as_they_compile(asm):
    """profiles/guardrails/isa.txt names every instantiation with the fingerprint it has now."""
    import isa_loop_count as I
    import isa_table as T
    listing = open(os.path.join(ROOT, "profiles", "guardrails", "isa.txt")).read()
    prefix, symbols = T.instantiations(asm, "guardrails_kernel")
    for sym in symbols:
        variant = sym[len(prefix):]
        assert f"guardrails_kernel{variant}:" in listing and f"fingerprint {I.fingerprint(asm, variant, 'guardrails_kernel')[:16]}" in listing, variant
