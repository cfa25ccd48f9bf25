"""Real cash flows without a GPU: the restatement of the contract (tests/real_cashflow_reference.py) against the one it
must agree with -- tests/portfolio_cashflow_reference.py through the three identities of include/smmc.h --, what
inflation changes, its prefix property, the sizing of the schedules that run on the device; the entry points declared,
exported and bound; every argument error include/smmc.h lists as SMMC_ERR_INVALID with a text and without a launch, from
all three entries, the divide rule's answers and the accumulator lease after a failed launch (csrc/smmc_real_cashflow.cpp
+ the library's other host units over tests/cpp/fake_hip.cpp, driven by tests/cpp/real_cashflow_args.cpp, built with
-fsanitize=address,undefined and run directly); the ledger of tests/real_cashflow_matrix.py against the kernels as they
compile now, and no scratch in any of them.

The issue behind the feature counts 48 instantiations for K = 1 .. 3; three rungs of the mode ladder x two divides x
three K x two schedule forms are 36, and 36 are compiled and listed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import feature_matrix as M
import portfolio_cashflow_reference as pcref
import real_cashflow_matrix as RM
import real_cashflow_reference as ref
from stock_market_monte_carlo_amd._lib import RealCashflowOutputs  # noqa: F401  without the feature the module has no subject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_real_cashflow", "smmc_engine_simulate_real_cashflow_to_host", "smmc_engine_real_cashflow_divide_kind")
NOMINAL = ("final", "holdings", "paid", "ruin_period", "depleted_at")
f32 = np.float32


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _nominal_equal(got, want, tag):
    for key in NOMINAL:
        assert _same(got[key], want[key]), (tag, key)


# ---- the restatement: the three identities ----------------------------------------------------------------------------

@pytest.mark.parametrize("shape,K", ref.SHAPES)
@pytest.mark.parametrize("name", ref.SCHEDULES)
def test_identity_1_zero_inflation_is_the_parent_on_the_first_k_series(oracle, shape, K, name):
    """A multiplier of exactly 100 (a column of zeros; mean 0 and a zero row of the factor) keeps I at 1."""
    n, P = ref.n_paths(shape), ref.longest(shape)
    a = ref.multipliers(oracle, shape, K, n, P).copy()
    a[:, :, K] = f32(100.0)
    kw = ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name]
    for R in (0, 5):
        got, want = ref.simulate(a, ref.WEIGHTS[K], R, **kw), pcref.simulate(a[:, :, :K], ref.WEIGHTS[K], R, **kw)
        assert 0 < want["depleted_at"][0] < n
        _nominal_equal(got, want, (shape, K, name, R))
        assert _same(got["final_real"], got["final"]) and (got["index"] == 1.0).all()


@pytest.mark.parametrize("shape,K", ref.SHAPES)
def test_identity_2_without_amount_and_floor_the_nominal_outputs_are_the_parents(oracle, shape, K):
    n, P = ref.n_paths(shape), ref.longest(shape)
    a = ref.multipliers(oracle, shape, K, n, P)
    frac = np.where(np.arange(P) % 3 == 0, 0.0, 0.02).astype(f32)
    for R, kw in ((0, dict(fraction=0.03)), (5, dict(fractions=frac)), (12, {})):
        got, want = ref.simulate(a, ref.WEIGHTS[K], R, **kw), pcref.simulate(a[:, :, :K], ref.WEIGHTS[K], R, **kw)
        _nominal_equal(got, want, (shape, K, R))
        assert not _same(got["final_real"], got["final"]) and np.unique(got["index"]).size > n // 2


@pytest.mark.parametrize("T,K", [(37, 1), (37, 3), (2500, 2)])
def test_identity_3_a_constant_inflation_column_is_the_parents_amounts_array(oracle, T, K):
    """0.3 % every month: one sequence I_t, and the parent with amounts[t - 1] = fl(amount * I_t) and floor 0."""
    shape = "t%d" % T
    n, P = ref.n_paths(shape), ref.longest(shape)
    a = ref.multipliers(oracle, shape, K, n, P).copy()
    a[:, :, K] = f32(100.0) + f32(0.3)
    index = np.ones(P + 1, f32)
    for t in range(1, P + 1):
        index[t] = (index[t - 1] * (f32(100.0) + f32(0.3))) / f32(100.0)
    amount = f32(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])["amount"]["amount"])
    for R in (0, 5):
        got = ref.simulate(a, ref.WEIGHTS[K], R, amount=amount, fraction=0.001)
        want = pcref.simulate(a[:, :, :K], ref.WEIGHTS[K], R, amounts=(amount * index[1:]).astype(f32), fraction=0.001)
        assert 0 < want["depleted_at"][0] < n
        _nominal_equal(got, want, (shape, K, R))
        assert (got["index"] == index[P]).all() and index[P] > 1.1


@pytest.mark.parametrize("shape,K", ref.SHAPES)
def test_with_the_modules_inflation_a_real_amount_differs_from_a_nominal_one_and_depletes_more_paths(oracle, shape, K):
    n, P = ref.n_paths(shape), ref.longest(shape)
    a = ref.multipliers(oracle, shape, K, n, P)
    kw = ref.schedules(oracle, shape, K, ref.WEIGHTS[K])["amount"]
    real, nominal = ref.simulate(a, ref.WEIGHTS[K], 5, **kw), pcref.simulate(a[:, :, :K], ref.WEIGHTS[K], 5, **kw)
    assert not _same(real["final"], nominal["final"])
    assert (real["ruin_period"] > 0).sum() > (nominal["ruin_period"] > 0).sum()
    assert 1.0 < float(np.median(real["index"])) < 1.5 and (real["index"] < np.median(real["index"])).any()
    inflation = a[:, :, K] - f32(100.0)
    assert (inflation < 0).any() and 0.1 < float(inflation.mean()) < 0.5                      # sometimes negative, around 0.25 %
    assert abs(np.corrcoef(inflation.ravel(), a[:, :, 0].ravel())[0, 1]) > 0.05               # and correlated with the assets


@pytest.mark.parametrize("shape,K", ref.SHAPES)
def test_the_schedules_run_on_the_device_deplete_a_good_part_of_the_paths_and_not_all(oracle, shape, K):
    n, P, weights = ref.n_paths(shape), ref.longest(shape), ref.WEIGHTS[K]
    for name in ref.SCHEDULES:
        for R in ref.REBALANCE:
            got = ref.reference(oracle, shape, K, weights, R, name, P)
            depleted = 1.0 - got["depleted_at"][0] / n
            assert int(got["depleted_at"].sum()) == n and 0.10 <= depleted <= 0.90, (shape, K, name, R, depleted)
            alive = got["ruin_period"] == 0
            assert (got["final"][alive] > 0).all() and not got["final"][~alive].any() and not got["holdings"][:, ~alive].any()
            assert (got["final_real"][alive] > 0).all() and not got["final_real"][~alive].any()
            assert np.isfinite(got["index"]).all() and (got["index"] > 0.5).all()
    kw = ref.schedules(oracle, shape, K, weights)["varying"]
    assert (kw["amounts"][:10] < 0).all() and (kw["amounts"][10:] > 0).all()  # contributions first, then withdrawals


@pytest.mark.parametrize("shape,K", [("t37", 3), ("gauss", 2)])
@pytest.mark.parametrize("name", ["amount", "varying"])
def test_the_real_final_value_does_not_depend_on_n_periods(oracle, shape, K, name):
    """Columns p of the longest run give the outputs of a run of p periods (whose last period never rebalances)."""
    n, P, R = 70, ref.longest(shape), 5
    a = ref.multipliers(oracle, shape, K, ref.n_paths(shape), P)[:n]
    kw = ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name]
    long = ref.simulate(a, ref.WEIGHTS[K], R, columns=True, **kw)
    for p in range(1, P + 1):
        short = ref.simulate(a[:, :p], ref.WEIGHTS[K], R, **ref.cut(kw, p))
        assert _same(short["final"], long["values"][:, p].copy()) and _same(short["index"], long["indices"][:, p].copy()), p
        assert _same(short["final_real"], long["values"][:, p] / long["indices"][:, p]), p
        assert np.array_equal(short["ruin_period"], np.where(long["ruin_period"] <= p, long["ruin_period"], 0)), p


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
    assert ctypes.sizeof(_lib.RealCashflowOutputs) == 72
    assert "smmc_real_cashflow.cpp" in build.SOURCES  # part of the build digest
    for name in ("simulate_real_cashflow", "simulate_real_cashflow_raw", "simulate_real_cashflow_to_host", "real_cashflow_divide_kind",
                 "make_real_cashflow_outputs"):
        assert hasattr(S.Engine, name), name
    r = S.RealCashflowResult(4, 2, depleted_at=np.array([1, 2, 1], dtype=np.uint64), n_assets=2)
    assert np.array_equal(r.survival(), [1.0, 0.5, 0.25]) and r.final_real is None and r.index is None
    pf = S.Engine.make_real_portfolio((0.6, 0.4), 12, means=(0.5, 0.2, 0.25), factor=np.tril(np.ones((3, 3))))
    assert pf.n_assets == 2 and pf.weights[2] == 0.0 and pf.means[2] == 0.25 and pf.factor[2 * _lib.MAX_ASSETS + 2] == 1.0
    with pytest.raises(ValueError):
        S.Engine.make_real_portfolio((0.25, 0.25, 0.25, 0.25))


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """The units that lend their checks gain no undefined symbol of the new kernel: the existing host-only programs link
    them against their own launch stubs."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    units = [u for u in sorted(os.listdir(CSRC)) if u.endswith(".cpp")]
    assert "smmc_real_cashflow.cpp" in units
    for unit in units:
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        if unit == "smmc_real_cashflow.cpp":
            assert "launch_real_cashflow" in undefined
            assert "launch_portfolio_cashflow(" not in undefined and "launch_portfolio(" not in undefined and "launch_cashflow(" not in undefined
        else:
            assert "real_cashflow" not in undefined, (unit, undefined)


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/real_cashflow_args.cpp over the fake HIP runtime, a stand-alone executable under AddressSanitizer and
    UBSan: {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("real") / "real_cashflow_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_portfolio.cpp", "smmc_real_cashflow.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "portfolio_cashflow_launch_stub.cpp",
                                                            "real_cashflow_launch_stub.cpp", "real_cashflow_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "real_cashflow_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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


# case -> a word its error text must hold; the parent's refusals are made at the law's width, K + 1 = 3
INVALID = {"engine_null": "engine", "sim_null": "sim", "sim_struct_size_wrong": "struct_size", "portfolio_null": "smmc_portfolio",
           "portfolio_struct_size_wrong": "struct_size", "no_assets": "n_assets", "five_assets": "n_assets",
           "four_assets_leave_no_series_for_inflation": "SMMC_MAX_ASSETS - 1", "inflation_weighted": "weights[2]",
           "inflation_weighted_table": "weights[2]",
           "reserved_not_zero": "reserved", "weight_negative": "weights[0]", "weight_nan": "weights[0]",
           "weight_infinite": "weights[1]", "weight_beyond_the_law": "weights[3]", "weights_do_not_sum_to_one": "sum",
           "table_mode_without_asset_table": "set_asset_table", "asset_table_of_the_assets_alone": "2 columns",
           "asset_table_of_other_width": "4 columns",
           "gaussian_fields_in_table_mode": "table mode", "mean_nan": "means[1]", "factor_infinite": "factor[1][0]",
           "factor_above_diagonal": "factor[0][1]", "factor_beyond_the_law": "factor[3][3]", "mean_beyond_the_law": "means[3]",
           "diagonal_negative": "diagonal", "stream_ref": "REF", "stream_v2": "V2", "n_bins_above_max": "n_bins",
           "histogram_range_empty": "histogram", "unknown_mode": "mode",
           "cashflow_null": "cf", "cashflow_struct_size_wrong": "smmc_cashflow.struct_size", "no_periods": "n_periods",
           "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS", "floor_negative": "floor", "floor_nan": "floor",
           "amount_infinite": "amount", "fraction_nan": "fraction", "amounts_entry_nan": "amounts[200]",
           "fractions_entry_infinite": "fractions[359]"}
CALL_ONLY = {"outputs_null": "smmc_real_cashflow_outputs", "outputs_struct_size_wrong": "struct_size",
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
@pytest.mark.parametrize("case", ["valid_table", "valid_gaussian", "valid_buy_and_hold", "valid_no_inflation", "valid_varying",
                                  "valid_largest", "valid_no_outputs"])
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_and_no_error(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)


FAST, EXACT = 0, 1
KINDS = {
    # both conditions hold: the index inside its window, contributions only
    "zero_flows_table": FAST, "contributions_table": FAST, "contributions_floor_table": FAST, "contributions_varying_table": FAST,
    "contributions_varying_zero_fractions": FAST, "contributions_gaussian_36": FAST, "contributions_zero_weight": FAST,
    "inflation_doubling_36": FAST, "inflation_halving_36": FAST, "contributions_large_tame_inflation": FAST, "table_doubling_36": FAST,
    # the holdings' bounds fail, as in the parent
    "contributions_gaussian_360": EXACT, "contributions_too_large": EXACT, "contributions_tiny_weight": EXACT,
    "table_doubling_360": EXACT, "gaussian_may_go_negative": EXACT, "no_capital": EXACT,
    # the index may leave its window, or raises the contributions past the upper bound
    "inflation_doubling_360": EXACT, "inflation_halving_360": EXACT, "inflation_may_go_negative": EXACT,
    "contributions_inflated_too_large": EXACT,
    # anything that takes money out, the parent's "one constant amount" included: the nominal amount varies
    "one_withdrawal_among_contributions": EXACT, "withdrawal_floor_rebalanced": EXACT, "withdrawal_floor_gaussian_36": EXACT,
    "withdrawal_no_floor_buy_and_hold": EXACT, "fraction": EXACT, "contribution_and_fraction": EXACT, "varying_withdrawals": EXACT,
    "exact_flag": EXACT}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_rule(args_report, case):
    """The fast divide only where the header's rule proves every product inside its domain; never the checked form."""
    assert args_report["kind:" + case] == (KINDS[case],)


def test_every_divide_case_of_the_args_program_is_claimed(args_report):
    assert {k[5:] for k in args_report if k.startswith("kind:")} == set(KINDS)


def test_a_launch_is_given_the_form_the_rule_names(args_report):
    assert args_report["ran:fast"] == (-2, 0) and args_report["ran:exact"] == (-2, 1)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 40, 72)


def test_the_product_does_not_touch_the_oracle():
    text = open(os.path.join(CSRC, "smmc_real_cashflow.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text


# ---- the ledger and the kernels as they compile now -------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def _symbols(asm):
    import isa_table as T
    return T.instantiations(asm, RM.FAMILY)


def test_the_ledger_names_exactly_the_compiled_instantiations(asm):
    prefix, symbols = _symbols(asm)
    compiled = []
    for sym in symbols:
        m = re.match(r"(I(?:L[a-z]\d+E)+E)Ev", sym[len(prefix):])
        assert m, sym
        compiled.append(m.group(1))
    ledger = [RM.mangled(c["args"]) for c in RM.ROWS]
    assert len(compiled) == len(set(compiled)) == len(ledger) == len(set(ledger)) == 36
    assert sorted(compiled) == sorted(ledger)
    assert len({c["id"] for c in RM.CASES}) == len(RM.CASES) == 38
    for c in RM.CASES:  # a row's case is the one its arguments say
        a, dense = c["args"], c["mode"] == "table" and c["T"] <= 2048
        assert a[0] == (M.MODE_GAUSSIAN if c["mode"] == "gauss" else M.MODE_TABLE) and a[2] == dense, c["id"]
        assert a[1] == (c["kind"] == M.DIV_EXACT) == (c["exact"] is not None) and a[3] == c["K"] and a[4] == c["varying"], c["id"]
        assert c["P"] == (9 if dense else 5) and c["n"] == 64 * (8 if c["mode"] == "gauss" else 4) * 2 + 37, c["id"]


def test_no_instantiation_uses_scratch(asm):
    """The kernel metadata of the emitted assembly: private segment 0, and no scratch instruction in any body."""
    import isa_loops as L
    lines = open(asm).read().splitlines()
    prefix, symbols = _symbols(asm)
    assert len(symbols) == 36
    for sym in symbols:
        sizes = [int(m.group(1)) for l in lines for m in [re.match(r"\s*\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", l)] if m]
        assert sizes == [0], (sym, sizes)
        assert not any(l.split()[0].startswith("scratch_") for l in L.kernel_body(lines, sym) if l.strip() and l.strip()[0] not in ";."), sym
    meta = [l for l in lines if ".private_segment_fixed_size:" in l]
    names = [l for l in lines if re.match(r"\s*\.name:\s+" + re.escape(prefix), l)]
    assert len(names) == 36 and len(meta) >= 36


def test_the_ledgers_rows_deplete_part_of_their_paths(oracle):
    """No row is vacuous: the FAST rows, confined to contributions, are depleted by their floor."""
    for c in RM.ROWS:
        want = RM.reference(oracle, c)
        share = float((want["ruin_period"] > 0).mean())
        assert 0.05 < share < 0.95, (c["id"], share)
        if c["kind"] == M.DIV_FAST:
            sched = want["args"][1]
            assert (np.asarray(sched.get("amounts", sched.get("amount"))) <= 0).all() and not np.asarray(sched.get("fractions", sched.get("fraction"))).any()
        assert np.isfinite(want["index"]).all() and (want["index"] > 0).all()


@pytest.mark.parametrize("c", RM.EXTREME, ids=[c["id"] for c in RM.EXTREME])
def test_extreme_rows_tell_the_divides_apart(oracle, c):
    """Part of the paths, not all, form a product outside the fast divide's domain, and for some the restated fast divide
    gives other bits than the IEEE quotient (tests/feature_matrix.py: fast_div100); the index stays tame."""
    x = RM.asset_products(oracle, c)
    with np.errstate(all="ignore"):
        left = (((np.abs(x) < f32(M.TINY)) & (x != 0)) | ~np.isfinite(x)).any(axis=1)
        q, fq = x / f32(100.0), M.fast_div100(x)
    differs = ((q.view(np.uint32) != fq.view(np.uint32)) & ~(np.isnan(q) & np.isnan(fq))).any(axis=1)
    assert 0 < left.mean() < 1 and differs.any() and not (differs & ~left).any()
    want = RM.reference(oracle, c)
    assert np.isfinite(want["index"]).all() and (want["index"] > 0.5).all()
