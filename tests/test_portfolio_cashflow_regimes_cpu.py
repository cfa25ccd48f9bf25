"""Regime-switching plans (include/smmc.h, smmc_engine_simulate_portfolio_cashflow_regimes) without a GPU: the restatement
(tests/portfolio_cashflow_regimes_reference.py) against the restatements it is composed of -- equal regimes and a regime
never left are the parent's reference, one asset without flows is tests/regimes_reference.py, a shorter run is a prefix --,
the sizing of the schedules that run on the device, the entry points declared, exported and bound, make_portfolio_regimes,
the launch symbol confined to its unit, every refusal with its text from all three entries and the divide rule on the
union of the regimes' bounds (csrc/smmc_portfolio_cashflow_regimes.cpp + the library's other host units over
tests/cpp/fake_hip.cpp, driven by tests/cpp/portfolio_cashflow_regimes_args.cpp, a stand-alone program built with
-fsanitize=address,undefined and run directly), and the kernel's 16 instantiations as compiled: none with scratch, the
parents' lists unchanged.

On the commit before this feature the tests of the feature itself fail -- the symbols, the unit and the kernel do not
exist --; the tests of the restatement alone pass there too: they test the reference."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import portfolio_cashflow_reference as pcref
import portfolio_cashflow_regimes_reference as Q
import portfolio_reference as pref
import regimes_reference as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
UNIT = "smmc_portfolio_cashflow_regimes.cpp"
NAMES = ("smmc_engine_simulate_portfolio_cashflow_regimes", "smmc_engine_simulate_portfolio_cashflow_regimes_to_host",
         "smmc_engine_portfolio_cashflow_regimes_divide_kind")
KERNEL = "portfolio_cashflow_regimes_kernel"
f32 = np.float32


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _all_same(got, want):
    return set(got) == set(want) and all(_same(got[k], want[k]) for k in want)


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_equal_regimes_and_a_regime_never_left_are_the_parents_reference(oracle, K):
    """Identities 1 and 2: the same multipliers, so the same outputs, for every schedule, R and P."""
    (m0, m1), (f0, f1) = Q.laws(K)
    one = {0: pref.gauss_multipliers(oracle, m0, f0, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST),
           1: pref.gauss_multipliers(oracle, m1, f1, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST)}
    for prob in Q.PROBS[:3]:
        assert _same(Q.multipliers_of(oracle, (m0, m0), (f0, f0), Q.N, Q.LONGEST, prob), one[0])
        assert _same(Q.multipliers_of(oracle, (m1, m1), (f1, f1), Q.N, Q.LONGEST, prob), one[1])
    assert _same(Q.multipliers_of(oracle, (m0, m1), (f0, f1), Q.N, Q.LONGEST, ((0, 777), 0)), one[0])
    assert _same(Q.multipliers_of(oracle, (m0, m1), (f0, f1), Q.N, Q.LONGEST, ((777, 0), Q.ONE)), one[1])
    assert not _same(one[0], one[1]) and not _same(Q.multipliers(oracle, K, Q.PROBS[1]), one[0])
    for name, kw in Q.schedules(oracle, K, Q.PROBS[1]).items():
        for R, P in ((0, Q.LONGEST), (4, 9)):
            got = pcref.simulate(Q.multipliers_of(oracle, (m1, m1), (f1, f1), Q.N, P, Q.PROBS[0]), Q.WEIGHTS[K], R, **Q.cut(kw, P))
            assert _all_same(got, pcref.simulate(one[1][:, :P], Q.WEIGHTS[K], R, **Q.cut(kw, P))), (name, R, P)


@pytest.mark.parametrize("prob", Q.PROBS)
def test_one_asset_without_flows_is_the_regime_reference(oracle, prob):
    """Identity 3, for any R."""
    (m0, m1), (f0, f1) = Q.laws(1)
    want = rref.finals_bulk(oracle, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST, (m0[0], m1[0]), (f0[0, 0], f1[0, 0]), prob[0], prob[1], Q.CAPITAL)
    assert np.isfinite(want).all() and (want > 0).all()
    for R in (0, 4):
        got = pcref.simulate(Q.multipliers(oracle, 1, prob), (1.0,), R)
        assert _same(got["final"], want) and _same(got["holdings"][0], want) and not got["paid"].any() and not got["ruin_period"].any()


def test_a_shorter_run_is_a_prefix(oracle):
    """Identity 4."""
    K, prob, R = 3, Q.PROBS[1], 4
    kw = Q.schedules(oracle, K, prob)["varying"]
    long = pcref.simulate(Q.multipliers(oracle, K, prob), Q.WEIGHTS[K], R, **kw)
    for P in (5, 9, 16):
        short = pcref.simulate(Q.multipliers(oracle, K, prob, P), Q.WEIGHTS[K], R, **Q.cut(kw, P))
        assert np.array_equal(np.where(long["ruin_period"] <= P, long["ruin_period"], 0), short["ruin_period"])
        assert np.array_equal(long["depleted_at"][1:P + 1], short["depleted_at"][1:])


def test_states_and_fields_are_the_regime_references(oracle):
    for prob in Q.PROBS:
        s = Q.states(oracle, Q.N, Q.LONGEST, prob)
        f = rref.fields(oracle, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST)
        assert np.array_equal(s, rref.states(oracle, Q.SEED, Q.FIRST_PATH, Q.N, Q.LONGEST, prob[0], prob[1]))
        assert np.array_equal(s[:, 0], f[:, 0] < prob[1])
        leave = np.asarray(prob[0])
        assert np.array_equal(s[:, 1:] != s[:, :-1], f[:, 1:] < leave[s[:, :-1]])
    flips = Q.states(oracle, Q.N, Q.LONGEST, Q.PROBS[0])
    assert (flips[:, 1:] != flips[:, :-1]).all()  # probability 1: a flip at every period
    assert Q.FIRST_PATH > (1 << 32) and Q.N == 2 * 512 + 65


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_the_schedules_deplete_a_good_part_of_the_paths_and_the_cases_cover_the_product(oracle, K):
    for prob in Q.PROBS:
        for name in Q.SCHEDULES + ["fast_constant"]:
            got = Q.reference(oracle, K, prob, 0, name, Q.LONGEST)
            depleted = 1.0 - got["depleted_at"][0] / Q.N
            assert int(got["depleted_at"].sum()) == Q.N and 0.10 <= depleted <= 0.90, (K, prob, name, depleted)
    cases = list(Q.device_cases(K))
    assert {(tuple(p[0]), p[1], P) for p, P, _, _, _ in cases} == {(tuple(p[0]), p[1], P) for p in Q.PROBS for P in Q.PERIODS}
    assert {R for _, _, R, _, _ in cases} == set(Q.REBALANCE)
    assert {(name, forced) for _, _, _, name, forced in cases} == {(n, x) for n in Q.SCHEDULES + Q.FAST_SCHEDULES for x in (False, True)}
    assert {P % 8 for P in Q.PERIODS} == set(range(8)) and {P % 4 for P in Q.PERIODS} == {0, 1, 2, 3}
    assert set(Q.PERIODS) >= {1, 3, 4, 5, 7, 8, 9, 12, 16, 17, 37}
    # the laws stay inside the bounds the divide rule needs (7 deviations), differ in every entry, and turn every correlation
    (m0, m1), (f0, f1) = Q.laws(K)
    for m, f in ((m0, f0), (m1, f1)):
        assert all(100.0 + m[k] - 7.0 * np.abs(f[k]).sum() > 1.0 for k in range(K))
    assert all(m0[k] != m1[k] and f0[k, k] != f1[k, k] for k in range(K))
    assert all(np.sign(f0[k, j]) == -np.sign(f1[k, j]) for k in range(K) for j in range(k) if j == 0)


# ---- the C ABI and the Python layer ---------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound_and_the_documents_say_so():
    from stock_market_monte_carlo_amd import _lib, build, regimes
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    build.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert ctypes.sizeof(_lib.PortfolioRegimes) == 184 and "sizeof(smmc_portfolio_regimes) = 184" in hdr
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert UNIT in build.SOURCES  # part of the build digest
    import stock_market_monte_carlo_amd as S
    for name in ("make_portfolio_regimes", "simulate_portfolio_cashflow_regimes", "simulate_portfolio_cashflow_regimes_raw",
                 "simulate_portfolio_cashflow_regimes_to_host", "portfolio_cashflow_regimes_divide_kind"):
        assert callable(getattr(regimes, name)) and getattr(S, name) is getattr(regimes, name), name
    assert not any("regimes" in n for n in dir(S.Engine))  # functions of an engine: Engine gains no method
    for doc, words in (("DESIGN.md", ("— Regime-switching plans", "monotone", "v_cndmask")), ("INTEGRATION.md", ("simulate_portfolio_cashflow_regimes",)),
                       ("README.md", ("simulate_portfolio_cashflow_regimes",)), (os.path.join("tools", "README.md"), ("bench_regime_plan.py",))):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(w in text for w in words), doc


def test_make_portfolio_regimes_values_and_errors():
    from stock_market_monte_carlo_amd import _lib, regimes
    from stock_market_monte_carlo_amd.engine import cholesky_factor
    (m0, m1), (f0, f1) = Q.laws(3)
    rg = regimes.make_portfolio_regimes((m0, m1), (f0, f1), mean_durations=(40, 8))
    assert rg.struct_size == 184 and list(rg.leave_q16) == [1638, 8192] and rg.start1_q16 == rref.stationary_start((1638, 8192))
    for r, (m, f) in enumerate(((m0, f0), (m1, f1))):
        assert [rg.means[r][k] for k in range(4)] == [float(f32(x)) for x in m] + [0.0]
        L = np.array(list(rg.factor[r]), dtype=f32).reshape(4, 4)
        assert _same(L[:3, :3], f) and not L[3].any() and not L[:, 3].any()
    assert list(rg.reserved) == [0, 0]
    stds, corrs = ([4.0, 1.5], [7.0, 2.5]), ([[1, 0.6], [0.6, 1]], [[1, -0.6], [-0.6, 1]])
    by_corr = regimes.make_portfolio_regimes(((0.5, 0.2), (-1.0, 0.1)), leave_q16=(0, 65536), start1_q16=65536, stds=stds, corrs=corrs)
    for r in range(2):
        assert _same(np.array(list(by_corr.factor[r]), dtype=f32).reshape(4, 4)[:2, :2], cholesky_factor(stds[r], corrs[r]))
    assert list(by_corr.leave_q16) == [0, 65536] and by_corr.start1_q16 == 65536
    assert regimes.make_portfolio_regimes((m0, m1), (f0, f1), leave_q16=(5, 6), start=0.25).start1_q16 == 16384
    ok = dict(means=(m0, m1), factors=(f0, f1), mean_durations=(40, 8))
    for bad in (dict(ok, leave_q16=(1, 2)), dict(ok, mean_durations=None), dict(ok, start=0.5, start1_q16=3), dict(ok, mean_durations=(0.5, 8)),
                dict(ok, mean_durations=(1e9, 8)), dict(ok, mean_durations=None, leave_q16=(65537, 0)), dict(ok, mean_durations=None, leave_q16=(0, 0)),
                dict(ok, start=1.5), dict(ok, means=(m0,)), dict(ok, means=(m0[:2], m1[:2])), dict(ok, factors=(f0,)), dict(ok, factors=None),
                dict(ok, stds=stds), dict(ok, factors=None, stds=stds), dict(ok, means=((np.nan,) * 3, m1)), dict(ok, factors=(f0.T, f1)),
                dict(ok, factors=(-f0, f1)), dict(ok, means=(m0 + (1.0, 2.0), m1 + (1.0, 2.0)))):
        with pytest.raises(ValueError):
            regimes.make_portfolio_regimes(**bad)
    assert _lib.REGIME_Q16_ONE == 65536


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """The new unit has its own launch and no parent's; every other unit has nothing of the new kernel; and no unit but
    smmc_regimes.cpp leaves an undefined symbol with "egime" in its demangled text (tests/test_regimes_cpu.py)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    units = [u for u in sorted(os.listdir(CSRC)) if u.endswith(".cpp")]
    assert UNIT in units
    for unit in units:
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        if unit == UNIT:
            assert "launch_portfolio_cashflow_markov(" in undefined and "portfolio_cashflow_markov_lds_bytes(" in undefined
            assert "portfolio_cashflow_divide_of_bounds(" in undefined and "egime" not in undefined
            for other in ("launch_portfolio_cashflow(", "launch_portfolio(", "launch_regimes(", "launch_cashflow("):
                assert other not in undefined, other
        else:
            assert "portfolio_cashflow_markov" not in undefined and "PortfolioCashflowMarkovArgs" not in undefined, (unit, undefined)
    text = open(os.path.join(CSRC, UNIT)).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text
    assert "host_wave_walk_run(" in text and "host_outputs_struct_to_host(" in text and "static " not in text  # no state of its own
    assert text.count("portfolio_cashflow_markov_lds_bytes(") == 1  # the need is stated once on the host side
    internal = open(os.path.join(CSRC, "smmc_internal.h")).read()
    assert "launch_portfolio_cashflow_markov(" in internal and "markov_check_q16" not in internal  # nothing of the host side there


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/portfolio_cashflow_regimes_args.cpp over the fake HIP runtime, a stand-alone executable under
    AddressSanitizer and UBSan: {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("pfcfr") / "portfolio_cashflow_regimes_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp", "smmc_stationary.cpp",
                                           "smmc_portfolio.cpp", "smmc_portfolio_cashflow.cpp", UNIT, "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp", "stationary_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "portfolio_cashflow_launch_stub.cpp",
                                                            "portfolio_cashflow_regimes_launch_stub.cpp", "portfolio_cashflow_regimes_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "portfolio_cashflow_regimes_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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
INVALID = {"engine_null": "engine", "sim_null": "sim", "sim_struct_size_wrong": "smmc_sim.struct_size", "portfolio_null": "smmc_portfolio",
           "five_assets": "n_assets", "weights_do_not_sum_to_one": "sum", "n_bins_above_max": "n_bins", "cashflow_null": "cf",
           "no_periods": "n_periods", "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS", "floor_negative": "floor", "fraction_nan": "fraction",
           "table_mode": "mode must be SMMC_MODE_GAUSSIAN", "stream_ref": "REF", "stream_v2": "V2",
           "portfolio_means_set": "smmc_portfolio.means[1]", "portfolio_factor_set": "smmc_portfolio.factor[4]",
           "regimes_null": "the smmc_portfolio_regimes argument is NULL",
           "regimes_struct_size_wrong": "smmc_portfolio_regimes.struct_size is 188, this library expects 184",
           "leave0_above_one": "leave_q16[0] is 65537", "leave1_all_ones": "leave_q16[1] is 4294967295", "start_above_one": "start1_q16 is 65537",
           "mean_nan": "means[0][1] is not finite", "mean_infinite_in_regime_1": "means[1][0] is not finite",
           "mean_beyond_n_assets": "means[1][2] is set beyond n_assets", "factor_nan": "factor[1][1][0] is not finite",
           "factor_above_diagonal": "factor[0][0][1] is 0.5", "factor_beyond_n_assets": "factor[1][2][0] is 0.5",
           "factor_negative_diagonal": "factor[1][1][1] is -2: the diagonal", "regimes_reserved0_not_zero": "reserved is {1, 0}",
           "regimes_reserved1_not_zero": "reserved is {0, 7}", "lds_too_small": "draw tables, depletion counters and histogram need"}
CALL_ONLY = {"outputs_null": "smmc_portfolio_cashflow_outputs", "outputs_struct_size_wrong": "struct_size",
             "outputs_reserved_not_zero": "reserved", "paths_per_workgroup": "shard"}
DEVICE_ONLY = {"paid_misaligned": "4-byte", "depleted_at_misaligned": "8-byte"}
VALID = ["valid", "valid_never_left", "valid_always_left", "valid_exact_div_flag", "valid_varying", "valid_largest", "valid_no_outputs"]


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_their_text_and_without_a_launch(args_report, entry, case):
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
    for entry in ("device", "to_host", "divide_kind"):
        m = re.search(r"need (\d+) bytes of LDS, device allows (\d+)", args_report["_text"][f"{entry}:lds_too_small"])
        assert m and int(m.group(1)) > (1 << 20) > int(m.group(2)) > 0


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", VALID)
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result; the one
    launch is this kernel's, never the parent's.  sim.gauss_mean is NaN and sim.gauss_std negative throughout: not read."""
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
    assert {k for k in args_report if k.startswith(("kind:", "union:", "parent:", "ran:"))} == \
        {f"kind:{c}" for c in KINDS} | {"union:different_conditions", "parent:regime_0", "parent:regime_1", "ran:fast", "ran:exact", "ran:exact_flag"}


FAST, EXACT = 0, 1
# 120 periods, capital 1000, 60 / 40, R = 12 unless named.  The two requests without a withdrawal are EXACT by the rule's own
# bound: the bear regime's worst month, 100 - 1.5 - 49, halves a holding, and 120 halvings leave the fast divide's domain.
KINDS = {"both_calm": FAST, "both_calm_no_floor_buy_and_hold": FAST, "both_calm_no_floor_rebalanced": EXACT, "both_calm_zero_flows": EXACT,
         "both_calm_contributions": EXACT, "regime_never_entered_without_bounds": EXACT, "both_calm_too_many_periods": EXACT,
         "exact_flag": EXACT, "fraction": EXACT}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_kind_of_stated_requests(args_report, case):
    assert args_report[f"kind:{case}"] == (KINDS[case],), case


def test_fast_in_each_regime_through_a_different_condition_is_exact_on_the_union(args_report):
    """tests/cpp/portfolio_cashflow_regimes_args.cpp states the inputs: regime 0 alone is FAST by the shrinking bound and
    fails the per-asset one, regime 1 alone the other way round; the parent says FAST of each law; the union is EXACT."""
    assert args_report["union:different_conditions"] == (FAST, FAST, EXACT)
    assert args_report["parent:regime_0"] == (FAST,) and args_report["parent:regime_1"] == (FAST,)


def test_a_launch_is_given_the_form_the_rule_names_and_the_probabilities(args_report):
    assert args_report["ran:fast"] == (-2, 0, 12) and args_report["ran:exact"] == (-2, 1, 77) and args_report["ran:exact_flag"] == (-2, 1, 77)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 40, 184, 56)


# ---- the kernels as they compile now --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def test_sixteen_instantiations_none_with_scratch_and_the_parents_lists_unchanged(asm):
    """(exact | fast divide) x K = 1 .. 4 x (constant | varying schedule); private segment 0 and no scratch instruction."""
    import isa_loops as L
    import isa_table as T
    lines = open(asm).read().splitlines()
    prefix, symbols = T.instantiations(asm, KERNEL)
    got = sorted(re.match(r"(I(?:L[a-z]\d+E)+E)Ev", s[len(prefix):]).group(1) for s in symbols)
    assert got == sorted(f"ILb{x}ELi{K}ELb{v}EE" for x in (0, 1) for K in (1, 2, 3, 4) for v in (0, 1)) and len(got) == 16
    for sym in symbols:
        sizes = [int(m.group(1)) for l in lines for m in [re.match(r"\s*\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", l)] if m]
        assert sizes == [0], (sym, sizes)
        assert not any(l.split()[0].startswith("scratch_") for l in L.kernel_body(lines, sym) if l.strip() and l.strip()[0] not in ";."), sym
    # the parents' lists as the commit before this feature compiles them
    for kernel, n in (("portfolio_cashflow_kernel", 48), ("regimes_kernel", 3), ("paths_kernel", 18), ("blocks_kernel", 12)):
        found = T.instantiations(asm, kernel, lines)[1]
        assert len(found) == n and len(set(found)) == n, (kernel, len(found))


def test_the_committed_listing_is_of_the_kernels_as_they_compile(asm):
    """profiles/portfolio_cashflow_regimes/isa.txt names every instantiation with the fingerprint it has now."""
    import isa_loop_count as I
    import isa_table as T
    listing = open(os.path.join(ROOT, "profiles", "portfolio_cashflow_regimes", "isa.txt")).read()
    prefix, symbols = T.instantiations(asm, KERNEL)
    assert len(symbols) == 16
    for sym in symbols:
        variant = sym[len(prefix):]
        assert f"{KERNEL}{variant}:" in listing and f"fingerprint {I.fingerprint(asm, variant, KERNEL)[:16]}" in listing, variant
        assert re.search(re.escape(f"{KERNEL}{variant}:") + r" vgpr (\d+) .* private_segment 0 ", listing), variant
