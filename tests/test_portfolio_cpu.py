"""Portfolios without a GPU: the restatement's fused multiply-add against libm's fmaf; the restatement (tests/
portfolio_reference.py) against the CPU oracle where a portfolio is a plain path, its prefix property and the
independence of its draws from weights and rebalancing; the law of the correlated normals; the entry points declared,
exported and bound; every argument error include/smmc.h lists as SMMC_ERR_INVALID with a text and without a launch, from
all three entries (csrc/smmc_portfolio.cpp + the library's other host units over tests/cpp/fake_hip.cpp, driven by
tests/cpp/portfolio_args.cpp); the divide rule's answers; the accumulator lease after a failed launch; the engine's
extension slots with two owners.

Not reachable, with the reason: "asset table, histogram and partials beyond the device's LDS".  The largest request the
other checks let through is 5461 rows of 3 assets (padded to 4 words) with 4096 buckets, 103 KiB; an engine assumes 128 KiB
at the least, so the refusal guards a device smaller than any the library runs on."""
import ctypes
import ctypes.util
import os
import re
import subprocess

import numpy as np
import pytest

import portfolio_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_set_asset_table", "smmc_engine_simulate_portfolio", "smmc_engine_simulate_portfolio_to_host",
         "smmc_engine_portfolio_divide_kind")
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- fma32 ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return lambda a, b, c: np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=f32)


def test_fma32_is_fmaf_on_random_triples(fmaf):
    """120000 triples: products and addends of like and of very different magnitude, and sums that cancel."""
    rng = np.random.default_rng(11)
    n = 40000
    a = np.concatenate([rng.normal(0, 1, n), rng.normal(0, 1, n) * 2.0 ** rng.integers(-40, 40, n), rng.normal(0, 4, n)]).astype(f32)
    b = np.concatenate([rng.normal(0, 1, n), rng.normal(0, 1, n) * 2.0 ** rng.integers(-40, 40, n), rng.normal(0, 4, n)]).astype(f32)
    c = np.concatenate([rng.normal(0, 1, n), rng.normal(0, 1, n) * 2.0 ** rng.integers(-40, 40, n), np.zeros(n)]).astype(f32)
    c[2 * n:] = -(a[2 * n:] * b[2 * n:]) * (1 + rng.integers(-2, 3, n) * 2.0 ** -23)  # near-cancelling
    got, want = ref.fma32(a, b, c), fmaf(a, b, c)
    assert got.dtype == f32 and np.array_equal(_bits(got), _bits(want))


def test_fma32_on_double_rounding_traps(fmaf):
    """The exact sum lies just beside the middle of two binary32 neighbours, so that rounding it to binary64 first lands ON
    the middle and the second rounding goes the wrong way.  The issue's trap first; then a family of them."""
    e = 2.0 ** -23
    a, b, c = f32(2.0 ** -12 * (1 + e)), f32(2.0 ** -12 * (1 - e)), f32(1 + e)
    assert ref.fma32(a, b, c) == f32(1 + e)
    assert f32(np.float64(a) * np.float64(b) + np.float64(c)) == f32(1 + 2 * e)  # what the plain binary64 sum gives
    assert fmaf([a], [b], [c])[0] == f32(1 + e)
    A, B, C = [], [], []
    for k in range(1, 40):          # c odd in its last place, the product half a unit in c's last place minus a speck
        for s in (1.0, -1.0):
            for sign in (1.0, -1.0):
                A.append(2.0 ** -12 * (1 + k * e))
                B.append(s * 2.0 ** -12 * (1 - k * e))
                C.append(sign * (1 + (2 * k + 1) * e))
    A, B, C = (np.array(x, dtype=f32) for x in (A, B, C))
    got, want = ref.fma32(A, B, C), fmaf(A, B, C)
    assert np.array_equal(_bits(got), _bits(want))
    plain = (A.astype(np.float64) * B.astype(np.float64) + C.astype(np.float64)).astype(f32)
    assert (plain != want).any()  # the family does contain traps


# ---- properties of the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("T,P", [(37, 41), (2500, 9)])
@pytest.mark.parametrize("R", [0, 1, 5])
def test_one_asset_with_weight_one_is_the_plain_table_path(oracle, T, P, R):
    n = 300
    table = ref.asset_table(T, 1)
    a = ref.table_multipliers(oracle, table, ref.SEED, ref.FIRST_PATH, n, P)
    values, h = ref.simulate(a, (1.0,), R)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_TABLE, P, n, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL,
                                             table=table[:, 0]))
    assert np.array_equal(_bits(values[:, P]), _bits(o["final"])) and np.array_equal(_bits(h[0]), _bits(o["final"]))


def test_asset_zero_reads_the_plain_gaussian_words(oracle):
    """Standard normals of asset 0, scaled as the plain stream scales them in law: the same Philox words, so with std = 1
    and mean = 0 the oracle's own Gaussian multipliers minus 100 are these normals up to the rounding of 100 + z."""
    n, P = 200, 10
    z = ref.standard_normals(oracle, 2, ref.SEED, ref.FIRST_PATH, n, P)
    p = oracle.make_params(oracle.MODE_GAUSSIAN, P, n, ref.SEED, first_path=ref.FIRST_PATH, gauss_mean=0.0, gauss_std=1.0)
    for i in (0, 99, 100, n - 1):  # the id crosses 2^32 between 99 and 100
        r = oracle.counter_path_returns(p, ref.FIRST_PATH + i)
        assert np.abs(r.astype(np.float64) - z[i, :, 0]).max() < 1e-5
    assert np.abs(np.corrcoef(z[:, :, 0].ravel(), z[:, :, 1].ravel())[0, 1]) < 0.1  # asset 1 reads other words


@pytest.mark.parametrize("shape,K", [("t37", 3), ("gauss", 3)])
def test_prefix_property(oracle, shape, K):
    """V_p of a run with P = 41 is the final value of a run with P = p, and its holdings are those before a rebalance at p."""
    n, P, R = 70, 41, 5
    a = ref.multipliers(oracle, shape, K, n, P)
    long_values, _ = ref.simulate(a, ref.WEIGHTS[K], R)
    for p in range(P + 1):
        short, h = ref.simulate(a[:, :p], ref.WEIGHTS[K], R)
        assert np.array_equal(_bits(short[:, p]), _bits(long_values[:, p])), p
        assert np.array_equal(_bits(ref.value(list(h))), _bits(short[:, p])), p


def test_rebalancing_matters_and_the_draws_do_not_depend_on_it(oracle):
    n, P = 100, 24
    a = ref.multipliers(oracle, "t37", 2, n, P)
    assert a is ref.multipliers(oracle, "t37", 2, n, P)  # no argument of the draw names weights or R
    hold, _ = ref.simulate(a, (0.6, 0.4), 0)
    yearly, _ = ref.simulate(a, (0.6, 0.4), 12)
    assert np.array_equal(_bits(hold[:, :13]), _bits(yearly[:, :13])) and (hold[:, 13:] != yearly[:, 13:]).any()
    only0, _ = ref.simulate(a, (1.0, 0.0), 5)
    plain, _ = ref.simulate(a[:, :, :1], (1.0,), 0)
    assert np.array_equal(_bits(only0), _bits(plain))  # a holding of exactly 0 stays 0 and adds nothing


# ---- the law ----------------------------------------------------------------------------------------------------------

def _law(oracle, means, stds, corr, n):
    K = len(means)
    a = ref.gauss_multipliers(oracle, means, ref.factor_of(stds, corr), ref.SEED, 0, n, 1)[:, 0, :].astype(np.float64)
    for k in range(K):  # weights e_k: after one period V_1 = capital * a_k / 100
        w = [1.0 if j == k else 0.0 for j in range(K)]
        v, _ = ref.simulate(a[:, None, :].astype(f32), w, 0)
        assert np.allclose(v[:, 1], ref.CAPITAL * a[:, k] / 100.0, rtol=1e-6)
        assert abs(a[:, k].mean() - (100.0 + means[k])) <= 5 * stds[k] / np.sqrt(n), k
        assert abs(a[:, k].std() - stds[k]) <= 5 * stds[k] / np.sqrt(2 * n), k
    c = np.corrcoef(a.T)
    for k in range(K):
        for j in range(k):
            assert abs(c[k, j] - corr[k][j]) <= 5 * (1 - corr[k][j] ** 2) / np.sqrt(n), (k, j, c[k, j])


@pytest.mark.parametrize("rho", [0.6, -0.3])
def test_the_law_of_two_correlated_assets(oracle, rho):
    """2e5 paths, one period: means, standard deviations and the correlation within five standard errors of their
    estimators under the normal law."""
    _law(oracle, [0.5, 0.2], [4.0, 1.5], [[1.0, rho], [rho, 1.0]], 200000)


def test_the_law_of_four_assets_with_a_full_correlation_matrix(oracle):
    means, stds, corr = ref.gauss_setup(4)
    _law(oracle, means, stds, corr, 200000)


def test_cholesky_factor():
    from stock_market_monte_carlo_amd.engine import cholesky_factor
    means, stds, corr = ref.gauss_setup(4)
    L = cholesky_factor(stds, corr)
    assert L.dtype == f32 and np.array_equal(L, ref.factor_of(stds, corr)) and np.array_equal(L, np.tril(L))
    cov = np.diag(stds) @ corr @ np.diag(stds)
    assert np.allclose(L.astype(np.float64) @ L.astype(np.float64).T, cov, rtol=1e-6)
    with pytest.raises(ValueError):
        cholesky_factor([1.0, 1.0], [[1.0, 1.2], [1.2, 1.0]])
    with pytest.raises(ValueError):
        cholesky_factor([1.0, 1.0, 1.0], [[1.0, 0.0], [0.0, 1.0]])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

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
    m = re.search(r"#define SMMC_MAX_ASSETS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_ASSETS == S.MAX_ASSETS == 4
    assert ctypes.sizeof(_lib.Sim) == 72 and ctypes.sizeof(_lib.Portfolio) == 112 and ctypes.sizeof(_lib.PortfolioOutputs) == 32
    assert "smmc_portfolio.cpp" in build.SOURCES  # part of the build digest
    for name in ("set_asset_table", "simulate_portfolio", "simulate_portfolio_to_host", "portfolio_divide_kind"):
        assert hasattr(S.Engine, name), name
    assert S.cholesky_factor and S.PortfolioResult


def test_the_other_host_units_gained_no_undefined_symbol(tmp_path):
    """csrc/smmc_capi.cpp and the other feature units refer to nothing of csrc/smmc_portfolio.cpp or of its kernel."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for unit in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp"):
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        assert "portfolio" not in undefined and "asset_table" not in undefined, (unit, undefined)


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/portfolio_args.cpp over the fake HIP runtime: {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("pf") / "portfolio_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_portfolio.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "portfolio_launch_stub.cpp", "portfolio_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "portfolio_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
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
           "histogram_range_empty": "histogram", "unknown_mode": "mode"}
CALL_ONLY = {"outputs_null": "smmc_portfolio_outputs", "outputs_struct_size_wrong": "struct_size",
             "outputs_reserved_not_zero": "reserved", "paths_per_workgroup": "shard"}


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    assert INVALID[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", sorted(CALL_ONLY))
def test_errors_of_the_two_simulating_entries(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)
    assert CALL_ONLY[case] in args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("case", ["engine_null", "table_null", "no_rows", "no_assets", "five_assets", "too_large"])
def test_set_asset_table_refuses(args_report, case):
    rc, text_len, _ = args_report["set:" + case]
    assert rc == -1 and text_len > 0


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", ["valid_table", "valid_gaussian", "valid_buy_and_hold", "valid_largest_table"])
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result.  The
    table-mode requests run on an engine that has no single-series table."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_and_no_error(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)


FAST, EXACT = 0, 1
KINDS = {"table_calm": FAST, "gaussian_calm_36": FAST, "gaussian_calm_360": EXACT, "exact_flag": EXACT, "table_doubling_360": EXACT,
         "table_doubling_36": FAST, "gaussian_may_go_negative": EXACT, "gaussian_tiny_weight": EXACT, "gaussian_zero_weight": FAST,
         "no_capital": EXACT}


@pytest.mark.parametrize("case", sorted(KINDS))
def test_the_divide_rule(args_report, case):
    """The fast divide only where the header's rule proves every product inside its domain; never the checked form."""
    assert args_report["kind:" + case] == (KINDS[case],)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    """A portfolio call whose launch fails after it has counted into the engine's accumulator: the record of the next
    call, a plain simulate with buckets, is that call's alone."""
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1)


def test_two_owners_of_extension_slots(args_report):
    """The asset table and the cash-flow schedule on one engine: each allocates once (1 and 2 device or pinned-host
    allocations as the fake runtime counts device ones), finds its state again, and smmc_engine_destroy releases both."""
    set1, cf1, cf2, kind_after, set2, table_allocs, cashflow_allocs, later_allocs, leaked = args_report["slots:two_owners"]
    assert (set1, set2) == (0, 0) and (cf1, cf2) == (-2, -2) and kind_after == FAST
    assert table_allocs == 1 and cashflow_allocs >= 1 and later_allocs == 0 and leaked == 0


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (72, 112, 32)


def test_the_product_does_not_touch_the_oracle():
    text = open(os.path.join(CSRC, "smmc_portfolio.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "portfolio_reference" not in text
