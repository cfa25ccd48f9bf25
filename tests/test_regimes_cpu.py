"""Regime-switching Gaussian paths (include/smmc.h, smmc_engine_simulate_regimes) without a GPU: the identities that tie the
numpy restatement (tests/regimes_reference.py) to the portfolio's; the law -- regime share, sojourn lengths, the start -- on
the restatement alone; the entry points declared, exported and bound; make_regimes and its refusals; every argument error
the header lists, from all three entries (csrc/smmc_regimes.cpp and the other host units over tests/cpp/fake_hip.cpp, driven
by tests/cpp/regimes_args.cpp, a stand-alone program under AddressSanitizer and UBSan); and the kernel's three
instantiations as compiled.

On the commit before this feature every test here fails: neither the module's subject nor the symbols exist."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import portfolio_reference as pref
import regimes_reference as ref
import stationary_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_regimes", "smmc_engine_simulate_regimes_to_host", "smmc_engine_regimes_divide_kind")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _one_asset(oracle, n, P, mean, std):
    a = pref.gauss_multipliers(oracle, (mean,), ((std,),), ref.SEED, ref.FIRST_PATH, n, P)
    return pref.simulate(a, (1.0,), 0, ref.CAPITAL)[0][:, P]


# ---- the restatement against the portfolio's ---------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 7, 41, 360])
def test_equal_regimes_are_one_asset(oracle, P):
    """Identity 1: with mean[0] == mean[1] and std[0] == std[1] the state selects between equal numbers."""
    want = _one_asset(oracle, 300, P, 0.9, 3.5)
    for leave, start1 in (((1638, 8192), 10920), ((65536, 65536), 32768), ((0, 0), 0), ((12345, 54321), 65536)):
        got = ref.finals_bulk(oracle, ref.SEED, ref.FIRST_PATH, 300, P, (0.9, 0.9), (3.5, 3.5), leave, start1)
        assert np.array_equal(_bits(got), _bits(want)), (leave, start1)


@pytest.mark.parametrize("P", [1, 9, 360])
def test_a_regime_never_left_is_one_asset(oracle, P):
    """Identity 2: a path that starts in a regime it never leaves reads that regime's numbers alone."""
    got0 = ref.finals_bulk(oracle, ref.SEED, ref.FIRST_PATH, 300, P, ref.MEANS, ref.STDS, (0, 40000), 0)
    got1 = ref.finals_bulk(oracle, ref.SEED, ref.FIRST_PATH, 300, P, ref.MEANS, ref.STDS, (40000, 0), 65536)
    assert np.array_equal(_bits(got0), _bits(_one_asset(oracle, 300, P, ref.MEANS[0], ref.STDS[0])))
    assert np.array_equal(_bits(got1), _bits(_one_asset(oracle, 300, P, ref.MEANS[1], ref.STDS[1])))
    assert not np.array_equal(_bits(got0), _bits(got1))


def test_the_prefix_property(oracle):
    """Identity 3: states and multipliers of the first p periods do not depend on n_periods."""
    args = (ref.MEANS, ref.STDS, (1638, 8192), 10920)
    a = ref.multipliers(oracle, ref.SEED, ref.FIRST_PATH, 16, 40, *args)
    s = ref.states(oracle, ref.SEED, ref.FIRST_PATH, 16, 40, (1638, 8192), 10920)
    for p in (1, 3, 4, 5, 7, 8, 9, 23):
        assert np.array_equal(_bits(ref.multipliers(oracle, ref.SEED, ref.FIRST_PATH, 16, p, *args)), _bits(a[:, :p])), p
        assert np.array_equal(ref.states(oracle, ref.SEED, ref.FIRST_PATH, 16, p, (1638, 8192), 10920), s[:, :p]), p


def test_the_fields_are_the_halves_of_the_tag_4_block(oracle):
    """Field t of a path, looked up one Philox block at a time: counter (t / 8, id lo, id hi, 4), word (t % 8) / 2, the low
    half for an even t % 8; and they are not the renewal fields of the stationary bootstrap (tag 2)."""
    f = ref.fields(oracle, ref.SEED, ref.FIRST_PATH, 3, 19)
    key = np.array([ref.SEED & 0xFFFFFFFF, ref.SEED >> 32], dtype=np.uint32)
    for i in range(3):
        path = ref.FIRST_PATH + i
        for t in range(19):
            w = int(oracle.philox4x32_10(np.array([t // 8, path & 0xFFFFFFFF, path >> 32, 4], dtype=np.uint32), key)[(t % 8) // 2])
            assert f[i, t] == ((w >> 16) if t % 2 else (w & 0xFFFF)), (i, t)
    other = sref.fields(oracle, ref.SEED, ref.FIRST_PATH, 3, 19)
    assert np.array_equal(ref.fields(oracle, ref.SEED, ref.FIRST_PATH, 3, 19, tag=2), other) and (f != other).mean() > 0.99


def test_a_state_changes_the_bits(oracle):
    """The test regimes are far enough apart: one flipped state changes the multiplier of every path."""
    z = pref.standard_normals(oracle, 1, ref.SEED, ref.FIRST_PATH, 549, 33)[:, :, 0]
    a = [pref.fma32(np.float32(ref.STDS[r]), z, np.float32(100.0) + np.float32(ref.MEANS[r])) for r in (0, 1)]
    assert (_bits(a[0]) != _bits(a[1])).all()


# ---- the law, on the restatement alone -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def law(oracle):
    n, P, leave, start1 = 4096, 360, (1638, 8192), 40000
    return {"n": n, "P": P, "leave": leave, "start1": start1, "s": ref.states(oracle, ref.SEED, ref.FIRST_PATH, n, P, leave, start1)}


def test_the_start_is_honoured(law):
    """Period 0 is in regime 1 with probability start1_q16 / 65536: binomial, within 5 sigma."""
    p = law["start1"] / 65536.0
    got, mean, sigma = int(law["s"][:, 0].sum()), law["n"] * p, (law["n"] * p * (1.0 - p)) ** 0.5
    print(f"paths starting in regime 1: {got}, expected {mean:.0f} +- {sigma:.0f}")
    assert abs(got - mean) < 5.0 * sigma


def test_the_share_of_regime_one(law):
    """From period 100 on (the start's weight (1 - l0 - l1)^t is below 1e-7 there) the share of regime 1 is l0 / (l0 + l1).
    Periods of one path are correlated: the standard error is taken over the paths' own shares, which are independent."""
    l0, l1 = law["leave"]
    per_path = law["s"][:, 100:].mean(axis=1)
    got, want, se = float(per_path.mean()), l0 / (l0 + l1), float(per_path.std(ddof=1)) / law["n"] ** 0.5
    print(f"share of regime 1: {got:.5f}, l0 / (l0 + l1) = {want:.5f}, standard error {se:.5f}")
    assert abs(got - want) < 5.0 * se


@pytest.mark.parametrize("r", (0, 1))
def test_the_mean_sojourn(law, r):
    """Sojourns in regime r with a flip at both ends (a path's first and last are cut by the horizon and left out): geometric
    with mean 1 / p = 65536 / l_r and second moment (2 - p) / p^2.  A complete sojourn of length L fits fewer places of a
    horizon of P periods the longer it is, so the observed mean lies below 1 / p, by less than E[L^2] / P; apart from that
    bias it sits within 5 standard errors."""
    lengths = []
    for row in law["s"]:
        flips = np.flatnonzero(np.diff(row))  # a flip between t and t + 1
        if flips.size >= 2:
            runs, regime = np.diff(flips), row[flips[:-1] + 1]
            lengths.append(runs[regime == r])
    lengths = np.concatenate(lengths)
    p = law["leave"][r] / 65536.0
    got, want, se = float(lengths.mean()), 1.0 / p, ((1.0 - p) / p ** 2 / lengths.size) ** 0.5
    print(f"regime {r}: {lengths.size} sojourns, mean {got:.3f}, 65536 / l = {want:.3f}, standard error {se:.3f}")
    assert lengths.size > 1000
    assert want - (2.0 - p) / (p * p * law["P"]) - 5.0 * se < got < want + 5.0 * se


# ---- the C ABI and the Python interface ------------------------------------------------------------------------------

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
    assert ctypes.sizeof(_lib.Regimes) == 40
    assert re.search(r"#define SMMC_REGIME_Q16_ONE 65536u\b", hdr) and _lib.REGIME_Q16_ONE == 65536
    assert "smmc_regimes.cpp" in build.SOURCES  # part of the build digest
    assert "gauss_mean and sim->gauss_std are NOT read" in hdr
    for name in ("make_regimes", "simulate_regimes", "simulate_regimes_raw", "simulate_regimes_to_host", "regimes_divide_kind"):
        assert callable(getattr(S, name)), name
        assert not hasattr(S.Engine, name), name  # the engine's public callables are held to their golden
    for doc, word in (("README.md", "smmc_engine_simulate_regimes"), ("INTEGRATION.md", "smmc_engine_simulate_regimes"),
                      ("DESIGN.md", "Regime-switching Gaussian paths"), (os.path.join("tools", "README.md"), "bench_regimes.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_make_regimes():
    import stock_market_monte_carlo_amd as S
    rg = S.make_regimes((0.9, -1.5), (3.5, 7.0), mean_durations=(40, 8))
    assert (rg.struct_size, list(rg.leave_q16), rg.start1_q16, list(rg.reserved)) == (40, [1638, 8192], 10920, [0, 0])
    assert [round(x, 5) for x in rg.mean] == [0.9, -1.5] and [round(x, 5) for x in rg.std] == [3.5, 7.0]
    assert list(S.make_regimes((0, 0), (1, 1), mean_durations=(1, 65536)).leave_q16) == [65536, 1]
    assert list(S.make_regimes((0, 0), (1, 1), mean_durations=(2, 65536 / 65535)).leave_q16) == [32768, 65535]
    assert S.make_regimes((0, 0), (1, 1), leave_q16=(0, 0), start=0.25).start1_q16 == 16384
    assert S.make_regimes((0, 0), (1, 1), leave_q16=(0, 0), start1_q16=65536).start1_q16 == 65536
    assert S.make_regimes((0, 0), (1, 1), leave_q16=(0, 7)).start1_q16 == 0 and S.make_regimes((0, 0), (1, 1), leave_q16=(7, 0)).start1_q16 == 65536
    bad = [dict(), dict(mean_durations=(40, 8), leave_q16=(1, 1)), dict(mean_durations=(0.5, 8)), dict(mean_durations=(40, 131072)),
           dict(mean_durations=(40, float("nan"))), dict(leave_q16=(65537, 1)), dict(leave_q16=(1, -1)), dict(leave_q16=(1.5, 1)),
           dict(leave_q16=(0, 0)), dict(leave_q16=(1, 1), start=1.5), dict(leave_q16=(1, 1), start1_q16=65537),
           dict(leave_q16=(1, 1), start=0.5, start1_q16=3), dict(leave_q16=(1, 1, 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            S.make_regimes((0.9, -1.5), (3.5, 7.0), **kw)
    for means, stds in (((0.9,), (3.5, 7.0)), ((0.9, float("inf")), (3.5, 7.0)), ((0.9, -1.5), (3.5, -7.0)), ((0.9, -1.5), (float("nan"), 7.0))):
        with pytest.raises(ValueError):
            S.make_regimes(means, stds, leave_q16=(1, 1))


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """csrc/smmc_blocks.cpp lends its enqueue and gains no undefined symbol; no other unit refers to the new kernel."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for unit in sorted(u for u in os.listdir(CSRC) if u.endswith(".cpp")):
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        if unit == "smmc_regimes.cpp":
            for own in ("launch_regimes", "regimes_lds_bytes", "host_enqueue_paths", "host_simulate_to_host", "host_divide_kind_of_bounds"):
                assert own in undefined, own
            for other in ("launch_blocks", "launch_paths", "launch_finalize", "engine_acc_lease", "launch_portfolio"):
                assert other not in undefined, other
        else:
            assert "egime" not in undefined, (unit, undefined)
    text = open(os.path.join(CSRC, "smmc_regimes.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text


# ---- the argument checks ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/regimes_args.cpp over the fake HIP runtime, a stand-alone executable under AddressSanitizer and UBSan:
    {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("regimes") / "regimes_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp", "smmc_regimes.cpp",
                                           "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "regimes_launch_stub.cpp", "regimes_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "regimes_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out, text, last = {}, {}, None
    for line in r.stdout.splitlines():
        if line.startswith("#") and last:
            text[last] = line[1:].strip()
            continue
        parts = line.split()
        if len(parts) >= 2 and parts[0] != "regimes_args:":
            out[parts[0]] = tuple(int(x) for x in parts[1:])
            last = parts[0]
    out["_text"] = text
    return out


ENTRIES = ["device", "to_host", "divide_kind"]
INVALID = {"regimes_null": "NULL", "struct_size_wrong": "struct_size", "mode_table": "SMMC_MODE_GAUSSIAN", "stream_v2": "V2",
           "stream_ref": "REF", "leave0_above_one": "leave_q16[0]", "leave1_all_ones": "leave_q16[1]", "start1_above_one": "start1_q16",
           "mean0_nan": "mean[0]", "mean1_inf": "mean[1]", "std0_inf": "std[0]", "std1_nan": "std[1]", "std1_negative": "std[1]",
           "reserved0_not_zero": "reserved", "reserved1_not_zero": "reserved", "lds_too_small": "LDS", "engine_null": None,
           "n_bins_above_max": None}
VALID = ["valid", "valid_edges", "valid_no_periods"]
KINDS = {"kind:calm": 0, "kind:crash": 2, "kind:unbounded": 1, "kind:crash_never_entered": 2, "kind:exact_flag": 1}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text(args_report, entry, case):
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -1, (entry, case, rc)  # SMMC_ERR_INVALID
    assert text_len > 0
    if INVALID[case]:  # the message names the cause
        assert INVALID[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", VALID)
def test_a_valid_request_passes_the_argument_checks(args_report, entry, case):
    """The host-only build then stops at its missing kernel: an error of its own (SMMC_ERR_HIP), not SMMC_ERR_INVALID and
    not a result.  The sim of these requests holds a NaN gauss_mean and a negative gauss_std: neither is read."""
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0
    assert "launch_regimes" in args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_launch_nothing(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0)


def test_divide_kind(args_report):
    """Three stated requests over 360 periods from 1000: FAST (0) for regimes (0.5, 0.8) and (-0.5, 1.5), whose union
    [88.999, 106.101] is proven; CHECKED (2) for (0.5, 1.0) and (-40, 8), union [3.999, 116.001], also when the second regime
    can never be entered (the rule reads the bounds, not the probabilities); EXACT (1) for a regime with 98.5 - 7 * 15 < 0,
    and on request."""
    for case, kind in KINDS.items():
        assert args_report[case] == (kind,), case
    assert args_report["sizes"] == (72, 40)


def test_every_case_of_the_args_program_is_claimed(args_report):
    want = {f"{e}:{c}" for e in ENTRIES for c in INVALID}
    want |= {f"{e}:{c}" for e in ("device", "to_host") for c in VALID + ["valid_no_paths"]}
    want |= set(KINDS) | {"sizes", "_text"}
    assert set(args_report) == want, set(args_report) ^ want


# ---- the kernel as compiled ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def _instantiations(asm, kernel):
    import isa_table as T
    prefix, symbols = T.instantiations(asm, kernel)
    return sorted(s[len(prefix):].split("Ev")[0] for s in symbols), symbols


def test_the_three_instantiations_without_scratch(asm):
    """Three divides; none with a private segment."""
    args, symbols = _instantiations(asm, "regimes_kernel")
    assert args == sorted(f"ILi{div}EE" for div in (0, 1, 2)), args
    text = open(asm).read()
    for sym in symbols:
        m = re.search(r"\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", text)
        assert m and int(m.group(1)) == 0, sym


def test_the_other_families_are_what_they_were(asm):
    """The lists tests/test_stationary_cpu.py knows, and the stationary walk's own six: blocks_body's new template argument
    adds no instantiation to the families that pass it a plain word."""
    blocks, _ = _instantiations(asm, "blocks_kernel")
    assert blocks == sorted(f"ILi{div}ELb{dense}ELb{wide}EE" for div in (0, 1, 2) for dense in (0, 1) for wide in (0, 1)), blocks
    paths, _ = _instantiations(asm, "paths_kernel")
    assert paths == sorted(f"ILi{mode}ELi{div}ELb{dense}EE" for mode in (0, 1, 2, 3) for div in (0, 1, 2) for dense in (0, 1)
                           if not (mode in (1, 2) and dense)), paths
    stationary, _ = _instantiations(asm, "stationary_kernel")
    assert stationary == sorted(f"ILi{div}ELb{dense}EE" for div in (0, 1, 2) for dense in (0, 1)), stationary
