"""The stationary bootstrap (include/smmc.h, smmc_engine_simulate_stationary) without a GPU: the two identities that tie
the numpy restatement (tests/stationary_reference.py) to restatements that already exist; the law -- renewal count, run
lengths, uniform indices -- on the restatement alone; the entry points declared, exported and bound; every argument error
the header lists, from all three entries (csrc/smmc_stationary.cpp and the other host units over tests/cpp/fake_hip.cpp,
driven by tests/cpp/stationary_args.cpp, a stand-alone program under AddressSanitizer and UBSan); and the kernel's six
instantiations as compiled.

On the commit before this feature every test here fails: neither the module's subject nor the symbols exist."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import blocks_reference as bref
import stationary_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_stationary", "smmc_engine_simulate_stationary_to_host", "smmc_engine_stationary_divide_kind")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement against restatements that already exist ---------------------------------------------------------

@pytest.mark.parametrize("key,P", [("bundled", 41), ("7", 9), ("2500", 13), ("1", 5)])
def test_probability_one_is_the_table_stream(oracle, key, P):
    """q = 65536: every period takes its candidate, so the restatement is oracle.counter_mc in table mode, bit for bit."""
    table, n = bref.table_of(key), 300
    got = ref.result(oracle, table, n, P, ref.ONE)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_TABLE, P, n, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL,
                                             table=table, n_bins=bref.BINS, hist_lo=bref.LO, hist_hi=bref.HI, below_threshold=bref.BELOW))
    assert np.array_equal(_bits(got["final"]), _bits(o["final"]))
    assert np.array_equal(got["hist"], o["hist"]) and got["stats"].below == o["stats"].below
    assert got["stats"].min == o["stats"].min and got["stats"].max == o["stats"].max


@pytest.mark.parametrize("key,P", [("bundled", 41), ("7", 9), ("2500", 13), ("1", 5), ("bundled", 1200)])
def test_probability_zero_is_one_block(oracle, key, P):
    """q = 0: one run from c_0, which is blocks_reference.finals_bulk with a block as long as the path."""
    table, n = bref.table_of(key), 300
    got = ref.finals_bulk(oracle, table, ref.SEED, ref.FIRST_PATH, n, P, 0)
    assert np.array_equal(_bits(got), _bits(bref.finals_bulk(oracle, table, ref.SEED, ref.FIRST_PATH, n, P, P)))


def test_the_fields_are_the_halves_of_the_second_block(oracle):
    """Field t of a path, looked up one Philox block at a time: counter (t / 8, id lo, id hi, 2), word (t % 8) / 2, the low
    half for an even t % 8."""
    f = ref.fields(oracle, ref.SEED, ref.FIRST_PATH, 3, 19)
    key = np.array([ref.SEED & 0xFFFFFFFF, ref.SEED >> 32], dtype=np.uint32)
    for i in range(3):
        path = ref.FIRST_PATH + i
        for t in range(19):
            w = int(oracle.philox4x32_10(np.array([t // 8, path & 0xFFFFFFFF, path >> 32, 2], dtype=np.uint32), key)[(t % 8) // 2])
            assert f[i, t] == ((w >> 16) if t % 2 else (w & 0xFFFF)), (i, t)


def test_the_prefix_property(oracle):
    """The value after p periods does not depend on n_periods."""
    table = bref.table_of("bundled")
    idx = ref.indices_bulk(oracle, table, ref.SEED, ref.FIRST_PATH, 16, 40, 5461)
    for p in (1, 7, 8, 9, 23):
        assert np.array_equal(ref.indices_bulk(oracle, table, ref.SEED, ref.FIRST_PATH, 16, p, 5461), idx[:, :p]), p


def test_the_one_pass_chunk_statistics_agree_with_the_oracles(oracle):
    v = ref.finals_bulk(oracle, bref.table_of("bundled"), ref.SEED, ref.FIRST_PATH, 775, 41, 5461)
    cm, cv = ref.chunk_mean_var_device_order(v)
    om, ov = oracle.chunk_mean_var(v)
    assert cm.size == 4 and np.allclose(cm, om, rtol=1e-6, atol=0.0) and np.allclose(cv, ov, rtol=1e-5, atol=0.0)


# ---- the law, on the restatement alone -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def law(oracle):
    n, P, q = 2000, 360, 5461
    table = bref.table_of("bundled")
    idx = ref.indices_bulk(oracle, table, ref.SEED, ref.FIRST_PATH, n, P, q)
    f = ref.fields(oracle, ref.SEED, ref.FIRST_PATH, n, P)
    return {"n": n, "P": P, "q": q, "T": int(table.size), "idx": idx, "renew": f[:, 1:] < q}


def test_the_number_of_renewals(law):
    """Binomial((P - 1) n, q / 65536): within 5 sigma of its mean."""
    trials, p = (law["P"] - 1) * law["n"], law["q"] / 65536.0
    got, mean, sigma = int(law["renew"].sum()), trials * p, (trials * p * (1.0 - p)) ** 0.5
    print(f"renewals: {got}, expected {mean:.0f} +- {sigma:.0f}")
    assert abs(got - mean) < 5.0 * sigma


def test_a_renewal_jumps_and_nothing_else_does(law):
    idx, T = law["idx"], law["T"]
    on = (idx[:, :-1] + 1) % T
    assert np.array_equal(idx[:, 1:][~law["renew"]], on[~law["renew"]])
    assert (idx[:, 1:][law["renew"]] != on[law["renew"]]).mean() > 0.99  # a candidate is the next month once in T


def test_the_mean_run_length(law):
    """Runs that a renewal ends (the last run of a path is cut by P): their empirical mean within 5 % of 65536 / q."""
    lengths = []
    for row in law["renew"]:
        starts = np.flatnonzero(np.concatenate([[True], row]))  # period 0 starts a run
        lengths.append(np.diff(starts))
    lengths = np.concatenate(lengths)
    got, want = float(lengths.mean()), 65536.0 / law["q"]
    print(f"{lengths.size} runs, mean length {got:.3f}, 65536 / q = {want:.3f}")
    assert abs(got - want) < 0.05 * want


def test_the_last_index_is_uniform(law):
    """Chi-square of the indices at period 359 over 49 cells of 23 months (1127 = 49 * 23) at the 1e-4 level: the 99.99 %
    quantile of chi-square with 48 degrees of freedom is 93.22 (Wilson-Hilferty's 48 (1 - 2/432 + 3.719 sqrt(2/432))^3
    gives 93.4)."""
    assert law["T"] == 49 * 23
    counts = np.bincount(law["idx"][:, law["P"] - 1] // 23, minlength=49)
    expected = law["n"] / 49.0
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print(f"chi-square {chi2:.1f} on 48 degrees of freedom")
    assert chi2 < 93.22


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
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    assert ctypes.sizeof(_lib.Stationary) == 16
    assert re.search(r"#define SMMC_RENEW_Q16_ONE 65536u\b", hdr) and _lib.RENEW_Q16_ONE == 65536
    assert "smmc_stationary.cpp" in build.SOURCES  # part of the build digest
    # smmc_blocks.kind is no longer held back for this feature
    assert "only kind for now" not in hdr and "is reserved for it" not in open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("simulate_stationary", "simulate_stationary_raw", "simulate_stationary_to_host", "stationary_divide_kind", "renew_q16_of"):
        assert callable(getattr(S, name)), name
        assert not hasattr(S.Engine, name), name  # the engine's public callables are held to their golden
    for doc, word in (("README.md", "smmc_engine_simulate_stationary"), ("INTEGRATION.md", "smmc_engine_simulate_stationary"),
                      ("DESIGN.md", "Stationary bootstrap"), (os.path.join("tools", "README.md"), "bench_stationary.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_renew_q16_of():
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import stationary
    assert [S.renew_q16_of(m) for m in (1, 2, 3, 12, 60, 1.5, 65536, 131071)] == [65536, 32768, 21845, 5461, 1092, 43691, 1, 1]
    for bad in (0, 0.99, -3, float("nan"), 131072, 1e9, float("inf")):  # round(0.5) is 0: Python rounds a tie to even
        with pytest.raises(ValueError):
            S.renew_q16_of(bad)
    assert stationary.make_stationary(renew_q16=0).renew_q16 == 0 and stationary.make_stationary(mean_block_len=12).renew_q16 == 5461
    st = stationary.make_stationary(renew_q16=65536)
    assert (st.struct_size, st.renew_q16, st.reserved[0], st.reserved[1]) == (16, 65536, 0, 0)
    for kw in ({}, {"mean_block_len": 12, "renew_q16": 5461}, {"renew_q16": 65537}, {"renew_q16": -1}):
        with pytest.raises(ValueError):
            stationary.make_stationary(**kw)


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """csrc/smmc_blocks.cpp lends its enqueue and gains no undefined symbol; no other unit refers to the new kernel."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    seen = {}
    for unit in sorted(u for u in os.listdir(CSRC) if u.endswith(".cpp")):
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        seen[unit] = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
    for unit, undefined in seen.items():
        if unit == "smmc_stationary.cpp":
            for own in ("launch_stationary", "stationary_lds_bytes", "host_enqueue_paths", "host_simulate_to_host"):
                assert own in undefined, own
            for other in ("launch_blocks", "launch_paths", "launch_finalize", "engine_acc_lease"):
                assert other not in undefined, other
        else:
            assert "stationary" not in undefined, (unit, undefined)
    launches = set(re.findall(r"smmc::(launch_\w+|\w+_lds_bytes)\(", seen["smmc_blocks.cpp"]))
    assert launches == {"launch_blocks", "blocks_lds_bytes", "launch_finalize"}, launches
    text = open(os.path.join(CSRC, "smmc_stationary.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text


# ---- the argument checks ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/stationary_args.cpp over the fake HIP runtime, a stand-alone executable under AddressSanitizer and UBSan:
    {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("stationary") / "stationary_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp", "smmc_stationary.cpp",
                                           "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "stationary_launch_stub.cpp", "stationary_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stationary_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out, text, last = {}, {}, None
    for line in r.stdout.splitlines():
        if line.startswith("#") and last:
            text[last] = line[1:].strip()
            continue
        parts = line.split()
        if len(parts) >= 3:
            out[parts[0]] = tuple(int(x) for x in parts[1:])
            last = parts[0]
    out["_text"] = text
    return out


ENTRIES = ["device", "to_host", "divide_kind"]
INVALID = {"stationary_null": "NULL", "struct_size_wrong": "struct_size", "renew_above_one": "renew_q16", "renew_all_ones": "renew_q16",
           "reserved0_not_zero": "reserved", "reserved1_not_zero": "reserved", "mode_gaussian": "SMMC_MODE_TABLE", "stream_v2": "V2",
           "stream_ref": "REF", "no_table": "set_table", "lds_too_small": "LDS", "engine_null": None, "n_bins_above_max": None}
VALID = ["valid", "valid_never", "valid_always", "valid_largest_table"]


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
    not a result."""
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0
    assert "launch_stationary" in args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_launch_nothing(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0)


def test_divide_kind(args_report):
    """tests/cpp/blocks_args.cpp's cases: CHECKED (2) for the +100 % / -50 % table and for a table with the S&P 500's best
    and worst month over 360 periods, FAST (0) for a +-1 % table, EXACT (1) on request: always what
    smmc_engine_divide_kind(e, sim, 0) says, whatever the renewal probability."""
    assert args_report["kind:redo_table"] == (2, 2)
    assert args_report["kind:best_and_worst_month"] == (2, 2)
    assert args_report["kind:calm_table"] == (0, 0)
    assert args_report["kind:calm_table_always"] == (0, 0)
    assert args_report["kind:exact_flag"] == (1, 1)
    assert args_report["sizes"] == (72, 16)


def test_every_case_of_the_args_program_is_claimed(args_report):
    want = {f"{e}:{c}" for e in ENTRIES for c in INVALID}
    want |= {f"{e}:{c}" for e in ("device", "to_host") for c in VALID + ["valid_no_paths"]}
    want |= {"kind:redo_table", "kind:best_and_worst_month", "kind:calm_table", "kind:calm_table_always", "kind:exact_flag", "sizes", "_text"}
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


def test_the_six_instantiations_without_scratch(asm):
    """Three divides x (eight | four) candidates per Philox block; none with a private segment."""
    args, symbols = _instantiations(asm, "stationary_kernel")
    assert args == sorted(f"ILi{div}ELb{dense}EE" for div in (0, 1, 2) for dense in (0, 1)), args
    text = open(asm).read()
    for sym in symbols:
        m = re.search(r"\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", text)
        assert m and int(m.group(1)) == 0, sym
        v = re.search(r"\.set " + re.escape(sym) + r"\.num_vgpr, (\d+)", text)
        assert v and int(v.group(1)) <= 72, sym  # seven waves per SIMD


def test_the_other_families_are_what_they_were(asm):
    """The lists test_feature_matrix_cpu and tools/pmc_traffic.py know: twelve blocks_kernel, eighteen paths_kernel."""
    blocks, _ = _instantiations(asm, "blocks_kernel")
    assert blocks == sorted(f"ILi{div}ELb{dense}ELb{wide}EE" for div in (0, 1, 2) for dense in (0, 1) for wide in (0, 1)), blocks
    paths, _ = _instantiations(asm, "paths_kernel")
    assert paths == sorted(f"ILi{mode}ELi{div}ELb{dense}EE" for mode in (0, 1, 2, 3) for div in (0, 1, 2) for dense in (0, 1)
                           if not (mode in (1, 2) and dense)), paths
