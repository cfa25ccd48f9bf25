"""The circular block bootstrap without a GPU: the numpy restatement (tests/blocks_reference.py) against the CPU
oracle's table stream, the structure of its indices, the prefix property, the frozen fixture; the entry points are
declared, exported and bound; every argument error include/smmc.h lists comes back as SMMC_ERR_INVALID with a text from
all three entries (csrc/smmc_blocks.cpp + csrc/smmc_capi.cpp over tests/cpp/fake_hip.cpp, driven by
tests/cpp/blocks_args.cpp); and which divide a launch uses."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import blocks_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_blocks", "smmc_engine_simulate_blocks_to_host", "smmc_engine_blocks_divide_kind")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("key,P", [("bundled", 360), ("7", 9), ("2049", 41), ("1", 5)])
def test_block_length_one_is_the_table_stream(oracle, key, P):
    """L = 1: every period starts a block, so the restatement is oracle.counter_mc in table mode, bit for bit."""
    table, n = ref.table_of(key), 300
    got = ref.result(oracle, table, n, P, 1)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_TABLE, P, n, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL,
                                             table=table, n_bins=ref.BINS, hist_lo=ref.LO, hist_hi=ref.HI, below_threshold=ref.BELOW))
    assert np.array_equal(_bits(got["final"]), _bits(o["final"]))
    assert np.array_equal(got["hist"], o["hist"]) and got["stats"].below == o["stats"].below
    assert got["stats"].min == o["stats"].min and got["stats"].max == o["stats"].max


@pytest.mark.parametrize("key,L,P", [("bundled", 12, 360), ("bundled", 7, 57), ("7", 9, 100), ("2", 5, 41), ("1", 4, 9),
                                     ("2049", 12, 49), ("bundled", 1130, 1200), ("bundled", 365, 360)])
def test_index_structure(oracle, key, L, P):
    """Inside a block every index is its predecessor + 1 mod T; a block starts where the i.i.d. stream draws its
    index for that path at period b; a block longer than the table wraps around it."""
    table = ref.table_of(key)
    T = table.size
    for path in (0, 5, ref.FIRST_PATH, ref.FIRST_PATH + 255):
        idx = ref.indices(oracle, table, ref.SEED, path, P, L).astype(np.int64)
        assert idx.size == P and idx.min() >= 0 and idx.max() < T
        n_blocks = -(-P // L)
        iid = oracle.counter_path_indices(oracle.make_params(oracle.MODE_TABLE, n_blocks, 1, ref.SEED, table=table), path)
        assert np.array_equal(idx[::L], iid.astype(np.int64))
        t = np.arange(1, P)
        inside = t % L != 0
        assert np.array_equal(idx[1:][inside], (idx[:-1][inside] + 1) % T)
        if L > T:  # the whole table, in order, from the start on
            assert np.array_equal(idx[:T], (idx[0] + np.arange(T)) % T) and idx[T] == idx[0]


def test_the_starts_are_not_all_consecutive(oracle, table):
    """...so the structure test is not vacuous: at L = 12 most block boundaries jump."""
    idx = ref.indices(oracle, table, ref.SEED, 17, 360, 12).astype(np.int64)
    jumps = (idx[12::12] != (idx[11:-1:12] + 1) % table.size).sum()
    assert jumps >= 25  # 29 boundaries


@pytest.mark.parametrize("key,L", [("bundled", 3), ("7", 9), ("2049", 4)])
def test_prefix_property(oracle, key, L):
    """The value after p periods does not depend on n_periods: a run with n_periods = p is column p of a longer one."""
    table = ref.table_of(key)
    for path in (3, ref.FIRST_PATH + 1):
        long = ref.trajectory(oracle, table, ref.SEED, path, 40, L)
        for p in range(0, 41):
            short = ref.trajectory(oracle, table, ref.SEED, path, p, L)
            assert np.array_equal(_bits(short), _bits(long[:p + 1])), (path, p)


def test_the_redo_law(oracle):
    """Five +100 % months and three -50 % months in blocks of four over 360 periods: some, not all, paths end infinite,
    and many pass outside the checked window [2^-81, 2^111] on the way (what tests/test_blocks_gpu.py then runs)."""
    table = ref.redo_table()
    n = 512
    inf = outside = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            tr = ref.trajectory(oracle, table, ref.SEED, ref.FIRST_PATH + i, 360, 4)
            inf += bool(np.isinf(tr[-1]))
            outside += bool(((tr < 2.0 ** -81) | (tr > 2.0 ** 111)).any())
    print(f"redo table: {inf / n:.3f} end at +inf, {outside / n:.3f} leave [2^-81, 2^111]")
    assert 0 < inf < n and inf < outside < n


def test_the_fixture_regenerates_bit_for_bit():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_blocks_golden as G
    assert json.load(open(G.OUT)) == G.generate()


def test_entry_points_are_declared_exported_and_bound():
    import ctypes
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
    assert ctypes.sizeof(_lib.Sim) == 72 and ctypes.sizeof(_lib.Blocks) == 16
    assert re.search(r"#define SMMC_BLOCKS_CIRCULAR 0\b", hdr) and _lib.BLOCKS_CIRCULAR == 0
    assert "smmc_blocks.cpp" in build.SOURCES  # part of the build digest
    for name in ("simulate_blocks", "simulate_blocks_raw", "simulate_blocks_to_host", "blocks_divide_kind"):
        assert hasattr(S.Engine, name), name


def test_the_other_host_units_gained_no_undefined_symbol(tmp_path):
    """csrc/smmc_capi.cpp, smmc_cashflow.cpp and smmc_excursions.cpp refer to nothing of csrc/smmc_blocks.cpp or of
    the blocks kernel: they still link against the stand-ins that predate this feature."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for unit in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp"):
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        assert "blocks" not in undefined, (unit, undefined)


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/blocks_args.cpp over the fake HIP runtime: {case: (return code, length of the error text)}."""
    exe = str(tmp_path_factory.mktemp("bl") / "blocks_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp",
                                           "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp",
                                                            "blocks_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    env.pop("SMMC_BLOCKS_READ", None)
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "blocks_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    out, text = {}, {}
    last = None
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


INVALID = ["mode_gaussian", "no_table", "stream_v2", "stream_ref", "block_len_zero", "struct_size_wrong", "kind_not_circular",
           "reserved_not_zero", "blocks_null", "engine_null", "n_bins_above_max"]
CAUSE = {"mode_gaussian": "SMMC_MODE_TABLE", "no_table": "set_table", "stream_v2": "V2", "stream_ref": "REF",
         "block_len_zero": "block_len", "struct_size_wrong": "struct_size", "kind_not_circular": "kind",
         "reserved_not_zero": "reserved"}


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", INVALID)
def test_argument_errors_are_invalid_with_a_text(args_report, entry, case):
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -1, (entry, case, rc)  # SMMC_ERR_INVALID
    assert text_len > 0
    if case in CAUSE:  # the message names the cause
        assert CAUSE[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", ["valid", "valid_block_len_max", "valid_largest_table"])
def test_a_valid_request_passes_the_argument_checks(args_report, entry, case):
    """The host-only build then stops at its missing kernel: an error of its own (SMMC_ERR_HIP), not SMMC_ERR_INVALID
    and not a result."""
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0


def test_divide_kind(args_report):
    """CHECKED (2) for the +100 % / -50 % table and for a table with the S&P 500's best and worst month over 360 periods, FAST (0) for a +-1 % table, EXACT (1) on request:
    always what smmc_engine_divide_kind(e, sim, 0) says, whatever the block length."""
    assert args_report["kind:redo_table"] == (2, 2)
    assert args_report["kind:best_and_worst_month"] == (2, 2)
    assert args_report["kind:calm_table"] == (0, 0)
    assert args_report["kind:calm_table_L1"] == (0, 0)
    assert args_report["kind:exact_flag"] == (1, 1)
    assert args_report["sizes"] == (72, 16)


def test_the_product_does_not_touch_the_oracle():
    """Neither the package nor the library's sources name the checker."""
    pkg = os.path.join(ROOT, "stock_market_monte_carlo_amd")
    for base, _, files in os.walk(pkg):
        if "_build" in base or "__pycache__" in base:
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".inc")):
                text = open(os.path.join(base, f), errors="replace").read()
                assert "blocks_reference" not in text and "import oracle" not in text and "from oracle" not in text, f
    text = open(os.path.join(CSRC, "smmc_blocks.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text
