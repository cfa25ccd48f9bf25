"""Pins against code compiled from the REFERENCE's own sources (oracle/_ref/, built by
`make -C oracle _ref`: src/helpers.cpp and the statistics helpers inside
examples/benchmark_mc_gpu.cpp, against this repository's header and library).  The
reference engine itself stays unbuildable; these are its host-side callers.

Runs on CPU.  What those helpers return and write on the inputs below is stored in
tests/golden/ref_callers.json (tests/golden/make_golden.py ref_callers): the oracle and the
drop-in are checked against it everywhere, and where oracle/_ref/ was built (it needs the
reference sources at build time) the compiled helpers are checked against it too."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libsmmc_ref_callers.so")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import WRITER_RETURNS, WRITER_VALUES, ref_callers_inputs  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "ref_callers.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref():
    """The reference's compiled helpers, or None where oracle/_ref/ was not built."""
    return load_ref() if os.path.exists(REF_SO) else None


def load_ref():
    from stock_market_monte_carlo_amd import _lib, build
    build.build()
    _lib.lib()  # loads torch's HIP runtime and libsmmc_hip.so first; the reference objects link to it
    L = C.CDLL(REF_SO)
    L.ref_update_mean_std.argtypes = [C.c_void_p, C.c_long, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ref_update_count_below_min.restype = C.c_long
    L.ref_update_count_below_min.argtypes = [C.c_void_p, C.c_long, C.c_float]
    L.ref_write_data_file.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    L.ref_write_vector_file.argtypes = [C.c_char_p, C.c_void_p, C.c_long]
    return L


def test_oracle_statistics_match_reference_compiled_helpers(ref, golden, oracle, table):
    """update_mean_std / update_count_below_min of examples/benchmark_mc_gpu.cpp:7-41 (compiled
    from the reference) on final values produced by the oracle engine."""
    cases = ref_callers_inputs(table)
    assert len(cases) == len(golden["statistics"])
    for (v, thresholds), rec in zip(cases, golden["statistics"]):
        assert v.size == rec["n"]
        mean, std = np.float32(rec["mean"]), np.float32(rec["std"])
        if ref is not None:  # the recorded outputs are the compiled helpers' own
            m, s = C.c_float(), C.c_float()
            ref.ref_update_mean_std(v.ctypes.data_as(C.c_void_p), v.size, C.byref(m), C.byref(s))
            assert np.float32(m.value) == mean and np.float32(s.value) == std
            assert [ref.ref_update_count_below_min(v.ctypes.data_as(C.c_void_p), v.size, t) for t in thresholds] == rec["below"]
        st, _ = oracle.values_stats(v, below_threshold=1000.0)
        # the reference accumulates the sum in double in index order -> float(sum / n): same as the oracle
        assert np.float32(st.sum / v.size) == mean
        want_std = np.sqrt(max(st.sumsq / v.size - (st.sum / v.size) ** 2, 0.0))
        assert float(std) == pytest.approx(want_std, rel=2e-4, abs=1e-3)  # reference: float residuals, two passes
        for thr, below in zip(thresholds, rec["below"]):
            st, _ = oracle.values_stats(v, below_threshold=thr)
            assert below == st.below


def test_csv_writers_byte_identical_to_reference_helpers(ref, golden, tmp_path):
    """write_data_file / write_vector_file (src/helpers.cpp:18-39, compiled from the reference)
    against the drop-in's, byte for byte."""
    exe = tmp_path / "writers_check"
    pkg = os.path.join(ROOT, "stock_market_monte_carlo_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "writers_check.cpp"), "-o", str(exe), "-L" + pkg,
                           "-lsmmc_hip", "-Wl,-rpath," + pkg, "-pthread"])
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        subprocess.check_call([str(exe)])
        theirs, theirs_vec = golden["data_file"].encode(), golden["vector_file"].encode()
        if ref is not None:  # the recorded files are the compiled writers' own
            r = np.array(WRITER_RETURNS, dtype=np.float32)
            v = np.array(WRITER_VALUES, dtype=np.float32)
            ref.ref_write_data_file(b"theirs.csv", r.ctypes.data_as(C.c_void_p), r.size, v.ctypes.data_as(C.c_void_p), v.size)
            ref.ref_write_vector_file(b"outputs/theirs_vec.csv", v.ctypes.data_as(C.c_void_p), v.size)
            C.CDLL(None).fflush(None)  # the reference's writer announces its file through C stdio: not at interpreter exit
            assert open("outputs/theirs.csv", "rb").read() == theirs
            assert open("outputs/theirs_vec.csv", "rb").read() == theirs_vec
        assert open("outputs/ours.csv", "rb").read() == theirs
        assert open("outputs/ours_vec.csv", "rb").read() == theirs_vec
        assert open("outputs/ours.csv").read().startswith("Returns,,1.5,-2.25,0.1,1e-07,12345.7,-0,\nValues,1000,1015,")
    finally:
        os.chdir(cwd)
