"""Regenerates the fixtures in tests/golden/ (run from the repo root, CPU only).

  libstdcxx_random.json   system libstdc++ <random> outputs + whole reference-style
                          paths, produced by oracle/pin/pin_libstdcxx.cpp (the real
                          library the reference calls at src/simulations.cpp:245-250).
                          This pins the oracle's hand-written mt19937 / Lemire map.
  counter_stream_v2.json  frozen outputs of the oracle's counter-stream engine (C):
  counter_stream_v3.json  regression vectors for the HIP kernels that also travel to
                          the GPU box (v2: round 1's stream, selected with SMMC_FLAG_STREAM_V2;
                          v3: the default).  The stream number sets the Philox counter layout in
                          BOTH modes, so the table-mode values of counter_stream_v3.json are NOT
                          those of round 1 (counter_stream_v2.json holds them, bit-unchanged).
                          Pinned to the oracle itself only.
  ref_callers.json        `python tests/golden/make_golden.py ref_callers`: what the reference's own
                          host helpers return / write on the inputs of tests/test_ref_callers_cpu.py
                          (update_mean_std and update_count_below_min of examples/benchmark_mc_gpu.cpp,
                          write_data_file and write_vector_file of src/helpers.cpp), executed from
                          oracle/_ref/ (`make -C oracle _ref`, which needs the reference sources).

The reference engine itself could not be built here (see oracle/Makefile); ref_callers.json is
the only fixture in this directory that comes from executed reference code.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

HERE = os.path.join(ROOT, "tests", "golden")


def load_table():
    vals = []
    with open(os.path.join(ROOT, "data", "SP500_monthly_returns.csv")) as f:
        header = f.readline().strip().split(",")
        col = header.index("returns")
        for line in f:
            cell = line.rstrip("\n").split(",")[col]
            if cell != "":
                vals.append(np.float32(cell))
    return np.array(vals, dtype=np.float32)


def main():
    table = load_table()
    assert table.size == 1127
    # --- libstdc++ pin -----------------------------------------------------
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "pin/pin_libstdcxx"])
    tab_txt = os.path.join(HERE, "_table.txt")
    with open(tab_txt, "w") as f:
        for v in table:
            f.write(f"{float(v):.9g}\n")
    out = subprocess.check_output([os.path.join(ROOT, "oracle", "pin", "pin_libstdcxx"), tab_txt])
    os.remove(tab_txt)
    pin = json.loads(out)
    pin["table_bits_fnv1a"] = int(fnv1a(table.view(np.uint32)))
    with open(os.path.join(HERE, "libstdcxx_random.json"), "w") as f:
        json.dump(pin, f, indent=1)
    # --- counter stream regression vectors (v2 = round 1's Gaussian draw, v3 = the default) -------
    for stream in (2, 3):
        cases = []
        for mode, name in ((O.MODE_TABLE, "table"), (O.MODE_GAUSSIAN, "gaussian")):
            for P in (1, 3, 4, 5, 360, 1000):
                for first in (0, (1 << 32) - 100):
                    p = O.make_params(mode, P, 300, seed=0x5EED0123456789AB, first_path=first, table=table,
                                      n_bins=100, hist_lo=0.0, hist_hi=20000.0, stream=stream)
                    r = O.counter_mc(p)
                    st = r["stats"]
                    cases.append({
                        "mode": name, "n_periods": P, "first_path": first, "n_paths": 300,
                        "seed": 0x5EED0123456789AB, "initial_capital": 1000.0,
                        "gauss_mean": 0.5, "gauss_std": float(np.float32(0.83333)),
                        "n_bins": 100, "hist_lo": 0.0, "hist_hi": 20000.0, "below_threshold": 1000.0,
                        "final_bits": [int(x) for x in r["final"].view(np.uint32)],
                        "hist": [int(x) for x in r["hist"]],
                        "below": int(st.below), "underflow": int(st.underflow), "overflow": int(st.overflow),
                        "sum": st.sum, "sumsq": st.sumsq, "min": float(st.min), "max": float(st.max),
                    })
        with open(os.path.join(HERE, f"counter_stream_v{stream}.json"), "w") as f:
            json.dump({"table_bits_fnv1a": int(fnv1a(table.view(np.uint32))), "stream": stream, "cases": cases}, f)
    print("wrote fixtures")


def ref_callers_inputs(table):
    """The value sets tests/test_ref_callers_cpu.py feeds the reference's statistics helpers, and their thresholds."""
    final = O.counter_mc(O.make_params(O.MODE_TABLE, 120, 200000, 31, table=table))["final"]
    sets = [final, final[:1], final[:257], np.exp(np.random.default_rng(1).normal(7, 2, 50000)).astype(np.float32)]
    return [(v, (1000.0, float(np.median(v)), 0.0, 1e30)) for v in sets]


WRITER_RETURNS = [1.5, -2.25, 0.1, 1e-7, 12345.678, -0.0]  # tests/cpp/writers_check.cpp writes the same two vectors
WRITER_VALUES = [1000.0, 1015.0, 992.1625, 993.154663, 1.0e9, 3.4e38, 1.17549435e-38]


def ref_callers():
    import ctypes as C
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_ref_callers_cpu import REF_SO, load_ref
    L = load_ref()
    stats = []
    for v, thresholds in ref_callers_inputs(load_table()):
        mean, std = C.c_float(), C.c_float()
        L.ref_update_mean_std(v.ctypes.data_as(C.c_void_p), v.size, C.byref(mean), C.byref(std))
        below = [int(L.ref_update_count_below_min(v.ctypes.data_as(C.c_void_p), v.size, t)) for t in thresholds]
        stats.append({"n": int(v.size), "mean": float(mean.value), "std": float(std.value), "below": below})
    r = np.array(WRITER_RETURNS, dtype=np.float32)
    v = np.array(WRITER_VALUES, dtype=np.float32)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("outputs")
            L.ref_write_data_file(b"theirs.csv", r.ctypes.data_as(C.c_void_p), r.size, v.ctypes.data_as(C.c_void_p), v.size)
            L.ref_write_vector_file(b"outputs/theirs_vec.csv", v.ctypes.data_as(C.c_void_p), v.size)
            C.CDLL(None).fflush(None)
            data_file = open("outputs/theirs.csv").read()
            vector_file = open("outputs/theirs_vec.csv").read()
        finally:
            os.chdir(cwd)
    with open(os.path.join(HERE, "ref_callers.json"), "w") as f:
        json.dump({"source": os.path.relpath(REF_SO, ROOT), "statistics": stats, "data_file": data_file,
                   "vector_file": vector_file}, f, indent=1)
    print("wrote ref_callers.json")


def fnv1a(words):
    h = 0xCBF29CE484222325
    for w in np.asarray(words, dtype=np.uint32).tobytes():
        h = ((h ^ w) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


if __name__ == "__main__":
    if sys.argv[1:] == ["ref_callers"]:
        ref_callers()
    else:
        main()
