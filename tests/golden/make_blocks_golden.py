"""Writes tests/golden/blocks_v3.json: frozen final values of the circular block bootstrap (counter stream v3), from
the restatement in tests/blocks_reference.py over the CPU oracle.  tests/test_blocks_cpu.py regenerates the file's
content bit for bit; tests/test_blocks_gpu.py runs the device against it.

usage: python tests/golden/make_blocks_golden.py [--check]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "blocks_v3.json")
# (table, block_len, n_periods, n_paths)
CASES = [("bundled", 12, 360, 64), ("bundled", 1, 9, 16), ("7", 9, 73, 32), ("2049", 12, 49, 32)]


def generate():
    import numpy as np
    import blocks_reference as ref
    from oracle import oracle as O
    O.build()
    cases = []
    for key, L, P, n in CASES:
        final = ref.finals(O, ref.table_of(key), ref.SEED, ref.FIRST_PATH, n, P, L)
        cases.append({"table": key, "block_len": L, "n_periods": P, "n_paths": n,
                      "final_bits": [int(x) for x in final.view(np.uint32)]})
    return {"stream": 3, "seed": ref.SEED, "first_path": ref.FIRST_PATH, "initial_capital": ref.CAPITAL, "cases": cases}


if __name__ == "__main__":
    doc = generate()
    if "--check" in sys.argv:
        assert json.load(open(OUT)) == doc, "tests/golden/blocks_v3.json differs from the restatement"
        print("blocks_v3.json: ok")
    else:
        with open(OUT, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        print(OUT)
