"""One row per instantiation of a kernel in a gfx950 .s file: registers, scratch, the period loop (the largest
innermost loop, tools/isa_loops.py) with its scalar loads, the instruction count and isa_loop_count's fingerprint.
What profiles/{checkpoints,cashflow,excursions}/isa.txt and the tables of their READMEs are made of; with --json
the rows can be kept and two builds compared (--against).

usage: isa_table.py <file.s | source.hip> <kernel name> [--json | --against rows.json]
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_loop_count as I  # noqa: E402
import isa_loops as L  # noqa: E402


def instantiations(path, kernel, lines=None):
    """(symbol prefix, symbols) of every instantiation of smmc::(anon)::<kernel> in the .s file: names only, which is all
    tests/test_feature_matrix_cpu.py needs of rows() -- the per-row loop analysis below takes seconds per kernel."""
    lines = open(path).read().splitlines() if lines is None else lines
    prefix = f"_ZN4smmc12_GLOBAL__N_1{len(kernel)}{kernel}"
    return prefix, [l.split(":")[0] for l in lines if l.startswith(prefix) and ": ; @" in l]


def rows(path, kernel):
    lines = open(path).read().splitlines()
    prefix, symbols = instantiations(path, kernel, lines)
    out = {}
    for sym in symbols:
        variant = sym[len(prefix):]
        meta = {}
        for l in lines:
            m = re.match(r"\s*\.set " + re.escape(sym) + r"\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size), (\d+)", l)
            if m:
                meta[m.group(1)] = int(m.group(2))
        loops = L.loops(L.kernel_body(lines, sym))
        label, c = max(loops, key=lambda lc: sum(lc[1].values()))
        out[kernel + variant] = {
            "vgpr": meta["num_vgpr"], "agpr": meta["num_agpr"], "sgpr": meta["numbered_sgpr"],
            "private_segment": meta["private_seg_size"], "period_loop": list(L.summary(c)),
            "scalar_loads": {k: n for k, n in sorted(c.items()) if k.startswith("s_load") or k.startswith("s_buffer_load")},
            "instructions": len(I.kernel_opcodes(path, variant, kernel)), "fingerprint": I.fingerprint(path, variant, kernel)}
    return out


if __name__ == "__main__":
    import argparse
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("kernel")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--against", metavar="ROWS.json")
    a = ap.parse_args()
    path, kernel = a.path, a.kernel
    if not path.endswith(".s"):
        with tempfile.TemporaryDirectory() as tmp:
            table = rows(I.emit_asm(os.path.join(tmp, os.path.basename(path) + ".s"), os.path.basename(path)), kernel)
    else:
        table = rows(path, kernel)
    if a.json:
        print(json.dumps(table, indent=1, sort_keys=True))
        sys.exit(0)
    before = json.load(open(a.against)) if a.against else None
    for name, r in table.items():
        line = (f"{name}: vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} private_segment {r['private_segment']} "
                f"period loop {tuple(r['period_loop'])} scalar loads {r['scalar_loads']} instructions {r['instructions']} "
                f"fingerprint {r['fingerprint'][:16]}")
        if before is not None:
            b = before[name]
            same = all(b[k] == r[k] for k in ("agpr", "private_segment", "period_loop", "scalar_loads")) and r["vgpr"] <= b["vgpr"]
            line += ("  | conditions hold" if same else "  | CONDITION BROKEN") + \
                    (", fingerprint identical" if b["fingerprint"] == r["fingerprint"] else
                     f", fingerprint differs (before: {b['instructions']} instructions, vgpr {b['vgpr']})")
        print(line)
