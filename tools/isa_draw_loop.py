"""The draw-block loop of a wave-walk kernel whose period loop is no single basic block (a rebalance branch per period, a
field block per second trip): for every instantiation of a kernel in a gfx950 .s file, the smallest backward-branch span
that holds at least 16 v_mad_u64_u32 (one Philox block), with its STATIC instruction counts -- both sides of every branch
inside the span are counted -- and the whole kernel's v_writelane / v_readlane (SGPRs spilled into VGPR lanes).  What
profiles/portfolio_cashflow_regimes/isa.txt lists beside tools/isa_table.py's rows.

usage: isa_draw_loop.py <file.s> <kernel name> [variant prefix]
"""
import os
import re
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_loops as L  # noqa: E402
import isa_table as T  # noqa: E402


def spans(body):
    """(label, first line, last line) of every backward branch of a kernel body."""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    for k, l in enumerate(body):
        p = l.split()
        if p and (p[0].startswith("s_cbranch") or p[0] == "s_branch") and labels.get(p[-1], k) < k:
            yield p[-1], labels[p[-1]], k


def opcodes(body, a, b):
    return Counter(x.split()[0] for x in body[a + 1:b + 1] if x.strip() and x.strip()[0] not in ";.")


def rows(path, kernel, want=""):
    lines = open(path).read().splitlines()
    prefix, symbols = T.instantiations(path, kernel, lines)
    for sym in symbols:
        variant = sym[len(prefix):]
        if not variant.startswith(want):
            continue
        body = L.kernel_body(lines, sym)
        found = [(b - a, t, opcodes(body, a, b)) for t, a, b in spans(body)]
        _, label, c = min((f for f in found if f[2].get("v_mad_u64_u32", 0) >= 16), key=lambda f: f[0])
        whole = opcodes(body, 0, len(body) - 1)
        count = lambda *heads: sum(n for k, n in c.items() if k.startswith(heads))  # noqa: E731
        yield (f"{kernel}{re.match(r'(I(?:L[a-z][0-9]+E)+)E', variant).group(1)}: draw-block loop {label}: VALU {count('v_')} LDS {count('ds_')} "
               f"v_cndmask {count('v_cndmask')} fma {count('v_fma', 'v_fmac')} v_mad_u64_u32 {c.get('v_mad_u64_u32', 0)} "
               f"lane moves inside {count('v_writelane', 'v_readlane')} | whole kernel: v_writelane {whole.get('v_writelane_b32', 0)} "
               f"v_readlane {whole.get('v_readlane_b32', 0)}")


if __name__ == "__main__":
    for line in rows(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ""):
        print(line)
