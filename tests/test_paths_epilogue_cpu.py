"""What the compiled paths_kernel must keep, beside the loop counts tests/test_measurement_cpu.py pins:

* the Gaussian draw's residual angle is formed by v_bitop3_b32 (full rate), not by v_and_or_b32 (half rate);
* the Gaussian fast-divide kernel stays inside 64 VGPRs without scratch (eight waves per SIMD);
* the chunk loop around the period loop -- the chunk statistics' epilogue -- reduces over the wave with DPP row shifts
  and v_permlane*_swap, not through the LDS crossbar (ds_bpermute_b32), and divides (v_rcp_f64 and its train) only in
  the one block that handles a ragged chunk, which a full chunk branches around.

Read from the gfx950 assembly of the kernels as they compile now (tools/isa_loop_count.py); no GPU needed.
"""
import os
import re
import sys
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = {"gaussian": "ILi1ELi0ELb0E", "table": "ILi0ELi0ELb1E"}
DIVIDE_TRAIN = ("v_rcp_f64", "v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return open(I.emit_asm(str(tmp_path_factory.mktemp("isa_epilogue") / "smmc_kernels.s"))).read().splitlines()


def _symbol(variant):
    return "_ZN4smmc12_GLOBAL__N_112paths_kernel" + variant


def _body(lines, variant):
    beg = [i for i, l in enumerate(lines) if l.startswith(_symbol(variant))][0]
    fin = [i for i, l in enumerate(lines) if i > beg and "s_endpgm" in l][0]
    return lines[beg:fin + 1]


def _descriptor(lines, variant):
    """The .amdhsa_ directives of the kernel as {name: value}."""
    beg = [i for i, l in enumerate(lines) if l.strip().startswith(".amdhsa_kernel " + _symbol(variant))][0]
    end = [i for i, l in enumerate(lines) if i > beg and ".end_amdhsa_kernel" in l][0]
    return {l.split()[0]: l.split()[1] for l in lines[beg + 1:end] if l.strip().startswith(".amdhsa_")}


def _opcode(line):
    return re.sub(r"_e(32|64)$", "", line.split()[0])


def _blocks(body):
    """Basic blocks as (tag, [instruction lines]): a block starts at a label or a `; %bb.N:` line; the tag is that
    line and the comment lines that follow it (where the compiler says which loop the block belongs to)."""
    out = []
    for l in body:
        s = l.strip()
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", s):
            out.append([s, []])
        elif not out:
            continue
        elif s.startswith(";"):
            if not out[-1][1]:
                out[-1][0] += " " + s
        elif s and not s.startswith("."):
            out[-1][1].append(s)
    return out


def _chunk_loop_blocks(body):
    """The blocks of the depth-1 loop that holds the period loop, without the period loop's own."""
    blocks = _blocks(body)
    head = [t for t, _ in blocks if "Loop Header: Depth=1" in t and "Child Loop" in t]
    assert len(head) == 1, head
    name = re.match(r"^\.L(BB\d+_\d+):", head[0]).group(1)
    mine = [(t, ins) for t, ins in blocks if t == head[0] or f"in Loop: Header={name} Depth=1" in t]
    assert len(mine) > 8 and not any("Depth=2" in t for t, _ in mine)
    return mine


@pytest.mark.parametrize("mode", ["gaussian", "table"])
def test_period_loop_keeps_its_counts_and_the_angle_mask_is_a_bitop3(asm, mode):
    import bench
    import isa_loop_count as I
    variant, periods = I.VARIANTS[mode]
    assert variant == KERNELS[mode]
    lines = [l.strip() for l in _body(asm, variant)]
    start = [i for i, l in enumerate(lines) if "Inner Loop Header: Depth=2" in l][0]
    end = [i for i, l in enumerate(lines) if i > start and "s_cbranch_scc" in l][0]
    loop = [l for l in lines[start:end + 1] if l and l[0] not in ";."]
    c = Counter(_opcode(l) for l in loop)
    assert sum(n for k, n in c.items() if k.startswith("v_")) == bench.VALU_INSTS_PER_STEP[mode] * periods == {"gaussian": 70, "table": 84}[mode]
    assert sum(n for k, n in c.items() if k.startswith("ds_")) == periods
    assert "v_and_or_b32" not in c
    assert c["v_bitop3_b32"] == {"gaussian": 17, "table": 15}[mode]
    if mode == "gaussian":  # two draw pairs per block: (ub & mask) | 1.0f, truth table 0xEA, the mask a scalar
        masks = [l for l in loop if l.startswith("v_bitop3_b32") and "bitop3:0xea" in l]
        assert len(masks) == 2 and all(re.search(r", s\d+, 1\.0 bitop3:0xea$", l) for l in masks), masks
    assert not any(k in c for k in ("v_readlane_b32", "v_writelane_b32")) and not any(k.startswith("scratch_") for k in c)


def test_gaussian_kernel_fits_eight_waves_per_simd(asm):
    d = _descriptor(asm, KERNELS["gaussian"])
    assert int(d[".amdhsa_next_free_vgpr"]) <= 64
    assert int(d[".amdhsa_private_segment_fixed_size"]) == 0
    assert not any(l.split()[0].startswith("scratch_") for l in _body(asm, KERNELS["gaussian"]) if l.strip() and l.strip()[0] not in ";.")


@pytest.mark.parametrize("mode", ["gaussian", "table"])
def test_chunk_epilogue_reduces_without_lds_and_divides_only_a_ragged_chunk(asm, mode):
    body = _body(asm, KERNELS[mode])
    assert int(_descriptor(asm, KERNELS[mode])[".amdhsa_private_segment_fixed_size"]) == 0
    blocks = _chunk_loop_blocks(body)
    c = Counter(_opcode(l) for _, ins in blocks for l in ins)
    assert "ds_bpermute_b32" not in c and "ds_swizzle_b32" not in c
    # both sums in one register pair: one v_permlane32_swap and one v_permlane16_swap per 32-bit half, four row shifts
    assert c["v_permlane32_swap_b32"] == 2 and c["v_permlane16_swap_b32"] == 2 and c["v_mov_b32_dpp"] == 8
    assert c["s_barrier"] == 1
    # the wave's two results (lane 0, lane 32) go to LDS in ONE store
    assert c["ds_write_b64"] == 1 and c["ds_write_b32"] == 0 and c["ds_write2_b64"] == 0
    # the IEEE divides: two (mean, mean square), in ONE block, which a conditional branch in front of it skips for
    # a full chunk
    with_div = [i for i, (_, ins) in enumerate(blocks) if any(_opcode(l) in DIVIDE_TRAIN for l in ins)]
    assert len(with_div) == 1, [blocks[i][0] for i in with_div]
    ragged = Counter(_opcode(l) for l in blocks[with_div[0]][1])
    assert ragged["v_rcp_f64"] == 2 and c["v_rcp_f64"] == 2
    before = blocks[with_div[0] - 1][1]
    assert before[-1].startswith("s_cbranch_"), before[-3:]  # conditional: on the exec mask, or scalar where the chunk index is
    # the full chunk's path: two scalings by 2^-8 (v_ldexp_f64 by -8, or a multiply) and no divide
    others = [l for i, (_, ins) in enumerate(blocks) if i != with_div[0] for l in ins]
    scaled = [l for l in others if (l.startswith("v_ldexp_f64") and l.rstrip().endswith(", -8")) or (l.startswith("v_mul_f64") and "0x3f700000" in l)]
    assert len(scaled) == 2, scaled
