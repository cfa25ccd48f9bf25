"""paths_hi_kernel (launches whose paths share the id bits 63..32) without a GPU: the staged form of the first Philox
rounds restated in numpy and held to the oracle's Philox4x32-10, and the sibling kernels as they compile now.

Counter stream v3 counts (block, path_lo, path_hi, mode tag).  With the block AND path_hi wave-uniform
(smmc_kernels.hip, philox4x32_10<kPhiloxUniformHi>) the rounds 0 .. 3 split into
    a scalar loop invariant        M1 path_hi
    a per-path hoisted part        n0 of round 0 and (H, L) = M0 n0
    a per-block scalar part        M0 blk, round 1's M1 n2 and its n0, round 2's M0 n0, the scalar halves of four XORs
    a per-lane part                one XOR in round 1, one multiply and two XORs in round 2, round 3 with a scalar pair
and six plain rounds follow.  Equal words are required for every combination below.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def _mul(m, x):
    """(hi, lo) of the 32 x 32 -> 64 bit product, x a Python int or a uint32 array."""
    p = np.uint64(m) * np.asarray(x, dtype=np.uint64)
    return (p >> np.uint64(32)).astype(np.uint32), (p & np.uint64(MASK)).astype(np.uint32)


def staged_philox(blk, path_lo, path_hi, tag, key):
    """The words of counter (blk, path_lo[i], path_hi, tag) as philox4x32_10<kPhiloxUniformHi> stages them."""
    u32 = np.uint32
    k0 = [u32((key[0] + r * W0) & MASK) for r in range(10)]
    k1 = [u32((key[1] + r * W1) & MASK) for r in range(10)]
    path_lo = np.asarray(path_lo, dtype=np.uint32)
    # scalar loop invariant: round 0's M1 c2
    si_h1, si_l1 = _mul(M1, path_hi)
    # per path, hoisted: round 0's n0 and round 1's M0 n0
    n0 = si_h1 ^ path_lo ^ k0[0]
    H, L = _mul(M0, n0)
    # per block, scalar: round 0's M0 c0 and n2, round 1's M1 n2 and n0 (all scalar), round 2's M0 n0
    h0, c3 = _mul(M0, blk)
    n2_s = h0 ^ u32(tag) ^ k1[0]
    q_h1, q_l1 = _mul(M1, n2_s)
    n0_s = q_h1 ^ si_l1 ^ k0[1]
    pair2_r1 = c3 ^ k1[1]
    r_h0, r_l0 = _mul(M0, n0_s)
    pair0_r2 = q_l1 ^ k0[2]
    pair2_r2 = r_h0 ^ k1[2]
    pair2_r3 = r_l0 ^ k1[3]
    assert all(np.ndim(s) == 0 for s in (n2_s, n0_s, pair2_r1, pair0_r2, pair2_r2, pair2_r3))
    # per lane
    n2 = H ^ pair2_r1                      # round 1: one XOR
    p_h1, p_l1 = _mul(M1, n2)              # round 2: one multiply, two XORs
    c0, c2 = p_h1 ^ pair0_r2, L ^ pair2_r2
    c1 = p_l1
    a_h0, a_l0 = _mul(M0, c0)              # round 3: c3 = lo of round 2's scalar product sits in the pair
    b_h1, b_l1 = _mul(M1, c2)
    c0, c2 = b_h1 ^ c1 ^ k0[3], a_h0 ^ pair2_r3
    c1, c3 = b_l1, a_l0
    for r in range(4, 10):
        a_h0, a_l0 = _mul(M0, c0)
        b_h1, b_l1 = _mul(M1, c2)
        c0, c2 = b_h1 ^ c1 ^ k0[r], a_h0 ^ c3 ^ k1[r]
        c1, c3 = b_l1, a_l0
    return np.stack([c0, c1, c2, c3], axis=1)


def test_round_algebra_matches_the_oracle():
    from oracle import oracle as O
    rng = np.random.default_rng(20240611)
    lo = np.concatenate([np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32),
                         rng.integers(0, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32)])
    for key in ((2024, 0), (0x456789AB, 0x5EED0123)):
        for tag in (0, 1):
            for hi in (0, 1, 5, 0xFFFFFFFF):
                for blk in (0, 1, 89, 0xFFFFFFFF):
                    ctr = np.empty((lo.size, 4), dtype=np.uint32)
                    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = blk, lo, hi, tag
                    want = O.philox4x32_10_bulk(ctr, key)
                    got = staged_philox(blk, lo, hi, tag, key)
                    assert np.array_equal(got, want), (key, tag, hi, blk, np.flatnonzero((got != want).any(axis=1))[:4])


FORM_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "smmc_internal.h"
int main(int argc, char **argv) {  // mode stream table_len first_path n_paths [switch] -> paths_form
  smmc::KernelArgs a{};
  if (argc == 7) smmc::paths_uniform_hi().store(std::atoi(argv[6]));  // what smmc_set_uniform_hi stores
  a.mode = std::atoi(argv[1]);
  a.stream = std::atoi(argv[2]);
  a.table_len = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
  a.first_path = std::strtoull(argv[4], nullptr, 10);
  a.n_paths = std::strtoull(argv[5], nullptr, 10);
  std::printf("%d\n", smmc::paths_form(a));
  return argc == 6 || argc == 7 ? 0 : 1;
}
"""


def test_host_rule_for_the_form(tmp_path):
    """smmc::paths_form, what launch_paths and smmc_engine_paths_form both ask, as a stand-alone host program."""
    import subprocess
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src, exe = tmp_path / "form.cpp", str(tmp_path / "form")
    src.write_text(FORM_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc"), str(src), "-o", exe])

    def form(mode, stream, table_len, first, n, switch=None):
        args = [exe, str(mode), str(stream), str(table_len), str(first), str(n)] + ([str(switch)] if switch is not None else [])
        return int(subprocess.check_output(args))

    G, T = 1, 0  # SMMC_MODE_GAUSSIAN, SMMC_MODE_TABLE
    assert form(G, 3, 0, 0, 100_000_000) == 1 and form(T, 3, 1127, 0, 100_000_000) == 1
    assert form(T, 3, 2048, 5, 10) == 1 and form(T, 3, 2049, 5, 10) == 0          # dense tables only
    assert form(G, 2, 0, 0, 10) == 0 and form(T, 2, 1127, 0, 10) == 0              # stream v2
    assert form(G, 3, 0, 0, 1 << 32) == 1 and form(G, 3, 0, 0, (1 << 32) + 1) == 0  # a whole multiple, one more
    assert form(G, 3, 0, (1 << 32) - 10, 10) == 1 and form(G, 3, 0, (1 << 32) - 10, 11) == 0
    assert form(G, 3, 0, (1 << 40) + 12345, 1000) == 1
    assert form(G, 3, 0, (1 << 64) - 10, 10) == 1 and form(G, 3, 0, (1 << 64) - 10, 11) == 0  # a sum that wraps
    assert form(G, 3, 0, 1, (1 << 64) - 1) == 0 and form(G, 3, 0, 0, 0) == 0
    assert form(G, 3, 0, 0, 10, switch=0) == 0 and form(G, 3, 0, 0, 10, switch=1) == 1
    assert form(G, 3, 0, (1 << 32) - 10, 11, switch=1) == 0  # the switch never forces the form on


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa_hi") / "smmc_kernels.s"))


@pytest.mark.parametrize("mode,valu,lds", [("gaussian", 68, 4), ("table", 82, 8)])
def test_sibling_loops_as_they_compile_now(asm, mode, valu, lds):
    import isa_loop_count as I
    variant, periods = I.HI_VARIANTS[mode]
    c = I.count(asm, variant, I.HI_KERNEL)
    assert I.valu(c) == valu and I.lds(c) == lds == periods, dict(c)
    if mode == "gaussian":
        assert c["v_mad_u64_u32"] == 15, dict(c)
    # two instructions fewer than the generic kernel's loop, one of them a multiply
    g = I.count(asm, I.VARIANTS[mode][0])
    assert I.valu(g) - I.valu(c) == 2 and g["v_mad_u64_u32"] - c["v_mad_u64_u32"] == 1
    # the range-checked divide adds exactly the two compares per block that it adds to the generic kernel
    chk = I.count(asm, I.HI_VARIANTS[mode + "_checked"][0], I.HI_KERNEL)
    g_chk = I.count(asm, I.VARIANTS[mode + "_checked"][0])
    added = {k: chk[k] - c[k] for k in set(chk) | set(c) if k.startswith("v_") and chk[k] != c[k]}
    g_added = {k: g_chk[k] - g[k] for k in set(g_chk) | set(g) if k.startswith("v_") and g_chk[k] != g[k]}
    assert I.valu(chk) - I.valu(c) == 2 and added == g_added, (added, g_added)
    assert all(k.startswith("v_cmp") for k in added), added


def _metadata(asm_path, symbol):
    text = open(asm_path).read()
    m = re.search(r"\.name:\s+" + re.escape(symbol) + r"\s*\n(.*?)\.wavefront_size:", text, re.S)
    assert m, symbol
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", m.group(1))}


@pytest.mark.parametrize("div", ["gaussian", "gaussian_checked", "gaussian_exact"])
def test_gaussian_siblings_fit_eight_waves_per_simd(asm, div):
    import isa_loop_count as I
    sym = f"_ZN4smmc12_GLOBAL__N_1{len(I.HI_KERNEL)}{I.HI_KERNEL}{I.HI_VARIANTS[div][0]}EEvNS_10KernelArgsEj"
    md = _metadata(asm, sym)
    assert md["vgpr_count"] <= 64 and md["private_segment_fixed_size"] == 0, md
