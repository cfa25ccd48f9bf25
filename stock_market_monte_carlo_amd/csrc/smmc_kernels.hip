// smmc_kernels.hip -- gfx950 kernels of the Monte-Carlo returns engine.
//
// Replaces mc_simulations_gpu_kernel (reference src/simulations.cu:112-152) and
// mc_simulations_gpu_kernel_reduceBlock (:185-247); written from scratch for CDNA4
// (wave64, LDS-staged table, wave shuffles + LDS for reductions, no MFMA: the path
// has no contraction).  The arithmetic follows the CPU semantics
// (src/simulations.cpp:14-16, three binary32 roundings per period), not the
// reference GPU kernel's `total += total * (r * 0.01f)`.
//
// Bound: VALU issue (Philox4x32-10 + the dependent compounding chain).  HBM sees
// 4 B per path (the coalesced final-value store) or nothing (statistics only).
//
// Build with -ffp-contract=off: every fused multiply-add is an explicit
// __builtin_fmaf; results must be bit-identical to oracle/smmc_oracle.c engine (C).
#include <hip/hip_runtime.h>

#include "smmc_device.h"
#include "smmc_internal.h"

namespace smmc {
namespace {

using namespace dev;

constexpr uint32_t kPhiloxM0 = 0xD2511F53u;
constexpr uint32_t kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kWeyl0 = 0x9E3779B9u;
constexpr uint32_t kWeyl1 = 0xBB67AE85u;

// Philox4x32-10 (Salmon et al., SC'11).  The key schedule is wave-uniform and
// lives in SGPRs; per round the lanes pay two 32x32->64 multiplies
// (v_mad_u64_u32) and two three-input XORs (v_bitop3_b32).
// kPhiloxUniformBlock: the caller's c0 (counter stream v3: the block index) is wave-uniform and c1, c2 (the
// path) do not change along the caller's loop.  Rounds 0 and 1 then cost two VALU instructions:
//   round 0: M0 c0 is a scalar product, M1 c2 per-path constant; n0 = hi(M1 c2) ^ c1 ^ k0 is
//            per-path constant (hoisted out of the period loop), n2 = hi(M0 c0) ^ c3 ^ k1 scalar;
//   round 1: M0 n0 per-path constant (hoisted), M1 n2 a scalar product; each XOR has ONE per-lane
//            term and a scalar pair, which is formed on the SALU (opaque to the compiler, which
//            otherwise re-associates it apart: an instruction reads at most one SGPR, so a v_bitop3
//            with two scalar terms costs a v_mov); round 2's first XOR likewise.
// With the counter (path, block, mode) of stream v2 the same rounds cost four (one multiply among them).
// Issue rates on gfx950 (tools/ubench_ops.hip, profiles/r04/ubench_ops.jsonl): a VALU instruction that reads an
// SGPR operand issues at HALF rate (v_xor_b32 2.1 clk per wave with VGPR or literal operands, 4.1 with one
// SGPR; v_mul_f32, v_add_u32 the same), and v_bitop3_b32 takes 2.7 clk with three VGPRs against 4.1 with a
// scalar round key.  The wave-uniform constants the period loops read in every block -- the Philox round keys
// of the three-input XORs, the Gaussian draw's additive term -- are therefore held in VGPRs (made opaque to
// the compiler, which would otherwise put every uniform value into an SGPR): 16 + 1 registers per lane, set
// up once per kernel.  Values that change from block to block (the scalarised first rounds) stay scalar: a
// v_mov into a VGPR costs what the SGPR operand costs.
struct DrawRegs {
  uint32_t k0[10], k1[10];  // Philox round keys key + r * Weyl, as VGPRs
  float shift100;           // 100.0f + gauss_mean
};
__device__ __forceinline__ DrawRegs make_draw_regs(const KernelArgs &k) {
  DrawRegs d;
  uint32_t a = k.key0, b = k.key1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    d.k0[r] = a;
    d.k1[r] = b;
    asm("" : "+v"(d.k0[r]));  // not volatile: set up once, outside the loops; unused ones disappear
    asm("" : "+v"(d.k1[r]));
    a += kWeyl0;
    b += kWeyl1;
  }
  d.shift100 = k.gauss_shift100;
  asm("" : "+v"(d.shift100));
  return d;
}

// kPhiloxUniformHi (paths_hi_kernel): c2 (the path's id bits 63..32) is wave-uniform as well -- every path of a
// launch that does not reach across a multiple of 2^32 has the same.  Then
//   round 0: M1 c2 is a scalar loop invariant too; n0 = hi(M1 c2) ^ c1 ^ k0 stays per-path constant, n2 scalar;
//   round 1: (H, L) = M0 n0 per-path constant (hoisted); M1 n2 a scalar product; n0 is ALL scalar, n2 = H ^ pair;
//   round 2: M0 n0 is a scalar product, M1 n2 one v_mad_u64_u32; n0 = hi(M1 n2) ^ pair, n2 = L ^ pair;
//   round 3: four VALU instructions like the later rounds, n2's pair c3 ^ k1 scalar (c3 = lo of round 2's scalar product).
// Five VALU instructions for rounds 1 .. 2 instead of six, one multiply fewer among them, and two hoisted
// registers per path (H, L) instead of three.  A scalar pair handed a per-lane value would silently read lane 0's:
// the form is only for callers whose c0 and c2 come from scalar registers.
enum PhiloxForm { kPhiloxGeneric = 0, kPhiloxUniformBlock = 1, kPhiloxUniformHi = 2 };

template <PhiloxForm kForm = kPhiloxGeneric>
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, const DrawRegs &dr, uint32_t (&out)[4]) {
  constexpr bool kUniformFirst = kForm == kPhiloxUniformBlock;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(kPhiloxM0) * c0;
    const uint64_t p1 = static_cast<uint64_t>(kPhiloxM1) * c2;
    const uint32_t h0 = static_cast<uint32_t>(p0 >> 32), h1 = static_cast<uint32_t>(p1 >> 32);
    uint32_t n0, n2;
    if (r == 1 && kForm == kPhiloxUniformHi) {
      n0 = (h1 ^ k0) ^ c1;  // scalar throughout
      uint32_t pair2 = c3 ^ k1;
      asm("" : "+s"(pair2));
      n2 = pair2 ^ h0;  // h0 = H
    } else if (r == 2 && kForm == kPhiloxUniformHi) {
      uint32_t pair0 = c1 ^ k0, pair2 = h0 ^ k1;
      asm("" : "+s"(pair0));
      asm("" : "+s"(pair2));
      n0 = pair0 ^ h1;
      n2 = pair2 ^ c3;  // c3 = L
    } else if (r == 3 && kForm == kPhiloxUniformHi) {
      uint32_t pair2 = c3 ^ k1;
      asm("" : "+s"(pair2));
      n0 = xor3(h1, c1, dr.k0[r]);
      n2 = pair2 ^ h0;
    } else if (r == 1 && kUniformFirst) {
      uint32_t pair0 = h1 ^ k0, pair2 = c3 ^ k1;  // scalar ^ scalar
      asm("" : "+s"(pair0));
      asm("" : "+s"(pair2));
      n0 = pair0 ^ c1;
      n2 = pair2 ^ h0;
    } else if (r == 2 && kUniformFirst) {  // c1 = lo(M1 n2 of round 0) is still scalar
      uint32_t pair0 = c1 ^ k0;
      asm("" : "+s"(pair0));
      n0 = pair0 ^ h1;
      n2 = xor3(h0, c3, dr.k1[r]);
    } else if (r < 2) {  // plain XORs: invariant and scalar parts are the compiler's to hoist and to scalarise
      n0 = (h1 ^ k0) ^ c1;
      n2 = (h0 ^ k1) ^ c3;
    } else {
      n0 = xor3(h1, c1, dr.k0[r]);
      n2 = xor3(h0, c3, dr.k1[r]);
    }
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += kWeyl0;
    k1 += kWeyl1;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// N independent Philox4x32-10 blocks, round by round: the source order the compiler keeps is then
// N interleaved dependency chains (left to schedule two calls of philox4x32_10 it runs one after the
// other), so that one wave has 2 N multiplies and 2 N XORs in flight per round instead of 2 + 2.
// A wave alone can issue a dependent VALU instruction only every 4-8 cycles; below ~6 waves per SIMD
// this instruction-level parallelism is what fills the issue slots.
template <int N, bool kUniformFirst = false>
__device__ __forceinline__ void philox4x32_10_multi(uint32_t (&c)[N][4], uint32_t k0, uint32_t k1, const DrawRegs &dr) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint64_t p0[N], p1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      p0[i] = static_cast<uint64_t>(kPhiloxM0) * c[i][0];
      p1[i] = static_cast<uint64_t>(kPhiloxM1) * c[i][2];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const uint32_t h0 = static_cast<uint32_t>(p0[i] >> 32), h1 = static_cast<uint32_t>(p1[i] >> 32);
      uint32_t n0, n2;  // rounds 0 .. 2: see philox4x32_10
      if (r == 1 && kUniformFirst) {
        uint32_t pair0 = h1 ^ k0, pair2 = c[i][3] ^ k1;
        asm("" : "+s"(pair0));
        asm("" : "+s"(pair2));
        n0 = pair0 ^ c[i][1];
        n2 = pair2 ^ h0;
      } else if (r == 2 && kUniformFirst) {
        uint32_t pair0 = c[i][1] ^ k0;
        asm("" : "+s"(pair0));
        n0 = pair0 ^ h1;
        n2 = xor3(h0, c[i][3], dr.k1[r]);
      } else if (r < 2) {
        n0 = (h1 ^ k0) ^ c[i][1];
        n2 = (h0 ^ k1) ^ c[i][3];
      } else {
        n0 = xor3(h1, c[i][1], dr.k0[r]);
        n2 = xor3(h0, c[i][3], dr.k1[r]);
      }
      c[i][1] = static_cast<uint32_t>(p1[i]);
      c[i][3] = static_cast<uint32_t>(p0[i]);
      c[i][0] = n0;
      c[i][2] = n2;
    }
    k0 += kWeyl0;
    k1 += kWeyl1;
  }
}

// Box-Muller of counter stream v2 through two small LDS tables (generated by
// tools/gen_bm_tables.py, staged by the Gaussian kernels at LDS offset 0):
//   [0, 16.5 KiB)       radius: 2 sides x 33 octaves x 16 sub-intervals x {c0, c1, c2, c3}
//   [16.5, 18.5 KiB)    trig:   256 x {cos, sin}(2 pi i / 256)
// r = sqrt(-2 ln U) needs no log and no sqrt: the distance w of the uniform from the end of
// (0,1) it is nearer to is converted to binary32 (v_cvt_f32_u32 of 2w+1); the float's exponent is
// the octave, its top four mantissa bits the sub-interval, the other 19 the cubic's argument.
// The angle 2 pi ub / 2^32 is the table angle of its top 8 bits (rounded) plus |delta| <= pi/256,
// rotated in with sin(delta) = delta (1 - delta^2/6), cos(delta) = 1 - delta^2/2.  Integer steps
// and single IEEE operations only: bit-identical to the oracle's C version.
constexpr uint32_t kBmRadiusEntries = 1056, kBmTrigEntries = 256;
constexpr uint32_t kBmFloats = kBmRadiusEntries * 4 + kBmTrigEntries * 2;
// counter stream v3 (the default Gaussian draw): 2 x 256 radius bins (8 KiB), 2048 sectors (16 KiB)
// (kBm3SubBits, kBm3TrigBits, kBm3AngleK, kBm3AngleC: smmc_internal.h, checked against the generated tables)
constexpr uint32_t kBm3RadiusEntries = 64u << kBm3SubBits, kBm3TrigEntries = 1u << kBm3TrigBits;
constexpr uint32_t kBm3Floats = kBm3RadiusEntries * 4 + kBm3TrigEntries * 2;  // as they lie in global memory
// ... and in LDS (stage_tables): the radius bin's byte offset is (bits >> 16) & kBm3RadiusMask of the
// binary32 pattern of the SIGNED distance -- exponent's low five bits and three mantissa bits at
// [4, 12), the sign (the side) left where the shift puts it, bit 15 -- so side 0 lies at [0, 4 KiB) and
// side 1 at [32, 36 KiB); the angle table fills [4, 20 KiB) between them, [20, 32 KiB) stays unused.
// 36 KiB per workgroup instead of 24 are four workgroups of paths_kernel per CU instead of six (the same speed
// at 256 threads each, measured with a padded allocation, profiles/r02/ab_lds_pad.txt; two per CU lose 17 %).
// paths_kernel puts EIGHT waves on one copy (paths_halves): four workgroups are then 8 waves per SIMD instead of
// 4, which takes 6.6 % of the launch's clocks and, the chip holding 2.03 instead of 2.13 GHz under it, 1.95 % of
// the headline step's time (13.16 -> 12.91 ms, profiles/wide_groups/ab_wide_groups.txt).
constexpr uint32_t kBm3RadiusMask = 0x8000u | ((32u << kBm3SubBits) - 1u) << 4;
constexpr uint32_t kBm3Side1Bytes = 0x8000u, kBm3SideBytes = (32u << kBm3SubBits) * 16u;
constexpr uint32_t kBm3TrigBytes = kBm3SideBytes;                     // LDS byte address of the angle table
constexpr uint32_t kBm3LdsWords = (kBm3Side1Bytes + kBm3SideBytes) / 4u;
static_assert(kBm3TrigBytes + kBm3TrigEntries * 8u <= kBm3Side1Bytes, "angle table must fit between the radius sides");
// The kernels' kMode template argument: SMMC_MODE_TABLE (0) and SMMC_MODE_GAUSSIAN (1) are counter
// stream v3; kModeGaussianV2 and kModeTableV2 are stream v2 (SMMC_FLAG_STREAM_V2: its counter layout
// and, in Gaussian mode, its draw).  The Philox counter's mode word is 0 for table draws and 1 for
// Gaussian draws in both streams.
constexpr int kModeGaussianV2 = 2, kModeTableV2 = 3;
constexpr bool is_table(int mode) { return mode == SMMC_MODE_TABLE || mode == kModeTableV2; }
// Counter stream v3 (SMMC_MODE_TABLE, SMMC_MODE_GAUSSIAN) counts Philox blocks in the counter's FIRST
// word, (block, path_lo, path_hi, mode); stream v2 (the ...V2 modes) in its third, (path_lo, path_hi,
// block, mode).  With the block first, a wave-uniform block index and a path that does not change
// along the period loop the first two Philox rounds cost two VALU instructions instead of four
// (philox4x32_10).
constexpr bool counter_v3(int mode) { return mode == SMMC_MODE_TABLE || mode == SMMC_MODE_GAUSSIAN; }
constexpr uint32_t mode_tag(int mode) { return is_table(mode) ? 0u : 1u; }
constexpr uint32_t bm_floats(int mode) { return mode == kModeGaussianV2 ? kBmFloats : kBm3Floats; }
// LDS words the mode's Box-Muller tables take (what follows them starts there)
constexpr uint32_t bm_lds_words(int mode) { return mode == kModeGaussianV2 ? kBmFloats : kBm3LdsWords; }

// The two draws fma(r * scale, cos(theta), shift), fma(r * scale, sin(theta), shift), in two steps so
// that several of them can be in flight at once: bm_issue does the integer work and starts the two LDS
// gathers, bm_finish evaluates the cubic and rotates.
struct BmPending {
  float4 kr;      // the radius cubic of the uniform's bin
  float2 cs;      // (cos, sin) of the table angle
  float x;        // the cubic's argument
  float sd, cd;   // sin and cos of the residual angle
};

__device__ __forceinline__ BmPending bm_issue(const float *lds_bm, uint32_t ua, uint32_t ub) {
  BmPending p;
  const uint32_t mask = static_cast<uint32_t>(static_cast<int32_t>(ua) >> 31);  // all ones when U >= 1/2
  const uint32_t w1 = ((ua ^ mask) << 1) | 1u;                                   // 2 w + 1: odd
  const uint32_t bits = __float_as_uint(static_cast<float>(w1));                 // exponent 127 .. 159
  const uint32_t entry = (mask & 528u) + (bits >> 19) - (127u << 4);
  p.x = __uint_as_float(0x3f800000u | ((bits << 4) & 0x007ffff0u)) - 1.5f;
  p.kr = reinterpret_cast<const float4 *>(lds_bm)[entry];

  const uint32_t i = (ub + 0x00800000u) >> 24;
  const int32_t d = static_cast<int32_t>(ub << 8) >> 8;  // low 24 bits, sign-extended
  const float delta = static_cast<float>(d) * 0x1.921fb6p-30f;
  const float d2 = delta * delta;
  p.sd = delta * __builtin_fmaf(d2, -0x1.555556p-3f, 1.0f);
  p.cd = __builtin_fmaf(d2, -0.5f, 1.0f);
  p.cs = reinterpret_cast<const float2 *>(lds_bm + kBmRadiusEntries * 4)[i];
  return p;
}

__device__ __forceinline__ void bm_finish(const BmPending &p, float scale, float shift, float &d_cos, float &d_sin) {
  const float r = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(p.kr.w, p.x, p.kr.z), p.x, p.kr.y), p.x, p.kr.x);
  const float rs = r * scale;
  const float ct = __builtin_fmaf(-p.cs.y, p.sd, p.cs.x * p.cd);
  const float st = __builtin_fmaf(p.cs.x, p.sd, p.cs.y * p.cd);
  d_cos = __builtin_fmaf(rs, ct, shift);
  d_sin = __builtin_fmaf(rs, st, shift);
}

__device__ __forceinline__ void box_muller_scaled(const float *lds_bm, uint32_t ua, uint32_t ub, float scale,
                                                  float shift, float &d_cos, float &d_sin) {
  bm_finish(bm_issue(lds_bm, ua, ub), scale, shift, d_cos, d_sin);
}

// Counter stream v3: the same construction with cheaper arithmetic (6 instead
// of 16.5 VALU per draw).  The first word read as int32 IS the signed distance of the uniform from
// the nearer end of (0, 1); one v_cvt_f32_i32 turns it into a float f whose pattern holds everything:
// the radius bin is the top half of the pattern under a mask -- exponent's low five bits and three
// mantissa bits, the octaves stored rotated, the side left where the float has its sign (one SDWA
// v_and reading the upper word) -- and the cubic is evaluated in f itself (the coefficients carry the
// bin's position, the octave's powers of two, the sign and the factor std).  The angle is the low 30
// bits of the second word: its sector times 8 is again one masked read of the upper word, the table
// has 2048 entries at the MIDDLE of their sectors, and the residual angle -- low bits OR-ed into 1.0f,
// one fma, no conversion -- is small enough for a first-order rotation (c - s delta, s + c delta) (the
// table carries the factor that keeps the mean square length 1); and the draw is the MULTIPLIER
// itself, fma(r std, cos theta, 100 + mean).
struct Bm3Pending {
  float4 kr;
  float2 cs;
  float f, delta;
};

__device__ __forceinline__ Bm3Pending bm3_issue(const float *lds_bm, uint32_t ua, uint32_t ub) {
  Bm3Pending p;
  static_assert(23u - kBm3SubBits - 4u == 16u, "the bin's offset is the top half of the float's pattern");
  p.f = static_cast<float>(static_cast<int32_t>(ua));          // |f| <= 2^31; pattern 0 reads bin 0 (u = 2^-33)
  const uint32_t off = (__float_as_uint(p.f) >> 16) & kBm3RadiusMask;
  (void)lds_bm;
  const f32x4_t kr = lds_load_at<f32x4_t>(off);
  p.kr = make_float4(kr.x, kr.y, kr.z, kr.w);

  constexpr uint32_t kRes = kBm3AngleBits - kBm3TrigBits;      // residual bits below the sector
  static_assert(kRes - 3u == 16u, "sector * 8 is the word's upper half under a mask");
  const uint32_t aoff = (ub >> 16) & ((kBm3TrigEntries - 1u) << 3);  // sector * 8, no rounding add
  // residual angle from the sector's middle, (low bits - half a sector) 2 pi / 2^30: the low bits as the
  // mantissa of a float in [1, 1 + 2^-4), then one fma
  // (ub & mask) | 1.0f as ONE v_bitop3_b32 (truth table 0xEA): the only three-input logic opcode that issues at
  // full rate on gfx950 -- v_and_or_b32, which the compiler selects for the plain expression (and for a bitop3 of
  // two constants, hence the opaque mask), takes a half-rate slot like every other VOP3-only integer operation.
  // The mask stays scalar: one constant-bus read beside the inline constant, no register.
  uint32_t res_mask = (1u << kRes) - 1u;
  asm("" : "+s"(res_mask));
  const float ya = __uint_as_float(__builtin_amdgcn_bitop3_b32(ub, res_mask, 0x3f800000u, 0xEA));
  p.delta = __builtin_fmaf(ya, kBm3AngleK, -kBm3AngleC);
  const f32x2_t cs = lds_load_at<f32x2_t>(aoff + kBm3TrigBytes);
  p.cs = make_float2(cs.x, cs.y);
  return p;
}

// The staged radius coefficients carry the factor std (stage_tables): the cubic IS r std.
__device__ __forceinline__ void bm3_finish(const Bm3Pending &p, float shift, float &d_cos, float &d_sin) {
  const float rs = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(p.kr.w, p.f, p.kr.z), p.f, p.kr.y), p.f, p.kr.x);
  const float ct = __builtin_fmaf(-p.cs.y, p.delta, p.cs.x);
  const float st = __builtin_fmaf(p.cs.x, p.delta, p.cs.y);
  d_cos = __builtin_fmaf(rs, ct, shift);
  d_sin = __builtin_fmaf(rs, st, shift);
}

// Copies the mode's read-only tables from global memory (L2-resident) into LDS.
template <int kMode>
__device__ __forceinline__ void stage_tables(const KernelArgs &k, float *lds, uint32_t block = kBlock) {
  if constexpr (is_table(kMode)) {
    for (uint32_t i = threadIdx.x; i < k.table_len; i += block) lds[i] = k.table_a[i];
  } else {
    const float4 *src = reinterpret_cast<const float4 *>(k.bm_tables);
    float4 *dst = reinterpret_cast<float4 *>(lds);
    for (uint32_t i = threadIdx.x; i < bm_floats(kMode) / 4; i += block) {
      float4 v = src[i];
      uint32_t at = i;
      if (kMode == SMMC_MODE_GAUSSIAN) {
        if (i < kBm3RadiusEntries) {
          // counter stream v3: each radius coefficient times std, rounded once -- the cubic then yields
          // r std and the draw needs no multiply of its own; side 1 goes to its own place (kBm3Side1Bytes)
          v.x *= k.gauss_std;
          v.y *= k.gauss_std;
          v.z *= k.gauss_std;
          v.w *= k.gauss_std;
          if (i >= kBm3RadiusEntries / 2) at = kBm3Side1Bytes / 16u + (i - kBm3RadiusEntries / 2);
        } else {
          at = kBm3TrigBytes / 16u + (i - kBm3RadiusEntries);  // two (cos, sin) pairs per float4
        }
      }
      dst[at] = v;
    }
  }
}

// Draws per Philox block: 8 for table mode with T <= 2048 ("dense"), else 4.
template <int kMode, bool kDense>
struct Draws {
  static constexpr int value = (is_table(kMode) && kDense) ? 8 : 4;
};

// Four base-T digits of the 64-bit fraction (h:l): digit k = floor(T * frac(T^k x)) by
// exact 64 x 32-bit multiplies (two v_mad_u64_u32 each) for k = 0..2, the last one from
// the top 32 bits of what is left.  Relative bias < T^4/2^64 + T/2^32 (< 1.3e-6, T <= 2048).
__device__ __forceinline__ void digits4(uint32_t h, uint32_t l, uint32_t T, uint32_t (&idx)[4]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const uint64_t pl = static_cast<uint64_t>(l) * T;
    const uint64_t ph = static_cast<uint64_t>(h) * T + (pl >> 32);
    idx[d] = static_cast<uint32_t>(ph >> 32);
    h = static_cast<uint32_t>(ph);
    l = static_cast<uint32_t>(pl);
  }
  idx[3] = __umulhi(h, T);
}

// The per-period multipliers a = 100.0f + r that the four Philox words u of one block give: everything a draw does
// after Philox.  draw_words_kernel (the device self-test of the draws) feeds it chosen words.
template <int kMode, bool kDense>
__device__ __forceinline__ void multipliers_of_words(const KernelArgs &k, const DrawRegs &dr, const float *lds_table,
                                                     const uint32_t (&u)[4], float (&a)[Draws<kMode, kDense>::value]) {
  if constexpr (is_table(kMode) && kDense) {
    uint32_t ia[4], ib[4];
    digits4(u[0], u[1], k.table_len, ia);
    digits4(u[2], u[3], k.table_len, ib);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = lds_table[ia[j]];
      a[4 + j] = lds_table[ib[j]];
    }
  } else if constexpr (is_table(kMode)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = lds_table[__umulhi(u[j], k.table_len)];
  } else if constexpr (kMode == kModeGaussianV2) {
    float ret[4];  // the period returns in percent: N(gauss_mean, gauss_std)
    box_muller_scaled(lds_table, u[0], u[1], k.gauss_std, k.gauss_mean, ret[0], ret[1]);
    box_muller_scaled(lds_table, u[2], u[3], k.gauss_std, k.gauss_mean, ret[2], ret[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = 100.0f + ret[j];
  } else {  // counter stream v3: the multipliers themselves, N(100 + gauss_mean, gauss_std)
    const Bm3Pending p0 = bm3_issue(lds_table, u[0], u[1]);
    const Bm3Pending p1 = bm3_issue(lds_table, u[2], u[3]);
    bm3_finish(p0, dr.shift100, a[0], a[1]);
    bm3_finish(p1, dr.shift100, a[2], a[3]);
  }
}

// The per-period multipliers a = 100.0f + r of Philox block `blk` of a path.
template <int kMode, bool kDense, PhiloxForm kForm = kPhiloxGeneric>
__device__ __forceinline__ void block_multipliers(const KernelArgs &k, const DrawRegs &dr, const float *lds_table,
                                                  uint32_t path_lo, uint32_t path_hi, uint32_t blk,
                                                  float (&a)[Draws<kMode, kDense>::value]) {
  static_assert(kForm != kPhiloxUniformHi || counter_v3(kMode), "stream v2 counts blocks in the third word");
  uint32_t u[4];
  if constexpr (counter_v3(kMode))
    philox4x32_10<kForm>(blk, path_lo, path_hi, mode_tag(kMode), k.key0, k.key1, dr, u);
  else
    philox4x32_10<kPhiloxGeneric>(path_lo, path_hi, blk, mode_tag(kMode), k.key0, k.key1, dr, u);
  multipliers_of_words<kMode, kDense>(k, dr, lds_table, u, a);
}

// multipliers_of_words for the words of N blocks, drawn TOGETHER: all table gathers issued before the first is
// used.  The values are those of N calls of multipliers_of_words.
template <int kMode, bool kDense, int N>
__device__ __forceinline__ void multipliers_of_words_multi(const KernelArgs &k, const DrawRegs &dr, const float *lds_table,
                                                           const uint32_t (&u)[N][4],
                                                           float (&a)[N][Draws<kMode, kDense>::value]) {
  if constexpr (is_table(kMode) && kDense) {
    uint32_t idx[N][8];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      uint32_t ia[4], ib[4];
      digits4(u[i][0], u[i][1], k.table_len, ia);
      digits4(u[i][2], u[i][3], k.table_len, ib);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        idx[i][j] = ia[j];
        idx[i][4 + j] = ib[j];
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) a[i][j] = lds_table[idx[i][j]];
  } else if constexpr (is_table(kMode)) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[i][j] = lds_table[__umulhi(u[i][j], k.table_len)];
  } else if constexpr (kMode == kModeGaussianV2) {
    BmPending p[N][2];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      p[i][0] = bm_issue(lds_table, u[i][0], u[i][1]);
      p[i][1] = bm_issue(lds_table, u[i][2], u[i][3]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float ret[4];
      bm_finish(p[i][0], k.gauss_std, k.gauss_mean, ret[0], ret[1]);
      bm_finish(p[i][1], k.gauss_std, k.gauss_mean, ret[2], ret[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[i][j] = 100.0f + ret[j];
    }
  } else {
    Bm3Pending p[N][2];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      p[i][0] = bm3_issue(lds_table, u[i][0], u[i][1]);
      p[i][1] = bm3_issue(lds_table, u[i][2], u[i][3]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      bm3_finish(p[i][0], dr.shift100, a[i][0], a[i][1]);
      bm3_finish(p[i][1], dr.shift100, a[i][2], a[i][3]);
    }
  }
}

// The multipliers of the N consecutive Philox blocks blk .. blk + N - 1 of a path, drawn TOGETHER:
// interleaved Philox rounds, then multipliers_of_words_multi.  The values are those of N calls of block_multipliers.
template <int kMode, bool kDense, int N, bool kUniformBlock = false>
__device__ __forceinline__ void block_multipliers_multi(const KernelArgs &k, const DrawRegs &dr, const float *lds_table, uint32_t path_lo,
                                                        uint32_t path_hi, uint32_t blk,
                                                        float (&a)[N][Draws<kMode, kDense>::value]) {
  uint32_t u[N][4];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    u[i][0] = counter_v3(kMode) ? blk + i : path_lo;
    u[i][1] = counter_v3(kMode) ? path_lo : path_hi;
    u[i][2] = counter_v3(kMode) ? path_hi : blk + i;
    u[i][3] = mode_tag(kMode);
  }
  philox4x32_10_multi<N, kUniformBlock && counter_v3(kMode)>(u, k.key0, k.key1, dr);
  multipliers_of_words_multi<kMode, kDense, N>(k, dr, lds_table, u, a);
}

// kForm == kPhiloxUniformHi: the caller joins `path` from a per-lane low word and a SCALAR high word (philox4x32_10).
template <int kMode, int kDiv, bool kDense, PhiloxForm kForm = kPhiloxUniformBlock>
__device__ __forceinline__ float simulate_path(const KernelArgs &k, const DrawRegs &dr, const float *lds_table,
                                               uint64_t path) {
  constexpr int kDraws = Draws<kMode, kDense>::value;
  constexpr bool kExactDiv = kDiv == kDivExact;
  const uint32_t path_lo = static_cast<uint32_t>(path);
  const uint32_t path_hi = static_cast<uint32_t>(path >> 32);
  float total = k.initial_capital;
  bool left_window = false;
  const uint32_t full = k.n_periods / kDraws;
  // One Philox block per trip.  (Two blocks per trip with interleaved rounds -- block_multipliers_multi,
  // what the comb keepdata kernel uses at under 4 waves per SIMD -- ran 6 % SLOWER here: at 6 waves per
  // SIMD the VALU is already saturated once its multi-cycle multiplies are counted, 78 % of the plain
  // issue rate at the clock the chip holds under this load; so did issuing the next block's gathers in
  // front of this block's chain.)
  for (uint32_t blk = 0; blk < full; ++blk) {
    float a[kDraws];
    block_multipliers<kMode, kDense, kForm>(k, dr, lds_table, path_lo, path_hi, blk, a);
#pragma unroll
    for (int j = 0; j < kDraws; ++j) total = compound<kExactDiv>(total, a[j]);
    if constexpr (kDiv == kDivChecked) left_window |= !(total > k.chk_lo && total < k.chk_hi);  // NaN leaves too
  }
  const uint32_t rem = k.n_periods - full * kDraws;
  if (rem) {  // wave-uniform
    float a[kDraws];
    block_multipliers<kMode, kDense, kForm>(k, dr, lds_table, path_lo, path_hi, full, a);
#pragma unroll
    for (int j = 0; j < kDraws - 1; ++j)
      if (static_cast<uint32_t>(j) < rem) total = compound<kExactDiv>(total, a[j]);
  }
  if constexpr (kDiv == kDivChecked) {
    if (left_window) total = simulate_path<kMode, kDivExact, kDense, kForm>(k, dr, lds_table, path);
  }
  return total;
}

// ---- the workgroups' partial statistics ----------------------------------------------------------
//
// paths_kernel leaves one partial per workgroup; finalize_kernel (one 1024-thread workgroup, a launch later) folds them
// in a fixed order.  Round 4 tried to fold them INSIDE the launch (the workgroup that finishes last
// writes the header) in three forms, all bit-identical to the separate launch and all measured on the 1e6-path step
// (profiles/r04/config0_variants*.txt; the separate launch: 169.5 us per step, kernel 159 us): a release fence per
// workgroup + one arrival counter 178-265 us (the fence waits for every final value queued in the XCD's L2; same-address
// atomics take ~12 ns each); device-scope atomic exchanges instead of the fence + 64 + 1 counters, the last workgroup
// folding all 3907 partials 180.6 us (15 dependent rounds of device-scope loads per thread); a two-level fold -- the
// workgroup that completes a group of 64 folds it, the one that completes the groups folds those -- 172.5 us.  The
// floor is the chain itself: publish, count, load, publish, count, load are six device-scope round trips of ~1.7 us
// across the eight XCDs, as long as the launch boundary they replace.  The separate launch stays.
__device__ __forceinline__ void partial_identity(BlockPartial &t) {
  t.sum = 0.0;
  t.sumsq = 0.0;
  t.count = t.below = t.underflow = t.overflow = 0ull;
  t.min = __builtin_inff();
  t.max = -__builtin_inff();
}
__device__ __forceinline__ void partial_add(BlockPartial &a, const BlockPartial &b) {
  a.sum += b.sum;
  a.sumsq += b.sumsq;
  a.count += b.count;
  a.below += b.below;
  a.underflow += b.underflow;
  a.overflow += b.overflow;
  a.min = fminf(a.min, b.min);
  a.max = fmaxf(a.max, b.max);
}

// The two wave sums of a chunk's statistics, without LDS traffic: s1 summed over the wave arrives in lane 0, s2 in
// lane 32 (other lanes: partial sums nobody reads), each added in the association of dev::wave_sum,
//   for (off = 32; off > 0; off >>= 1) v += shfl_down(v, off),
// as lane 0 sees it -- ((x0 + x32) + (x16 + x48)) + ... -- because the sum of squares is not exact in binary64 and
// the chunk variance is a bit-exact contract.  v_permlane32_swap puts the low halves of BOTH operands into one
// register and the high halves into the other, so ONE add does the offset-32 step of both sums (s1 in lanes
// [0, 32), s2 in [32, 64)); v_permlane16_swap pairs rows 0 + 1 and 2 + 3; the offsets 8 .. 1 stay inside a row of
// 16 lanes, which DPP row shifts read (lanes shifted in from outside the row read 0 and only reach lanes that lane 0
// and lane 32 never take from).  20 VALU instructions for both sums; wave_sum's ds_bpermute form took 24 LDS
// instructions and about 20 of lane arithmetic beside the 12 adds.  Every lane of the wave must be enabled.
__device__ __forceinline__ uint32_t lo32(double v) { return static_cast<uint32_t>(__double_as_longlong(v)); }
__device__ __forceinline__ uint32_t hi32(double v) { return static_cast<uint32_t>(__double_as_longlong(v) >> 32); }
__device__ __forceinline__ double join64(uint32_t lo, uint32_t hi) {
  return __longlong_as_double(static_cast<long long>(static_cast<uint64_t>(hi) << 32 | lo));
}
template <int kShift>
__device__ __forceinline__ double row_shl_add(double v) {  // v[i] += v[i + kShift] inside each row of 16 lanes
  constexpr int kRowShl = 0x100 + kShift;                   // DPP control row_shl:kShift
  const uint32_t lo = __builtin_amdgcn_update_dpp(0u, lo32(v), kRowShl, 0xf, 0xf, true);
  const uint32_t hi = __builtin_amdgcn_update_dpp(0u, hi32(v), kRowShl, 0xf, 0xf, true);
  return v + join64(lo, hi);
}
__device__ __forceinline__ double wave_sum_pair(double s1, double s2) {
  const auto l = __builtin_amdgcn_permlane32_swap(lo32(s1), lo32(s2), false, false);  // [0]: low halves of s1, s2
  const auto h = __builtin_amdgcn_permlane32_swap(hi32(s1), hi32(s2), false, false);  // [1]: their high halves
  double v = join64(l[0], h[0]) + join64(l[1], h[1]);                                 // x[i] + x[i + 32]
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo32(v), lo32(v), false, false);  // [0]: rows 0 0 2 2, [1]: 1 1 3 3
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi32(v), hi32(v), false, false);
  v = join64(l16[0], h16[0]) + join64(l16[1], h16[1]);                                // ... + v[i + 16]
  v = row_shl_add<8>(v);
  v = row_shl_add<4>(v);
  v = row_shl_add<2>(v);
  return row_shl_add<1>(v);
}

// ---- main kernel ---------------------------------------------------------------

// Persistent workgroups; each iteration one chunk of 256 consecutive paths (one
// per lane) so the final-value store of a wave is one 256-byte line-aligned
// segment.  LDS: [table (100 + r)] [histogram u32 bins].
//
// Counter stream v3's Gaussian mode runs TWO such blocks per workgroup (paths_halves): threads [0, 256) and
// [256, 512) are "virtual blocks" vb = 2 blockIdx.x and 2 blockIdx.x + 1 of a grid of `vgrid`, and the eight waves
// read ONE staged copy of the draw tables -- four 36 KiB workgroups per CU are then eight waves per SIMD instead of
// four.  A half walks the chunks vb, vb + vgrid, ... with its own accumulators, reduction scratch and partial,
// exactly as a 256-thread workgroup of a vgrid-wide launch does: every output holds the same values added in the
// same order.  The halves share the LDS histogram (integer atomics) and the barriers, so the chunk loop runs the
// trip count of half 0 -- never the smaller one, its vb is the lower -- and a half whose chunk does not exist
// (vb == vgrid when vgrid is odd, or one trip short) goes through the trip with every lane inactive.
constexpr uint32_t paths_halves(int mode) { return mode == SMMC_MODE_GAUSSIAN ? 2u : 1u; }
// ... which needs the kernel inside 64 VGPRs: asked of the compiler for that mode only (1 = no constraint)
constexpr uint32_t paths_min_waves(int mode) { return paths_halves(mode) > 1 ? 8u : 1u; }
template <int kMode, int kDiv, bool kDense>
__global__ __launch_bounds__(kBlock * paths_halves(kMode)) __attribute__((amdgpu_waves_per_eu(paths_min_waves(kMode))))
void paths_kernel(const KernelArgs k, const uint32_t vgrid) {
  constexpr uint32_t kHalves = paths_halves(kMode);
  constexpr uint32_t kGroup = kBlock * kHalves;  // threads per workgroup
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *lds_table = reinterpret_cast<float *>(lds_raw);  // returns table, or the Box-Muller tables
  const uint32_t table_words = is_table(kMode) ? k.table_len : bm_lds_words(kMode);
  uint32_t *lds_hist = reinterpret_cast<uint32_t *>(lds_raw) + table_words;
  // The reduction scratch lives BEHIND the tables in the dynamic allocation (paths_lds_bytes), not in
  // static __shared__ arrays: static LDS is placed first, and a draw table that does not start at LDS
  // address 0 costs one address add per gather (two VALU instructions per Philox block in Gaussian mode).
  const uint32_t scratch_words = (table_words + ((k.partials != nullptr) ? k.n_bins : 0u) + 1u) & ~1u;  // 8-byte aligned
  double *red_scratch = reinterpret_cast<double *>(reinterpret_cast<uint32_t *>(lds_raw) + scratch_words);  // [kHalves][4 * kWaves]
  BlockPartial *wave_part = reinterpret_cast<BlockPartial *>(red_scratch + 4 * kWaves * kHalves);          // [kHalves][kWaves]

  const uint32_t half = kHalves > 1 ? threadIdx.x / kBlock : 0u;  // wave-uniform
  const uint32_t tid = kHalves > 1 ? threadIdx.x % kBlock : threadIdx.x;
  const uint32_t vb = blockIdx.x * kHalves + half;  // the virtual block: <= vgrid, == vgrid only for the idle half of an odd grid
  red_scratch += half * (4 * kWaves);
  wave_part += half * kWaves;
  bool parity = false;
  unsigned long long clk0 = 0, real0 = 0;
  if (k.clock_probe) {  // uniform; timing instrumentation only
    clk0 = __builtin_amdgcn_s_memtime();
    real0 = __builtin_amdgcn_s_memrealtime();
  }
  stage_tables<kMode>(k, lds_table, kGroup);
  const bool want_stats = k.partials != nullptr;
  const bool want_hist = want_stats && k.n_bins != 0;
  if (want_hist) {
    for (uint32_t i = threadIdx.x; i < k.n_bins; i += kGroup) lds_hist[i] = 0u;
  }
  __syncthreads();

  double sum = 0.0, sumsq = 0.0;
  uint32_t n_count = 0, n_below = 0, n_under = 0, n_over = 0;
  float vmin = __builtin_inff(), vmax = -__builtin_inff();
  const DrawRegs dr = make_draw_regs(k);

  const uint64_t n_chunks = (k.n_paths + kBlock - 1) / kBlock;
  // chunk0 is the chunk of half 0 and workgroup-uniform: every wave of the workgroup makes the same trips and
  // meets the same barriers; `live` says whether this half has a chunk in this trip
  for (uint64_t chunk0 = static_cast<uint64_t>(blockIdx.x) * kHalves; chunk0 < n_chunks; chunk0 += vgrid) {
    const uint64_t chunk = chunk0 + half;
    const bool live = kHalves == 1 || (vb < vgrid && chunk < n_chunks);  // wave-uniform
    const uint64_t i = chunk * kBlock + tid;
    const bool active = live && i < k.n_paths;
    float v = 0.0f;
    if (active) {
      v = simulate_path<kMode, kDiv, kDense>(k, dr, lds_table, k.first_path + i);
      if (k.d_final) k.d_final[i] = v;
    }
    if (want_stats && active) {
      const double dv = static_cast<double>(v);
      sum += dv;
      sumsq += dv * dv;
      n_count += 1;
      n_below += (v < k.below_threshold) ? 1u : 0u;
      vmin = fminf(vmin, v);
      vmax = fmaxf(vmax, v);
      if (want_hist) {
        if (v < k.hist_lo) {
          n_under += 1;
        } else if (v < k.hist_hi) {
          int32_t b = static_cast<int32_t>((dv - static_cast<double>(k.hist_lo)) * k.hist_inv);
          b = b < static_cast<int32_t>(k.n_bins) - 1 ? b : static_cast<int32_t>(k.n_bins) - 1;
          atomicAdd(&lds_hist[b], 1u);
        } else {
          n_over += 1;
        }
      }
    }
    if (k.d_chunk_mean || k.d_chunk_var) {  // uniform over the workgroup
      // mean and population variance of this chunk from one pass (sum and sum of squares in
      // double: the cancellation in E[x^2] - mean^2 costs ~1e-15 relative here), one barrier:
      // the scratch slots alternate with the iteration's parity
      const double dv = active ? static_cast<double>(v) : 0.0;
      const double s12 = wave_sum_pair(dv, dv * dv);  // lane 0: the wave's sum, lane 32: its sum of squares
      double *slot = red_scratch + (parity ? 2 * kWaves : 0);
      parity = !parity;
      const int lane = tid & 63, wave = tid >> 6;
      if ((lane & 31) == 0) slot[(lane ? kWaves : 0) + wave] = s12;
      __syncthreads();
      if (tid == 0 && live) {
        double t1 = slot[0], t2 = slot[kWaves];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
          t1 += slot[w];
          t2 += slot[kWaves + w];
        }
        // A full chunk -- every chunk but the last one of a launch -- needs no divide: t * 2^-8 and t / 256 are the
        // same binary64 for every sum of binary32 values or of their squares (no subnormal double arises; inf and
        // NaN go through alike).  The IEEE divides stay for the one chunk that may be ragged.
        double mean, var;
        if (chunk + 1 < n_chunks) {
          static_assert(kBlock == 256, "the full chunk's reciprocal is 2^-8");
          mean = t1 * 0x1p-8;
          var = t2 * 0x1p-8 - mean * mean;
        } else {
          const double n_in = static_cast<double>(k.n_paths - chunk * kBlock);  // 1 .. kBlock
          mean = t1 / n_in;
          var = t2 / n_in - mean * mean;
        }
        if (k.d_chunk_mean) k.d_chunk_mean[chunk] = static_cast<float>(mean);
        if (k.d_chunk_var) k.d_chunk_var[chunk] = static_cast<float>(var > 0.0 ? var : 0.0);
      }
    }
  }

  if (k.clock_probe && threadIdx.x == 0) {
    atomicAdd(&k.clock_probe[0], __builtin_amdgcn_s_memtime() - clk0);
    atomicAdd(&k.clock_probe[1], __builtin_amdgcn_s_memrealtime() - real0);
  }
  if (want_stats) {
    // per-lane u32 counters cannot overflow: a lane sees < 2^32 chunks
    BlockPartial p;
    p.sum = wave_sum(sum);
    p.sumsq = wave_sum(sumsq);
    p.count = wave_sum(static_cast<unsigned long long>(n_count));
    p.below = wave_sum(static_cast<unsigned long long>(n_below));
    p.underflow = wave_sum(static_cast<unsigned long long>(n_under));
    p.overflow = wave_sum(static_cast<unsigned long long>(n_over));
    p.min = wave_min(vmin);
    p.max = wave_max(vmax);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_part[wave] = p;
    __syncthreads();
    if (tid == 0 && vb < vgrid) {  // one partial per virtual block; the idle half of an odd grid has none
      BlockPartial t = wave_part[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        t.sum += wave_part[w].sum;
        t.sumsq += wave_part[w].sumsq;
        t.count += wave_part[w].count;
        t.below += wave_part[w].below;
        t.underflow += wave_part[w].underflow;
        t.overflow += wave_part[w].overflow;
        t.min = fminf(t.min, wave_part[w].min);
        t.max = fmaxf(t.max, wave_part[w].max);
      }
      k.partials[vb] = t;
    }
    if (want_hist) {  // LDS atomics of all waves are complete after the barrier above
      for (uint32_t b = threadIdx.x; b < k.n_bins; b += kGroup) {
        const uint32_t c = lds_hist[b];
        if (c) atomicAdd(&k.d_hist[b], static_cast<unsigned long long>(c));
      }
    }
  }
}

// paths_kernel for a launch whose paths all have the same id bits 63..32 (launch_paths decides: paths_form in
// smmc_internal.h): the high word is a kernel argument in a scalar register, not the carry of a per-lane 64-bit add,
// and the period loop runs philox4x32_10<kPhiloxUniformHi> -- 68 VALU instructions per Philox block instead of 70 in
// Gaussian mode, 82 instead of 84 in dense table mode, one of the two a half-rate multiply.  The draws, and with
// them every output, are paths_kernel's bit for bit (tests/test_uniform_hi_gpu.py).
//
// The chunk walk, the outputs, the epilogue, the LDS layout, the halves and the occupancy request are paths_kernel's
// statements, here a second time for the reason given above blocks_body: paths_kernel has to stay the instruction
// sequence its counters were taken on, and every way of sharing code with it that was built moved that sequence.
// A change to one copy belongs in the other.
template <int kMode, int kDiv, bool kDense>
__global__ __launch_bounds__(kBlock * paths_halves(kMode)) __attribute__((amdgpu_waves_per_eu(paths_min_waves(kMode))))
void paths_hi_kernel(const KernelArgs k, const uint32_t vgrid) {
  static_assert(counter_v3(kMode), "stream v2 has no uniform-high-word form");
  constexpr uint32_t kHalves = paths_halves(kMode);
  constexpr uint32_t kGroup = kBlock * kHalves;  // threads per workgroup
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *lds_table = reinterpret_cast<float *>(lds_raw);  // returns table, or the Box-Muller tables
  const uint32_t table_words = is_table(kMode) ? k.table_len : bm_lds_words(kMode);
  uint32_t *lds_hist = reinterpret_cast<uint32_t *>(lds_raw) + table_words;
  const uint32_t scratch_words = (table_words + ((k.partials != nullptr) ? k.n_bins : 0u) + 1u) & ~1u;  // 8-byte aligned
  double *red_scratch = reinterpret_cast<double *>(reinterpret_cast<uint32_t *>(lds_raw) + scratch_words);  // [kHalves][4 * kWaves]
  BlockPartial *wave_part = reinterpret_cast<BlockPartial *>(red_scratch + 4 * kWaves * kHalves);          // [kHalves][kWaves]

  const uint32_t half = kHalves > 1 ? threadIdx.x / kBlock : 0u;  // wave-uniform
  const uint32_t tid = kHalves > 1 ? threadIdx.x % kBlock : threadIdx.x;
  const uint32_t vb = blockIdx.x * kHalves + half;  // the virtual block: <= vgrid, == vgrid only for the idle half of an odd grid
  red_scratch += half * (4 * kWaves);
  wave_part += half * kWaves;
  bool parity = false;
  unsigned long long clk0 = 0, real0 = 0;
  if (k.clock_probe) {  // uniform; timing instrumentation only
    clk0 = __builtin_amdgcn_s_memtime();
    real0 = __builtin_amdgcn_s_memrealtime();
  }
  stage_tables<kMode>(k, lds_table, kGroup);
  const bool want_stats = k.partials != nullptr;
  const bool want_hist = want_stats && k.n_bins != 0;
  if (want_hist) {
    for (uint32_t i = threadIdx.x; i < k.n_bins; i += kGroup) lds_hist[i] = 0u;
  }
  __syncthreads();

  double sum = 0.0, sumsq = 0.0;
  uint32_t n_count = 0, n_below = 0, n_under = 0, n_over = 0;
  float vmin = __builtin_inff(), vmax = -__builtin_inff();
  const DrawRegs dr = make_draw_regs(k);
  // the launch's share of every path id: the low word wraps with the lane's index, the high word never moves
  const uint32_t first_lo = static_cast<uint32_t>(k.first_path);
  const uint64_t first_hi = k.first_path & 0xFFFFFFFF00000000ull;  // scalar

  const uint64_t n_chunks = (k.n_paths + kBlock - 1) / kBlock;
  for (uint64_t chunk0 = static_cast<uint64_t>(blockIdx.x) * kHalves; chunk0 < n_chunks; chunk0 += vgrid) {
    const uint64_t chunk = chunk0 + half;
    const bool live = kHalves == 1 || (vb < vgrid && chunk < n_chunks);  // wave-uniform
    const uint64_t i = chunk * kBlock + tid;
    const bool active = live && i < k.n_paths;
    float v = 0.0f;
    if (active) {
      const uint32_t path_lo = first_lo + static_cast<uint32_t>(i);
      v = simulate_path<kMode, kDiv, kDense, kPhiloxUniformHi>(k, dr, lds_table, first_hi | path_lo);
      if (k.d_final) k.d_final[i] = v;
    }
    if (want_stats && active) {
      const double dv = static_cast<double>(v);
      sum += dv;
      sumsq += dv * dv;
      n_count += 1;
      n_below += (v < k.below_threshold) ? 1u : 0u;
      vmin = fminf(vmin, v);
      vmax = fmaxf(vmax, v);
      if (want_hist) {
        if (v < k.hist_lo) {
          n_under += 1;
        } else if (v < k.hist_hi) {
          int32_t b = static_cast<int32_t>((dv - static_cast<double>(k.hist_lo)) * k.hist_inv);
          b = b < static_cast<int32_t>(k.n_bins) - 1 ? b : static_cast<int32_t>(k.n_bins) - 1;
          atomicAdd(&lds_hist[b], 1u);
        } else {
          n_over += 1;
        }
      }
    }
    if (k.d_chunk_mean || k.d_chunk_var) {  // uniform over the workgroup
      const double dv = active ? static_cast<double>(v) : 0.0;
      const double s12 = wave_sum_pair(dv, dv * dv);  // lane 0: the wave's sum, lane 32: its sum of squares
      double *slot = red_scratch + (parity ? 2 * kWaves : 0);
      parity = !parity;
      const int lane = tid & 63, wave = tid >> 6;
      if ((lane & 31) == 0) slot[(lane ? kWaves : 0) + wave] = s12;
      __syncthreads();
      if (tid == 0 && live) {
        double t1 = slot[0], t2 = slot[kWaves];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
          t1 += slot[w];
          t2 += slot[kWaves + w];
        }
        double mean, var;  // a full chunk needs no divide: see paths_kernel
        if (chunk + 1 < n_chunks) {
          static_assert(kBlock == 256, "the full chunk's reciprocal is 2^-8");
          mean = t1 * 0x1p-8;
          var = t2 * 0x1p-8 - mean * mean;
        } else {
          const double n_in = static_cast<double>(k.n_paths - chunk * kBlock);  // 1 .. kBlock
          mean = t1 / n_in;
          var = t2 / n_in - mean * mean;
        }
        if (k.d_chunk_mean) k.d_chunk_mean[chunk] = static_cast<float>(mean);
        if (k.d_chunk_var) k.d_chunk_var[chunk] = static_cast<float>(var > 0.0 ? var : 0.0);
      }
    }
  }

  if (k.clock_probe && threadIdx.x == 0) {
    atomicAdd(&k.clock_probe[0], __builtin_amdgcn_s_memtime() - clk0);
    atomicAdd(&k.clock_probe[1], __builtin_amdgcn_s_memrealtime() - real0);
  }
  if (want_stats) {
    // per-lane u32 counters cannot overflow: a lane sees < 2^32 chunks
    BlockPartial p;
    p.sum = wave_sum(sum);
    p.sumsq = wave_sum(sumsq);
    p.count = wave_sum(static_cast<unsigned long long>(n_count));
    p.below = wave_sum(static_cast<unsigned long long>(n_below));
    p.underflow = wave_sum(static_cast<unsigned long long>(n_under));
    p.overflow = wave_sum(static_cast<unsigned long long>(n_over));
    p.min = wave_min(vmin);
    p.max = wave_max(vmax);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_part[wave] = p;
    __syncthreads();
    if (tid == 0 && vb < vgrid) {  // one partial per virtual block; the idle half of an odd grid has none
      BlockPartial t = wave_part[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        t.sum += wave_part[w].sum;
        t.sumsq += wave_part[w].sumsq;
        t.count += wave_part[w].count;
        t.below += wave_part[w].below;
        t.underflow += wave_part[w].underflow;
        t.overflow += wave_part[w].overflow;
        t.min = fminf(t.min, wave_part[w].min);
        t.max = fmaxf(t.max, wave_part[w].max);
      }
      k.partials[vb] = t;
    }
    if (want_hist) {  // LDS atomics of all waves are complete after the barrier above
      for (uint32_t b = threadIdx.x; b < k.n_bins; b += kGroup) {
        const uint32_t c = lds_hist[b];
        if (c) atomicAdd(&k.d_hist[b], static_cast<unsigned long long>(c));
      }
    }
  }
}

// Reduces the per-workgroup partials in a fixed order and writes the record header.
// One 1024-thread workgroup: 16 k partials (64 workgroups per CU) take ~8 us instead of 26.
constexpr int kFinalizeBlock = 1024;
__global__ __launch_bounds__(kFinalizeBlock) void finalize_kernel(const BlockPartial *partials,
                                                                  uint32_t n_partials, smmc_stats *out,
                                                                  uint32_t n_bins, unsigned long long *hist_acc,
                                                                  uint32_t spread) {
  // The bucket counts were accumulated in the engine's own array (one copy by paths_kernel, kHistSpread copies by
  // values_stats): fold them into the record's and LEAVE THE ARRAY ZERO for the next launch -- the record needs no
  // memset before a launch and the accumulator none after it (two launches per step instead of three).
  if (spread) {
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(out + 1);
    for (uint32_t b = threadIdx.x; b < n_bins; b += kFinalizeBlock) {
      unsigned long long c = 0;
      for (uint32_t r = 0; r < spread; ++r) {
        unsigned long long *src = hist_acc + static_cast<size_t>(r) * n_bins + b;
        const unsigned long long v = *src;
        c += v;
        if (v) *src = 0;
      }
      hist[b] = c;
    }
  }
  __shared__ BlockPartial sh[kFinalizeBlock];
  BlockPartial t;
  partial_identity(t);
  for (uint32_t j = threadIdx.x; j < n_partials; j += kFinalizeBlock) partial_add(t, partials[j]);
  sh[threadIdx.x] = t;
  __syncthreads();
  for (uint32_t s = kFinalizeBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) partial_add(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const BlockPartial &r = sh[0];
    out->count = r.count;
    out->below = r.below;
    out->underflow = r.underflow;
    out->overflow = r.overflow;
    out->sum = r.sum;
    out->sumsq = r.sumsq;
    out->min = r.min;
    out->max = r.max;
    out->n_bins = n_bins;
    out->reserved = 0;
  }
}

// ---- block bootstrap: table paths drawn in runs of consecutive months ------------------------------
//
// smmc_engine_simulate_blocks (csrc/smmc_blocks.cpp; DESIGN.md, "Block bootstrap").  Block b of a path starts at the
// table index the i.i.d. table stream draws for that path at period b -- Philox block b / D, digit b % D, the key,
// counter layout and mode tag of SMMC_MODE_TABLE -- and period t reads entry (s_{t div L} + t mod L) mod T.  All
// lanes of a wave share t, L and the block boundaries: the control flow is wave-uniform, only addresses differ.
//
// The period loop walks a block in segments of kBlockSeg = 8 consecutive periods.  The table is staged with its
// beginning repeated behind its end, so that a segment reads `base + j` with j in the instruction's offset field: no
// address arithmetic and no wrap test per period; between segments the base advances by 8 mod T and wraps once, and
// the checked window is tested (a segment is at most 8 periods: the window smmc_capi.cpp derives for "at most 8
// periods until the next test" holds).  Two layouts (BlockLayout):
//   narrow  one copy, lds[i] = a[i mod T] for i < T + 7; a segment is eight 4-byte reads (the compiler pairs them
//           into ds_read2_b32), each half-wave hitting 32 random banks;
//   wide    four copies, copy c holding a[(i + c) mod T] at slot i < round4(T) + 8: a lane whose base is s reads
//           copy s & 3 at slot s & ~3, which is 16-byte aligned, so a segment is two ds_read_b128 (64 banks, 16
//           lanes per LDS cycle).  18 KiB at T = 1127; the host picks it while eight workgroups per CU still fit.
constexpr int kBlockSeg = 8;
constexpr uint32_t kBlockCopies = 4;
struct BlockLayout {  // wave-uniform
  uint32_t block_len;   // L
  uint32_t copy_words;  // words per staged copy
  uint32_t step;        // kBlockSeg mod T: what a base advances by between segments
};
constexpr uint32_t blocks_copy_words(uint32_t table_len, bool wide) {
  return wide ? ((table_len + 3u) & ~3u) + kBlockSeg : table_len + kBlockSeg - 1u;
}
constexpr uint32_t blocks_table_words(uint32_t table_len, bool wide) {
  return blocks_copy_words(table_len, wide) * (wide ? kBlockCopies : 1u);
}

template <bool kWide>
__device__ __forceinline__ void stage_block_table(const KernelArgs &k, const BlockLayout &g, float *lds, uint32_t threads) {
  const uint32_t T = k.table_len;
  for (uint32_t c = 0; c < (kWide ? kBlockCopies : 1u); ++c)
    for (uint32_t i = threadIdx.x; i < g.copy_words; i += threads) lds[c * g.copy_words + i] = k.table_a[(i + c) % T];
}

// The D block starts of Philox block `blk` of a path: exactly the table indices block_multipliers draws there, in its
// order ia[0..3], ib[0..3] (D = 8, T <= 2048) or the four __umulhi digits (D = 4).  The device-side draw of the block
// bootstrap, for whichever kernel walks blocks.
template <bool kDense>
__device__ __forceinline__ void block_starts(const KernelArgs &k, const DrawRegs &dr, uint32_t path_lo, uint32_t path_hi, uint32_t blk,
                                             uint32_t (&s)[Draws<SMMC_MODE_TABLE, kDense>::value]) {
  uint32_t u[4];
  philox4x32_10<kPhiloxUniformBlock>(blk, path_lo, path_hi, mode_tag(SMMC_MODE_TABLE), k.key0, k.key1, dr, u);
  if constexpr (kDense) {
    uint32_t ia[4], ib[4];
    digits4(u[0], u[1], k.table_len, ia);
    digits4(u[2], u[3], k.table_len, ib);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = ia[j];
      s[4 + j] = ib[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = __umulhi(u[j], k.table_len);
  }
}

// Where the segment that begins at table index s < T lies in LDS (word index).
template <bool kWide>
__device__ __forceinline__ uint32_t block_segment_at(const BlockLayout &g, uint32_t s) {
  if constexpr (kWide) return (s & 3u) * g.copy_words + (s & ~3u);
  return s;
}

// `len` >= 1 consecutive periods (wave-uniform) from table index s < T, wrapping at the end of the table.
template <bool kExactDiv, bool kChecked, bool kWide>
__device__ __forceinline__ void block_run(const KernelArgs &k, const BlockLayout &g, const float *lds, uint32_t s, uint32_t len,
                                          float &total, bool &left_window) {
  uint32_t rem = len;
  for (; rem >= kBlockSeg; rem -= kBlockSeg) {
    const float *at = lds + block_segment_at<kWide>(g, s);
    float a[kBlockSeg];
    if constexpr (kWide) {
      const f32x4_t q0 = *reinterpret_cast<const f32x4_t *>(at), q1 = *reinterpret_cast<const f32x4_t *>(at + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = q0[j];
        a[4 + j] = q1[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < kBlockSeg; ++j) a[j] = at[j];
    }
#pragma unroll
    for (int j = 0; j < kBlockSeg; ++j) total = compound<kExactDiv>(total, a[j]);
    if constexpr (kChecked) left_window |= !(total > k.chk_lo && total < k.chk_hi);  // NaN leaves too
    s += g.step;  // < 2 T
    s = s >= k.table_len ? s - k.table_len : s;
  }
  if (rem) {  // wave-uniform: the block's last 1 .. 7 periods
    const float *at = lds + block_segment_at<kWide>(g, s);
    if constexpr (kWide) {
      const f32x4_t q0 = *reinterpret_cast<const f32x4_t *>(at);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (static_cast<uint32_t>(j) < rem) total = compound<kExactDiv>(total, q0[j]);
      if (rem > 4) {
        const f32x4_t q1 = *reinterpret_cast<const f32x4_t *>(at + 4);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (static_cast<uint32_t>(4 + j) < rem) total = compound<kExactDiv>(total, q1[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kBlockSeg - 1; ++j)
        if (static_cast<uint32_t>(j) < rem) total = compound<kExactDiv>(total, at[j]);
    }
    if constexpr (kChecked) left_window |= !(total > k.chk_lo && total < k.chk_hi);
  }
}

template <int kDiv, bool kDense, bool kWide>
__device__ __forceinline__ float simulate_block_path(const KernelArgs &k, const BlockLayout &g, const DrawRegs &dr, const float *lds,
                                                     uint64_t path) {
  constexpr int kDraws = Draws<SMMC_MODE_TABLE, kDense>::value;
  constexpr bool kExactDiv = kDiv == kDivExact;
  const uint32_t path_lo = static_cast<uint32_t>(path);
  const uint32_t path_hi = static_cast<uint32_t>(path >> 32);
  float total = k.initial_capital;
  bool left_window = false;
  uint32_t t = 0;  // periods done; the block in hand covers [t, t + L)
  for (uint32_t blk = 0; t < k.n_periods; ++blk) {
    uint32_t s[kDraws];
    block_starts<kDense>(k, dr, path_lo, path_hi, blk, s);
#pragma unroll
    for (int d = 0; d < kDraws; ++d) {
      if (t < k.n_periods) {  // wave-uniform
        const uint32_t left = k.n_periods - t;
        const uint32_t len = left < g.block_len ? left : g.block_len;
        block_run<kExactDiv, kDiv == kDivChecked, kWide>(k, g, lds, s[d], len, total, left_window);
        t += len;
      }
    }
  }
  if constexpr (kDiv == kDivChecked) {
    if (left_window) total = simulate_block_path<kDivExact, kDense, kWide>(k, g, dr, lds, path);
  }
  return total;
}

// paths_kernel's chunk walk, outputs and epilogue for a 256-thread workgroup, as a function of what is staged in front
// of the histogram and of how a lane walks its path: `Walk` names both in static functions -- table_words(k, aux),
// stage(k, aux, lds_table, threads per workgroup), simulate(k, aux, dr, lds_table, path) -- and `aux` is a launch
// parameter of the walk's own (the block length; a structure for RegimesWalk).
//
// The statements are paths_kernel's (without its two-halves form), and they are here a second time because
// paths_kernel has to stay the instruction sequence its counters were taken on (profiles/pmc_traffic.json: 1047
// instructions in Gaussian mode, 1143 in table mode; tools/pmc_traffic.py --restamp compares the fingerprints).  Every
// way of calling shared code from paths_kernel that was built moved that sequence, although each computes the same
// values (same flags, same compiler; instructions Gaussian / table, "reordered" = same count, other order):
//   the whole body as this function, walk passed as lambdas or as a static-function struct     1043 / 1146
//   three pieces (per-path statistics + histogram, chunk mean/variance, partial fold + flush)   1046 / 1144
//   only the per-path statistics + histogram, accumulators in a struct                          reordered / reordered
//   only the per-path statistics + histogram, accumulators as reference arguments               unchanged / reordered
//   only the chunk mean / variance block                                                        1046 / 1144
//   only the partial fold + histogram flush (struct, or eight scalar arguments)                 reordered / reordered
//   only the accumulators gathered in a struct, no function at all                              reordered / reordered
//   only the histogram flush loop                                                               reordered / reordered
// A change to one copy belongs in the other; tests/test_blocks_gpu.py holds block length 1 to paths_kernel's bytes.
template <typename Walk, typename Aux = uint32_t>
__device__ __forceinline__ void blocks_body(const KernelArgs &k, const uint32_t vgrid, const Aux aux, unsigned char *lds_raw) {
  const uint32_t table_words = Walk::table_words(k, aux);
  constexpr uint32_t kGroup = kBlock;  // threads per workgroup
  float *lds_table = reinterpret_cast<float *>(lds_raw);  // returns table, or the Box-Muller tables
  uint32_t *lds_hist = reinterpret_cast<uint32_t *>(lds_raw) + table_words;
  // The reduction scratch lives BEHIND the tables in the dynamic allocation (paths_lds_bytes), not in
  // static __shared__ arrays: static LDS is placed first, and a draw table that does not start at LDS
  // address 0 costs one address add per gather (two VALU instructions per Philox block in Gaussian mode).
  const uint32_t scratch_words = (table_words + ((k.partials != nullptr) ? k.n_bins : 0u) + 1u) & ~1u;  // 8-byte aligned
  double *red_scratch = reinterpret_cast<double *>(reinterpret_cast<uint32_t *>(lds_raw) + scratch_words);  // [4 * kWaves]
  BlockPartial *wave_part = reinterpret_cast<BlockPartial *>(red_scratch + 4 * kWaves);  // [kWaves]

  const uint32_t tid = threadIdx.x;
  bool parity = false;
  unsigned long long clk0 = 0, real0 = 0;
  if (k.clock_probe) {  // uniform; timing instrumentation only
    clk0 = __builtin_amdgcn_s_memtime();
    real0 = __builtin_amdgcn_s_memrealtime();
  }
  Walk::stage(k, aux, lds_table, kGroup);
  const bool want_stats = k.partials != nullptr;
  const bool want_hist = want_stats && k.n_bins != 0;
  if (want_hist) {
    for (uint32_t i = threadIdx.x; i < k.n_bins; i += kGroup) lds_hist[i] = 0u;
  }
  __syncthreads();

  double sum = 0.0, sumsq = 0.0;
  uint32_t n_count = 0, n_below = 0, n_under = 0, n_over = 0;
  float vmin = __builtin_inff(), vmax = -__builtin_inff();
  const DrawRegs dr = make_draw_regs(k);

  const uint64_t n_chunks = (k.n_paths + kBlock - 1) / kBlock;
  // workgroup-uniform: every wave of the workgroup makes the same trips and meets the same barriers
  for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += vgrid) {
    const uint64_t i = chunk * kBlock + tid;
    const bool active = i < k.n_paths;
    float v = 0.0f;
    if (active) {
      v = Walk::simulate(k, aux, dr, lds_table, k.first_path + i);
      if (k.d_final) k.d_final[i] = v;
    }
    if (want_stats && active) {
      const double dv = static_cast<double>(v);
      sum += dv;
      sumsq += dv * dv;
      n_count += 1;
      n_below += (v < k.below_threshold) ? 1u : 0u;
      vmin = fminf(vmin, v);
      vmax = fmaxf(vmax, v);
      if (want_hist) {
        if (v < k.hist_lo) {
          n_under += 1;
        } else if (v < k.hist_hi) {
          int32_t b = static_cast<int32_t>((dv - static_cast<double>(k.hist_lo)) * k.hist_inv);
          b = b < static_cast<int32_t>(k.n_bins) - 1 ? b : static_cast<int32_t>(k.n_bins) - 1;
          atomicAdd(&lds_hist[b], 1u);
        } else {
          n_over += 1;
        }
      }
    }
    if (k.d_chunk_mean || k.d_chunk_var) {  // uniform over the workgroup
      // mean and population variance of this chunk from one pass (sum and sum of squares in
      // double: the cancellation in E[x^2] - mean^2 costs ~1e-15 relative here), one barrier:
      // the scratch slots alternate with the iteration's parity
      const double dv = active ? static_cast<double>(v) : 0.0;
      const double s12 = wave_sum_pair(dv, dv * dv);  // lane 0: the wave's sum, lane 32: its sum of squares
      double *slot = red_scratch + (parity ? 2 * kWaves : 0);
      parity = !parity;
      const int lane = tid & 63, wave = tid >> 6;
      if ((lane & 31) == 0) slot[(lane ? kWaves : 0) + wave] = s12;
      __syncthreads();
      if (tid == 0) {
        double t1 = slot[0], t2 = slot[kWaves];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
          t1 += slot[w];
          t2 += slot[kWaves + w];
        }
        // A full chunk -- every chunk but the last one of a launch -- needs no divide: t * 2^-8 and t / 256 are the
        // same binary64 for every sum of binary32 values or of their squares (no subnormal double arises; inf and
        // NaN go through alike).  The IEEE divides stay for the one chunk that may be ragged.
        double mean, var;
        if (chunk + 1 < n_chunks) {
          static_assert(kBlock == 256, "the full chunk's reciprocal is 2^-8");
          mean = t1 * 0x1p-8;
          var = t2 * 0x1p-8 - mean * mean;
        } else {
          const double n_in = static_cast<double>(k.n_paths - chunk * kBlock);  // 1 .. kBlock
          mean = t1 / n_in;
          var = t2 / n_in - mean * mean;
        }
        if (k.d_chunk_mean) k.d_chunk_mean[chunk] = static_cast<float>(mean);
        if (k.d_chunk_var) k.d_chunk_var[chunk] = static_cast<float>(var > 0.0 ? var : 0.0);
      }
    }
  }

  if (k.clock_probe && threadIdx.x == 0) {
    atomicAdd(&k.clock_probe[0], __builtin_amdgcn_s_memtime() - clk0);
    atomicAdd(&k.clock_probe[1], __builtin_amdgcn_s_memrealtime() - real0);
  }
  if (want_stats) {
    // per-lane u32 counters cannot overflow: a lane sees < 2^32 chunks
    BlockPartial p;
    p.sum = wave_sum(sum);
    p.sumsq = wave_sum(sumsq);
    p.count = wave_sum(static_cast<unsigned long long>(n_count));
    p.below = wave_sum(static_cast<unsigned long long>(n_below));
    p.underflow = wave_sum(static_cast<unsigned long long>(n_under));
    p.overflow = wave_sum(static_cast<unsigned long long>(n_over));
    p.min = wave_min(vmin);
    p.max = wave_max(vmax);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_part[wave] = p;
    __syncthreads();
    if (tid == 0) {  // one partial per workgroup
      BlockPartial t = wave_part[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        t.sum += wave_part[w].sum;
        t.sumsq += wave_part[w].sumsq;
        t.count += wave_part[w].count;
        t.below += wave_part[w].below;
        t.underflow += wave_part[w].underflow;
        t.overflow += wave_part[w].overflow;
        t.min = fminf(t.min, wave_part[w].min);
        t.max = fmaxf(t.max, wave_part[w].max);
      }
      k.partials[blockIdx.x] = t;
    }
    if (want_hist) {  // LDS atomics of all waves are complete after the barrier above
      for (uint32_t b = threadIdx.x; b < k.n_bins; b += kGroup) {
        const uint32_t c = lds_hist[b];
        if (c) atomicAdd(&k.d_hist[b], static_cast<unsigned long long>(c));
      }
    }
  }
}

template <int kDiv, bool kDense, bool kWide>
struct BlocksWalk {  // aux: the block length
  static __device__ __forceinline__ BlockLayout layout(const KernelArgs &k, uint32_t block_len) {
    return {block_len, blocks_copy_words(k.table_len, kWide), static_cast<uint32_t>(kBlockSeg) % k.table_len};
  }
  static __device__ __forceinline__ uint32_t table_words(const KernelArgs &k, uint32_t) { return blocks_table_words(k.table_len, kWide); }
  static __device__ __forceinline__ void stage(const KernelArgs &k, uint32_t block_len, float *lds_table, uint32_t threads) {
    stage_block_table<kWide>(k, layout(k, block_len), lds_table, threads);
  }
  static __device__ __forceinline__ float simulate(const KernelArgs &k, uint32_t block_len, const DrawRegs &dr, const float *lds_table,
                                                   uint64_t path) {
    return simulate_block_path<kDiv, kDense, kWide>(k, layout(k, block_len), dr, lds_table, path);
  }
};
// The block walk inside blocks_body.  Eight waves per SIMD: the loop holds a base, a value and eight multipliers
// beside the Philox state.
template <int kDiv, bool kDense, bool kWide>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8)))
void blocks_kernel(const KernelArgs k, const uint32_t vgrid, const uint32_t block_len) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  blocks_body<BlocksWalk<kDiv, kDense, kWide>>(k, vgrid, block_len, lds_raw);
}

// ---- stationary bootstrap: table paths in runs of geometric length ---------------------------------
//
// smmc_engine_simulate_stationary (csrc/smmc_stationary.cpp; DESIGN.md, "Stationary bootstrap").  Every period t of a
// path has a candidate start c_t -- exactly the index the table stream draws for that path at period t, block_starts'
// digits -- and a 16-bit renewal field f_t out of a second Philox block (t / 8, id lo, id hi, kRenewTag) with the same
// key: the path starts a new run at c_t when f_t < q and otherwise reads on, i_t = i_{t-1} + 1, wrapped to 0 at T.
// Every lane has boundaries of its own, so nothing of block_run's wave-uniform run applies; but both counters are
// wave-uniform, the scalar rounds 0 and 1 of philox4x32_10<kPhiloxUniformBlock> hold for both blocks, and the loop has
// no divergent branch: the choice is a select.  One plain copy of the table is staged: the wrap is a select too.
constexpr uint32_t kRenewTag = 2u;  // fourth counter word of the renewal fields: 0 is the table's, odd ones the Gaussian series'
constexpr int kRenewSeg = 8;        // periods per block of renewal fields: four words, two 16-bit fields each

// Field j = 0 .. 7 of a block of renewal fields: word j / 2, the low half for an even j, the high half for an odd one.
__device__ __forceinline__ uint32_t renewal_field(const uint32_t (&f)[4], int j) { return (j & 1) ? f[j >> 1] >> 16 : f[j >> 1] & 0xffffu; }

// The table index of a period from the index of the period before (prev < T), the period's candidate start and its
// renewal field; `first` (wave-uniform): period 0, which takes its candidate whatever the field.  The device-side draw
// of the stationary bootstrap, for whichever kernel walks such paths.
__device__ __forceinline__ uint32_t stationary_index(uint32_t prev, uint32_t candidate, uint32_t field, uint32_t q, uint32_t T, bool first) {
  const uint32_t next = prev + 1u;
  const uint32_t on = next >= T ? 0u : next;
  return (first || field < q) ? candidate : on;
}

// Periods 8 g .. 8 g + n - 1 of a path, n = 8 (kFull) or the path's last 1 .. 7 (wave-uniform).
// stationary_rows (stationary-bootstrap plans, below) gathers candidates and fields the same way, line for line: a
// change to how either is taken here must be made there too.
template <bool kExactDiv, bool kDense, bool kFull>
__device__ __forceinline__ void stationary_segment(const KernelArgs &k, uint32_t q, const DrawRegs &dr, const float *lds, uint32_t path_lo,
                                                   uint32_t path_hi, uint32_t g, uint32_t n, uint32_t &idx, float &total) {
  uint32_t c[kRenewSeg];
  if constexpr (kDense) {
    block_starts<true>(k, dr, path_lo, path_hi, g, c);
  } else {  // four candidates per block of the table stream: blocks 2 g and 2 g + 1 (g < 2^29)
    uint32_t lo[4], hi[4] = {0u, 0u, 0u, 0u};
    block_starts<false>(k, dr, path_lo, path_hi, 2u * g, lo);
    if (kFull || n > 4u) block_starts<false>(k, dr, path_lo, path_hi, 2u * g + 1u, hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = lo[j];
      c[4 + j] = hi[j];
    }
  }
  uint32_t f[4];
  philox4x32_10<kPhiloxUniformBlock>(g, path_lo, path_hi, kRenewTag, k.key0, k.key1, dr, f);
#pragma unroll
  for (int j = 0; j < kRenewSeg; ++j) {
    if (kFull || static_cast<uint32_t>(j) < n) {
      idx = stationary_index(idx, c[j], renewal_field(f, j), q, k.table_len, j == 0 && g == 0u);
      total = compound<kExactDiv>(total, lds[idx]);
    }
  }
}

template <int kDiv, bool kDense>
__device__ __forceinline__ float simulate_stationary_path(const KernelArgs &k, uint32_t q, const DrawRegs &dr, const float *lds, uint64_t path) {
  constexpr bool kExactDiv = kDiv == kDivExact;
  const uint32_t path_lo = static_cast<uint32_t>(path);
  const uint32_t path_hi = static_cast<uint32_t>(path >> 32);
  float total = k.initial_capital;
  bool left_window = false;
  uint32_t idx = 0;
  const uint32_t full = k.n_periods / kRenewSeg;
  for (uint32_t g = 0; g < full; ++g) {
    stationary_segment<kExactDiv, kDense, true>(k, q, dr, lds, path_lo, path_hi, g, kRenewSeg, idx, total);
    // one test per 8 periods, the span the host derives the window for (smmc_capi.cpp, divide_kind)
    if constexpr (kDiv == kDivChecked) left_window |= !(total > k.chk_lo && total < k.chk_hi);  // NaN leaves too
  }
  const uint32_t rem = k.n_periods - full * kRenewSeg;
  if (rem) stationary_segment<kExactDiv, kDense, false>(k, q, dr, lds, path_lo, path_hi, full, rem, idx, total);  // wave-uniform
  if constexpr (kDiv == kDivChecked) {
    if (left_window) total = simulate_stationary_path<kDivExact, kDense>(k, q, dr, lds, path);
  }
  return total;
}

template <int kDiv, bool kDense>
struct StationaryWalk {  // aux: renew_q16, the renewal probability in units of 2^-16
  static __device__ __forceinline__ uint32_t table_words(const KernelArgs &k, uint32_t) { return k.table_len; }
  static __device__ __forceinline__ void stage(const KernelArgs &k, uint32_t, float *lds_table, uint32_t threads) {
    for (uint32_t i = threadIdx.x; i < k.table_len; i += threads) lds_table[i] = k.table_a[i];
  }
  static __device__ __forceinline__ float simulate(const KernelArgs &k, uint32_t q, const DrawRegs &dr, const float *lds_table, uint64_t path) {
    return simulate_stationary_path<kDiv, kDense>(k, q, dr, lds_table, path);
  }
};
// The stationary walk inside blocks_body: its chunk walk, outputs and epilogue as they are.  65 .. 69 VGPRs, seven waves
// per SIMD: eight candidates and four words of fields are live beside the Philox state and the round keys; asked for
// eight waves (64 VGPRs, as blocks_kernel) the compiler spills one 64-bit accumulator around the period loop.
template <int kDiv, bool kDense>
__global__ __launch_bounds__(kBlock)
void stationary_kernel(const KernelArgs k, const uint32_t vgrid, const uint32_t renew_q16) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  blocks_body<StationaryWalk<kDiv, kDense>>(k, vgrid, renew_q16, lds_raw);
}

// ---- regime-switching Gaussian paths: a two-state Markov law for returns ---------------------------
//
// smmc_engine_simulate_regimes (csrc/smmc_regimes.cpp; include/smmc.h and DESIGN.md, "Regime-switching Gaussian paths",
// state the contract).  Every period t of a path has a standard normal z_t -- exactly the one portfolio_kernel draws for
// asset 0, Philox block (t / 4, id lo, id hi, 1) over the v3 tables staged at scale 1 with dr.shift100 = 0 -- and a
// 16-bit field f_t out of a second Philox block (t / 8, id lo, id hi, kRegimeTag), taken by renewal_field.  The path's
// regime flips when f_t < leave_q16[regime before] (period 0: regime 1 when f_0 < start1_q16), and the multiplier is
// fma(std[s_t], z_t, 100 + mean[s_t]).  Every lane has a state of its own, both counters are wave-uniform, the scalar
// first rounds of philox4x32_10<kPhiloxUniformBlock> hold for all three blocks of a segment, and the loop has no
// divergent branch: the state is a lane mask, scale and shift are selects of kernel arguments.
constexpr uint32_t kRegimeTag = 4u;  // fourth counter word of the regime fields: even tags are field streams (0 the table's, 2 the renewal's)
constexpr int kRegimeSeg = 8;        // periods per block of fields, as kRenewSeg: two blocks of normals

// Periods 8 g .. 8 g + n - 1 of a path, n = 8 (kFull) or the path's last 1 .. 7 (wave-uniform).  The eight states are
// formed first, so the field words are dead when the compounding chain begins (as stationary_rows forms its rows).
template <bool kExactDiv, bool kFull>
__device__ __forceinline__ void regimes_segment(const KernelArgs &k, const RegimeArgs &r, const DrawRegs &dr, const float *lds,
                                                uint32_t path_lo, uint32_t path_hi, uint32_t g, uint32_t n, bool &state, float &total) {
  uint32_t f[4];
  philox4x32_10<kPhiloxUniformBlock>(g, path_lo, path_hi, kRegimeTag, k.key0, k.key1, dr, f);
  // period 0 comes from "regime 0" (the state's initial value) with start1_q16 in leave_q16[0]'s place: a scalar select
  const uint32_t q0 = g == 0u ? r.start1_q16 : r.leave_q16[0];
  bool s[kRegimeSeg];
#pragma unroll
  for (int j = 0; j < kRegimeSeg; ++j) {
    s[j] = false;
    if (kFull || static_cast<uint32_t>(j) < n) {
      const uint32_t q = state ? r.leave_q16[1] : (j == 0 ? q0 : r.leave_q16[0]);
      state = state != (renewal_field(f, j) < q);
      s[j] = state;
    }
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (half == 0 || kFull || n > 4u) {  // the second block of normals only if the segment has more than four periods
      float z[4];  // standard normals: the tables are staged at scale 1, dr.shift100 is 0
      block_multipliers<SMMC_MODE_GAUSSIAN, false, kPhiloxUniformBlock>(k, dr, lds, path_lo, path_hi, 2u * g + half, z);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 4 * half + i;
        if (kFull || static_cast<uint32_t>(j) < n) {
          const float scale = s[j] ? r.scale[1] : r.scale[0], shift = s[j] ? r.shift100[1] : r.shift100[0];
          total = compound<kExactDiv>(total, __builtin_fmaf(scale, z[i], shift));
        }
      }
    }
  }
}

template <int kDiv>
__device__ __forceinline__ float simulate_regimes_path(const KernelArgs &k, const RegimeArgs &r, const DrawRegs &dr, const float *lds,
                                                       uint64_t path) {
  constexpr bool kExactDiv = kDiv == kDivExact;
  const uint32_t path_lo = static_cast<uint32_t>(path);
  const uint32_t path_hi = static_cast<uint32_t>(path >> 32);
  float total = k.initial_capital;
  bool left_window = false;
  bool state = false;
  const uint32_t full = k.n_periods / kRegimeSeg;  // < 2^28: 2 g + 1 is a block index
  for (uint32_t g = 0; g < full; ++g) {
    regimes_segment<kExactDiv, true>(k, r, dr, lds, path_lo, path_hi, g, kRegimeSeg, state, total);
    // one test per 8 periods, the span the host derives the window for (smmc_capi.cpp, divide_kind)
    if constexpr (kDiv == kDivChecked) left_window |= !(total > k.chk_lo && total < k.chk_hi);  // NaN leaves too
  }
  const uint32_t rem = k.n_periods - full * kRegimeSeg;
  if (rem) regimes_segment<kExactDiv, false>(k, r, dr, lds, path_lo, path_hi, full, rem, state, total);  // wave-uniform
  if constexpr (kDiv == kDivChecked) {
    if (left_window) total = simulate_regimes_path<kDivExact>(k, r, dr, lds, path);
  }
  return total;
}

template <int kDiv>
struct RegimesWalk {  // aux: the two regimes' scales, shifts and probabilities
  static __device__ __forceinline__ uint32_t table_words(const KernelArgs &, const RegimeArgs &) { return bm_lds_words(SMMC_MODE_GAUSSIAN); }
  static __device__ __forceinline__ void stage(const KernelArgs &k, const RegimeArgs &, float *lds_table, uint32_t threads) {
    stage_tables<SMMC_MODE_GAUSSIAN>(k, lds_table, threads);  // k.gauss_std is 1.0f: the tables as they are
  }
  static __device__ __forceinline__ float simulate(const KernelArgs &k, const RegimeArgs &r, const DrawRegs &dr, const float *lds_table,
                                                   uint64_t path) {
    return simulate_regimes_path<kDiv>(k, r, dr, lds_table, path);
  }
};
// The regime walk inside blocks_body: its chunk walk, outputs and epilogue as they are.  A family of its own; no
// amdgpu_waves_per_eu: nothing measured asks for one.
template <int kDiv>
__global__ __launch_bounds__(kBlock)
void regimes_kernel(const KernelArgs k, const uint32_t vgrid, const RegimeArgs r) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  blocks_body<RegimesWalk<kDiv>, RegimeArgs>(k, vgrid, r, lds_raw);
}

// ---- the wave walk: the skeleton of checkpoints_kernel, cashflow_kernel and excursions_kernel ------
//
// Three kernels are one program with another step in the middle: the paths of paths_kernel, looked at after every
// period (cash flows, excursions) or after chosen ones (checkpoints).  What they share is written here once; a
// further path statistic is a per-period step and what it emits per chunk, not a fourth copy.  Bound like
// paths_kernel: VALU issue.
//
// Work (wave_chunks).  A WAVE owns a chunk of 64 consecutive paths (one 256-byte store per output) and walks the
// chunks wc = blockIdx.x * kW + wave, + gridDim.x * kW, ...; there is no barrier inside the walk.  Every lane of a
// wave runs a path, also beyond n_paths in the launch's last chunk (the wave reductions want the whole wave; such a
// lane stores and counts nothing), so control flow is wave-uniform throughout.
//
// LDS (walk_setup).  The draw tables sit at address 0 (a table elsewhere costs an address add per gather), the
// kernel's u32 counters -- histograms, per-period counts -- behind them, zeroed here, and behind those, 8-byte
// aligned, the waves' BlockPartial records.  The counters count paths of ONE workgroup: the host refuses a launch in
// which a workgroup would get 2^32 or more (host_wave_walk_grid, smmc_capi.cpp).
//
// Periods (walk_blocks, walk_periods).  k.n_periods / kDraws whole Philox blocks, then the path's partial block, whose
// draws past the last period are dropped; `prefetch(blk)` runs before a block's Philox rounds, `step(j, a, t)` after
// them for draw j, multiplier a, period t (1-based; j is a constant after unrolling).  portfolio_kernel draws K
// multipliers per period and walks the same blocks with a draw of its own; checkpoints_kernel has a block loop of its
// own (a fast and a slow form per block) and takes the other pieces.
//
// Records.  wave_record reduces the wave's 64 values to the wave-uniform sums, extremes and counts of one record
// and makes the LDS bucket adds; where the totals go is the kernel's (checkpoint_record, wave_record_add).  At the
// end fold_wave_partials leaves one BlockPartial per workgroup and record for finalize_kernel, and flush_counters
// adds the non-zero LDS counters to the engine's accumulator with 64-bit atomics.
constexpr uint32_t walk_waves(int mode) { return mode == SMMC_MODE_GAUSSIAN ? 8u : 4u; }  // per workgroup

struct WalkLds {  // wave-uniform
  float *table;             // the draw tables, LDS address 0
  uint32_t *counters;       // [counter_words], zero
  BlockPartial *wave_part;  // behind the counters, 8-byte aligned; as many as the launch's LDS size provides
  uint32_t lane, wave;
};
template <int kMode>
__device__ __forceinline__ uint32_t walk_table_words(const KernelArgs &k) {
  return is_table(kMode) ? k.table_len : bm_lds_words(kMode);
}
// Carves the dynamic LDS ([front_words, the draw tables first][counters][pad][partials]), stages the tables, zeroes
// the counters; ends with a barrier.
template <int kMode>
__device__ __forceinline__ WalkLds walk_setup(const KernelArgs &k, unsigned char *lds_raw, uint32_t front_words, uint32_t counter_words) {
  constexpr uint32_t kGroup = 64u * walk_waves(kMode);
  WalkLds s;
  s.table = reinterpret_cast<float *>(lds_raw);
  s.counters = reinterpret_cast<uint32_t *>(lds_raw) + front_words;
  s.wave_part = reinterpret_cast<BlockPartial *>(reinterpret_cast<uint32_t *>(lds_raw) + ((front_words + counter_words + 1u) & ~1u));
  stage_tables<kMode>(k, s.table, kGroup);
  for (uint32_t i = threadIdx.x; i < counter_words; i += kGroup) s.counters[i] = 0u;
  __syncthreads();
  s.lane = threadIdx.x & 63u;
  s.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return s;
}

// body(i, active, path_lo, path_hi) for every chunk of this wave: path index i of the launch, whether it is below
// n_paths, and the halves of the path's id.
template <int kMode, typename Body>
__device__ __forceinline__ void wave_chunks(const KernelArgs &k, const WalkLds &s, Body body) {
  constexpr uint32_t kW = walk_waves(kMode);
  const uint64_t n_wave_chunks = (k.n_paths + 63u) / 64u;
  for (uint64_t wc = static_cast<uint64_t>(blockIdx.x) * kW + s.wave; wc < n_wave_chunks;
       wc += static_cast<uint64_t>(gridDim.x) * kW) {
    const uint64_t i = wc * 64u + s.lane;
    const uint64_t path = k.first_path + i;
    body(i, i < k.n_paths, static_cast<uint32_t>(path), static_cast<uint32_t>(path >> 32));
  }
}

// The block walk under walk_periods and the portfolio's period loop: n_periods / kDraws whole Philox blocks, then the
// partial block.  draw(blk) makes the block's kDraws draws; step(j, t) consumes draw j at period t (1-based).
template <int kDraws, typename Draw, typename Step>
__device__ __forceinline__ void walk_blocks(uint32_t n_periods, Draw draw, Step step) {
  const uint32_t full = n_periods / kDraws, rem = n_periods - full * kDraws;
  for (uint32_t blk = 0; blk < full; ++blk) {
    draw(blk);
#pragma unroll
    for (int j = 0; j < kDraws; ++j) step(j, blk * kDraws + j + 1u);
  }
  if (rem) {  // wave-uniform: the path's last, partial block
    draw(full);
#pragma unroll
    for (int j = 0; j < kDraws - 1; ++j)
      if (static_cast<uint32_t>(j) < rem) step(j, full * kDraws + j + 1u);
  }
}

template <int kMode, bool kDense, typename Prefetch, typename Step>
__device__ __forceinline__ void walk_periods(const KernelArgs &k, const DrawRegs &dr, const float *lds_table, uint32_t path_lo,
                                             uint32_t path_hi, Prefetch prefetch, Step step) {
  constexpr int kDraws = Draws<kMode, kDense>::value;
  float a[kDraws];
  walk_blocks<kDraws>(
      k.n_periods,
      [&](uint32_t blk) {
        prefetch(blk);
        block_multipliers<kMode, kDense, kPhiloxUniformBlock>(k, dr, lds_table, path_lo, path_hi, blk, a);
      },
      [&](int j, uint32_t t) { step(j, a[j], t); });
}

template <int kShift>
__device__ __forceinline__ float row_shl_min(float v) {  // v[i] = min(v[i], v[i + kShift]) inside each row of 16 lanes
  constexpr int kRowShl = 0x100 + kShift;                 // lanes shifted in from outside the row keep +inf
  const uint32_t o = __builtin_amdgcn_update_dpp(0x7f800000u, __float_as_uint(v), kRowShl, 0xf, 0xf, false);
  return fminf(v, __uint_as_float(o));
}
// min of a over the wave in lane 0, of b in lane 32: the lane movements of wave_sum_pair.  No NaN among the inputs.
__device__ __forceinline__ float wave_min_pair(float a, float b) {
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  float v = fminf(__uint_as_float(s[0]), __uint_as_float(s[1]));
  const auto t = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fminf(__uint_as_float(t[0]), __uint_as_float(t[1]));
  v = row_shl_min<8>(v);
  v = row_shl_min<4>(v);
  v = row_shl_min<2>(v);
  return row_shl_min<1>(v);
}
__device__ __forceinline__ double read_lane(double v, int lane) {
  return join64(__builtin_amdgcn_readlane(lo32(v), lane), __builtin_amdgcn_readlane(hi32(v), lane));
}
__device__ __forceinline__ uint32_t ballot_count(bool pred) {
  return static_cast<uint32_t>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(pred)));
}

// What the wave's values v (lanes with !active: none) add to a record, the record values_stats forms of them; every
// member is wave-uniform.  Two double sums by wave_sum_pair, min and -max by the same lane movements
// (wave_min_pair), the four counters by ballots and scalar population counts, one LDS add per lane inside
// [lo, hi) into the n_bins buckets at lds_hist (n_bins 0: no buckets).  Some 70 VALU instructions.  Every lane of
// the wave must be enabled.
struct WaveRecord {
  double sum, sumsq;
  uint32_t count, below, under, over;
  float min, max;
};
__device__ __forceinline__ WaveRecord wave_record(float v, bool active, float below_threshold, float lo, float hi, double inv,
                                                  uint32_t n_bins, uint32_t *lds_hist) {
  const double dv = static_cast<double>(v);
  const double s12 = wave_sum_pair(active ? dv : 0.0, active ? dv * dv : 0.0);  // lane 0: sum, lane 32: sum of squares
  const bool ordered = active && v == v;  // min and max skip NaN, as fminf / fmaxf do
  const float mm = wave_min_pair(ordered ? v : __builtin_inff(), ordered ? -v : __builtin_inff());  // lane 0: min, lane 32: -max
  WaveRecord r;
  r.count = ballot_count(active);
  r.below = ballot_count(active && v < below_threshold);
  r.under = r.over = 0;
  if (n_bins) {  // uniform
    const bool under = active && v < lo;
    const bool inside = active && !under && v < hi;
    r.under = ballot_count(under);
    r.over = ballot_count(active && !under && !inside);  // >= hi, or NaN
    if (inside) {
      int32_t b = static_cast<int32_t>((dv - static_cast<double>(lo)) * inv);
      b = b < static_cast<int32_t>(n_bins) - 1 ? b : static_cast<int32_t>(n_bins) - 1;
      atomicAdd(&lds_hist[b], 1u);
    }
  }
  r.sum = read_lane(s12, 0);
  r.sumsq = read_lane(s12, 32);
  r.min = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mm), 0));
  r.max = -__uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mm), 32));
  return r;
}

// After the barrier that ends the walk: the kW partials of one record, in wave order, as the workgroup's.
template <uint32_t kW>
__device__ __forceinline__ void fold_wave_partials(const BlockPartial *wave_part, BlockPartial *out) {
  BlockPartial t = wave_part[0];
  for (uint32_t w = 1; w < kW; ++w) partial_add(t, wave_part[w]);
  *out = t;
}
// After that barrier too (the LDS adds of all waves are complete): out[b] += counters[b] for the non-zero ones.
template <uint32_t kGroup>
__device__ __forceinline__ void flush_counters(const uint32_t *counters, uint32_t n, unsigned long long *out) {
  for (uint32_t b = threadIdx.x; b < n; b += kGroup) {
    const uint32_t c = counters[b];
    if (c) atomicAdd(&out[b], static_cast<unsigned long long>(c));
  }
}

// A lane's running record of the final values of its paths, as paths_kernel forms it: the accumulators stay per lane
// from chunk to chunk (a wave record per chunk would add the doubles in another order) and are reduced over the wave
// once, at the end of the walk.  cashflow_kernel and portfolio_kernel.
struct LaneRecord {
  double sum = 0.0, sumsq = 0.0;
  uint32_t n_count = 0, n_below = 0, n_under = 0, n_over = 0;
  float vmin = __builtin_inff(), vmax = -__builtin_inff();
  // an active lane's value v; want_hist: one LDS add into the k.n_bins buckets at lds_hist
  __device__ __forceinline__ void add(const KernelArgs &k, float v, bool want_hist, uint32_t *lds_hist) {
    const double dv = static_cast<double>(v);
    sum += dv;
    sumsq += dv * dv;
    n_count += 1;
    n_below += (v < k.below_threshold) ? 1u : 0u;
    vmin = fminf(vmin, v);
    vmax = fmaxf(vmax, v);
    if (want_hist) {
      if (v < k.hist_lo) {
        n_under += 1;
      } else if (v < k.hist_hi) {
        int32_t b = static_cast<int32_t>((dv - static_cast<double>(k.hist_lo)) * k.hist_inv);
        b = b < static_cast<int32_t>(k.n_bins) - 1 ? b : static_cast<int32_t>(k.n_bins) - 1;
        atomicAdd(&lds_hist[b], 1u);
      } else {
        n_over += 1;
      }
    }
  }
  // the wave's partial into s.wave_part[s.wave]; every lane of the wave calls
  __device__ __forceinline__ void store(const WalkLds &s) const {
    BlockPartial p;
    p.sum = wave_sum(sum);
    p.sumsq = wave_sum(sumsq);
    p.count = wave_sum(static_cast<unsigned long long>(n_count));
    p.below = wave_sum(static_cast<unsigned long long>(n_below));
    p.underflow = wave_sum(static_cast<unsigned long long>(n_under));
    p.overflow = wave_sum(static_cast<unsigned long long>(n_over));
    p.min = wave_min(vmin);
    p.max = wave_max(vmax);
    if (s.lane == 0) s.wave_part[s.wave] = p;
  }
};

// ---- checkpoints: the value distribution at chosen periods ---------------------------------------
//
// smmc_engine_simulate_checkpoints: the paths of paths_kernel, reduced not only at the end but after each of
// c.n chosen periods -- one statistics record per checkpoint instead of a trajectory per path.  A wave walk (above);
// HBM sees 4 B per path (d_final) or nothing.
//
// Where the checkpoint test sits.  The sorted periods are kernel arguments, read with scalar loads; `next_p`, the
// next one, lives in an SGPR.  One scalar compare per Philox block decides between the block of simulate_path
// (no checkpoint inside: the same instructions) and the slow form, which keeps the block's kDraws prefix values
// and records those next_p names.  The path's last, partial block takes the slow form too.
//
// A record (checkpoint_record).  wave_record's totals, with the buckets in the [checkpoint][bucket] u32 histogram
// behind the draw tables, are ADDED BY LANE ck to the accumulators it holds in registers: lane k of a wave keeps
// checkpoint k (SMMC_MAX_CHECKPOINTS is the wave size), ten registers per lane for any number of checkpoints, no
// LDS, and a fixed order -- a wave's chunks in ascending order.  At the end the waves put their partials over the
// draw tables (no longer needed), thread k folds the kW of checkpoint k in wave order and writes
// partials[k][blockIdx.x]; finalize_checkpoints_kernel folds those in a fixed order, one workgroup per record.
struct CheckpointArgs {
  uint32_t n;                              // 1 .. SMMC_MAX_CHECKPOINTS
  uint32_t periods[SMMC_MAX_CHECKPOINTS];  // strictly increasing, 1 .. n_periods
};
static_assert(SMMC_MAX_CHECKPOINTS <= 64, "lane k of a wave accumulates checkpoint k");

// LDS words in front of the histogram: the draw tables, later the waves' partials [kW][n]
constexpr uint32_t checkpoint_front_words(uint32_t table_words, uint32_t waves, uint32_t n) {
  const uint32_t part_words = waves * n * static_cast<uint32_t>(sizeof(BlockPartial) / 4u);
  return ((table_words > part_words ? table_words : part_words) + 1u) & ~1u;
}

struct CheckpointAcc {  // what lane k holds for checkpoint k
  double sum, sumsq;
  uint32_t count, below, under, over;
  float min, max;
};

// The wave's values v go into checkpoint ck (wave-uniform): lane ck adds the wave's totals to its registers.
__device__ __forceinline__ void checkpoint_record(const KernelArgs &k, uint32_t ck, float v, bool active, uint32_t lane,
                                                  uint32_t *lds_hist, CheckpointAcc &acc) {
  const WaveRecord r = wave_record(v, active, k.below_threshold, k.hist_lo, k.hist_hi, k.hist_inv, k.n_bins, lds_hist + ck * k.n_bins);
  if (lane == ck) {
    acc.sum += r.sum;
    acc.sumsq += r.sumsq;
    acc.count += r.count;
    acc.below += r.below;
    acc.under += r.under;
    acc.over += r.over;
    acc.min = fminf(acc.min, r.min);
    acc.max = fmaxf(acc.max, r.max);
  }
}

template <int N>
__device__ __forceinline__ float pick(const float (&t)[N], uint32_t j) {  // t[j], j wave-uniform: N - 1 selects
  float v = t[0];
#pragma unroll
  for (int i = 1; i < N; ++i) {
    v = (j == static_cast<uint32_t>(i)) ? t[i] : v;
    asm("" : "+v"(v));  // left alone the compiler turns the chain into an array in scratch memory
  }
  return v;
}

template <int kMode, bool kExactDiv, bool kDense>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void checkpoints_kernel(const KernelArgs k, const CheckpointArgs c) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t hist_words = c.n * k.n_bins;
  const WalkLds s = walk_setup<kMode>(k, lds_raw, checkpoint_front_words(walk_table_words<kMode>(k), kW, c.n), hist_words);
  uint32_t *lds_hist = s.counters;  // [c.n][k.n_bins]; s.wave_part is not used: this launch's LDS ends with the histogram
  const uint32_t lane = s.lane, wave = s.wave;
  CheckpointAcc acc;
  acc.sum = acc.sumsq = 0.0;
  acc.count = acc.below = acc.under = acc.over = 0u;
  acc.min = __builtin_inff();
  acc.max = -__builtin_inff();
  const DrawRegs dr = make_draw_regs(k);

  const uint32_t n_blocks = (k.n_periods + kDraws - 1) / kDraws;  // >= 1: a checkpoint is a period >= 1
  const uint32_t last_j = k.n_periods - (n_blocks - 1) * kDraws - 1;  // the final value's place in the last block
  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float total = k.initial_capital;
    uint32_t ck = 0, next_p = c.periods[0];
    for (uint32_t blk = 0; blk < n_blocks; ++blk) {
      float a[kDraws];
      block_multipliers<kMode, kDense, kPhiloxUniformBlock>(k, dr, s.table, path_lo, path_hi, blk, a);
      const uint32_t p_end = (blk + 1) * kDraws;  // periods done after this block
      if (next_p > p_end && p_end <= k.n_periods) {  // uniform: no checkpoint inside, not the partial block
#pragma unroll
        for (int j = 0; j < kDraws; ++j) total = compound<kExactDiv>(total, a[j]);
      } else {
        float t[kDraws];
#pragma unroll
        for (int j = 0; j < kDraws; ++j) {
          total = compound<kExactDiv>(total, a[j]);
          t[j] = total;
        }
        while (next_p <= p_end) {  // next_p <= n_periods, or none is left
          checkpoint_record(k, ck, pick(t, next_p - blk * kDraws - 1), active, lane, lds_hist, acc);
          ++ck;
          next_p = ck < c.n ? c.periods[ck] : 0xffffffffu;
        }
        if (p_end > k.n_periods) total = pick(t, last_j);  // draws past the last period are dropped
      }
    }
    if (active && k.d_final) k.d_final[i] = total;
  });

  __syncthreads();  // every wave is through with the draw tables, and its LDS adds are complete
  BlockPartial *part = reinterpret_cast<BlockPartial *>(lds_raw);  // [kW][c.n]
  if (lane < c.n) {
    BlockPartial p;
    p.sum = acc.sum;
    p.sumsq = acc.sumsq;
    p.count = acc.count;
    p.below = acc.below;
    p.underflow = acc.under;
    p.overflow = acc.over;
    p.min = acc.min;
    p.max = acc.max;
    part[wave * c.n + lane] = p;
  }
  __syncthreads();
  if (threadIdx.x < c.n) {
    BlockPartial t = part[threadIdx.x];
    for (uint32_t w = 1; w < kW; ++w) partial_add(t, part[w * c.n + threadIdx.x]);
    k.partials[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = t;
  }
  flush_counters<kGroup>(lds_hist, hist_words, k.d_hist);
}

// One workgroup per checkpoint: folds its bucket counts out of the accumulator (left zero, as finalize_kernel
// leaves it) and its n_partials workgroup partials in a fixed order, and writes record blockIdx.x.
constexpr int kCheckpointFinalizeBlock = 256;
__global__ __launch_bounds__(kCheckpointFinalizeBlock) void finalize_checkpoints_kernel(
    const BlockPartial *partials, uint32_t n_partials, unsigned char *records, uint32_t n_bins,
    unsigned long long *hist_acc) {
  const size_t record_bytes = sizeof(smmc_stats) + sizeof(unsigned long long) * n_bins;
  smmc_stats *out = reinterpret_cast<smmc_stats *>(records + blockIdx.x * record_bytes);
  unsigned long long *hist = reinterpret_cast<unsigned long long *>(out + 1);
  for (uint32_t b = threadIdx.x; b < n_bins; b += kCheckpointFinalizeBlock) {
    unsigned long long *src = hist_acc + static_cast<size_t>(blockIdx.x) * n_bins + b;
    const unsigned long long v = *src;
    if (v) *src = 0;
    hist[b] = v;
  }
  __shared__ BlockPartial sh[kCheckpointFinalizeBlock];
  const BlockPartial *mine = partials + static_cast<size_t>(blockIdx.x) * n_partials;
  BlockPartial t;
  partial_identity(t);
  for (uint32_t j = threadIdx.x; j < n_partials; j += kCheckpointFinalizeBlock) partial_add(t, mine[j]);
  sh[threadIdx.x] = t;
  __syncthreads();
  for (uint32_t s = kCheckpointFinalizeBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) partial_add(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const BlockPartial &r = sh[0];
    out->count = r.count;
    out->below = r.below;
    out->underflow = r.underflow;
    out->overflow = r.overflow;
    out->sum = r.sum;
    out->sumsq = r.sumsq;
    out->min = r.min;
    out->max = r.max;
    out->n_bins = n_bins;
    out->reserved = 0;
  }
}

// ---- keepdata: every trajectory, path-major ------------------------------------
//
// mc_data of mc_simulations_keepdata (src/simulations.cpp:139-186): row i holds the
// n_periods + 1 values of path i (values[0] = initial capital).  This one IS
// HBM-bound: 4 (P + 1) bytes per path.
//
// A lane owns a path, so one period's values of a wave form a COLUMN of the output;
// rows are 4 (P + 1) bytes apart, i.e. start at arbitrary 4-byte offsets.  Writing
// tile-aligned runs leaves partial 128-byte lines in L2 for a whole tile time, and
// their in-flight footprint (~ waves x 16 KB) is the size of the aggregate L2: that
// version ran at 2.7 TB/s.  Here every lane runs its path with its own DELAY of phi
// columns, phi = (float address of its row start) mod kTile, so that column c of
// tile t of EVERY row lands on a float address that is c mod kTile: each wave-wide
// store covers whole aligned 128-byte windows, complete lines the moment they are
// written.  Only the first and last window of a row are partial.
//
// Column g of lane r holds value index s = g - phi_r (0 = initial capital, s >= 1 =
// after period s - 1).  Philox blocks stay wave-uniform in time: with D draws per
// block, at column group G every lane draws block G - q_r (phi_r + 1 = D q_r + rho_r),
// and draw j of it belongs to tile column D G + rho_r + j.  The residual shift rho_r is
// the position of the row inside its LDS slots (see kSlots below); a first version
// applied it with a log2(D)-stage register shifter over two blocks (4.25 VALU per
// value, 1.49 ms where this one takes 1.15).
//
// Column groups are of two kinds: INTERIOR groups (every lane inside its own row: no
// predicate at all) and the few general ones at the two ends of the row, where a
// lane's write goes to a trash word when the column is not its own.
//
// Row junctions.  Adjacent rows share the 128-byte line in which one ends and the next
// begins; written as two partial windows a whole path apart in time, that line reaches
// HBM as two masked writes (measured: 3.8 TB/s pattern ceiling instead of 6.2).  So the
// window in which a row ends is completed with the HEAD of the next row and stored whole,
// and the next row's lane skips its own (partial) first window.  The head costs no second
// simulation: the next row is the next LANE, which drew exactly those values in its own
// first window (the phases line up by construction: the next row starts where this one
// ends), so after the first tile every lane hands its first window to the lane before it
// (one wave shuffle per column, once per 64 paths) and keeps its neighbour's in registers
// until its own row ends.  Junctions between waves (lane 63 | lane 0) stay unmerged.  Needs
// rows of at least two windows so that a window holds at most one junction (`merge`).
// An earlier form ran the next row's stream a second time next to the lane's own in the
// tail groups: +15 % arithmetic, and too much for Gaussian mode to gain from merging.
//
// Store phase: a lane takes FOUR columns of one row (16-byte stores, 8 rows x 128 bytes
// per instruction); for interior tiles (all 32 columns of all 64 rows valid) the byte
// offset of row r is ((phi_0 + r L) & ~31) - phi_0 floats from the wave's first row.
constexpr int kKeepdataMaxBlock = 768;  // 12 waves: 3 per SIMD, so up to 168 VGPRs (the kernel keeps a 32-value window per lane)
// slots per tile row of keepdata_kernel, and the words reserved per row (the larger of its two strides)
constexpr int keepdata_slots(int tile, int draws) { return tile + draws; }
constexpr int keepdata_row_words(int tile, int draws) {
  const int slots = keepdata_slots(tile, draws);
  const int odd = slots | 1, even = slots + ((6 - slots % 4) % 4);
  return odd > even ? odd : even;
}
template <int kMode, bool kExactDiv, bool kDense, int kTile>
__global__ __launch_bounds__(kKeepdataMaxBlock) void keepdata_kernel(const KernelArgs k) {
  constexpr int kDraws = Draws<kMode, kDense>::value;
  // A row of the tile has kTile + kDraws slots; logical column c of row r sits in slot
  // kDraws - rho_r + c, which makes the slot a lane WRITES (kDraws + column-group base + j)
  // independent of its rho: bank = (stride * lane + const) mod 32.  (With rho in the write address,
  // bank = (7 + L mod 8) * lane for a stride of 39: 8-way conflicts at L = 361, and the LDS was the
  // bottleneck -- SQ_LDS_BANK_CONFLICT 73 % of SQ_LDS_IDX_ACTIVE.)  Slots from kTile up hold the
  // last group's columns that belong to the next tile and move down by kTile after the store
  // phase.  Row stride: odd when the row length is even, = 2 mod 4 when it is odd (writes then
  // 2-way, which ds_write_b32 absorbs): either way the store phase's reads -- 4 rows x 8 quads
  // per lane group, each row offset by its own rho -- are conflict-free.
  constexpr int kSlots = keepdata_slots(kTile, kDraws);
  constexpr int kStrideOdd = kSlots | 1;
  constexpr int kStrideEven = kSlots + ((6 - kSlots % 4) % 4);  // smallest >= kSlots that is 2 mod 4
  constexpr int kRowMax = keepdata_row_words(kTile, kDraws);
  constexpr int kQuads = kTile / 4;                          // 16-byte pieces of a window
  constexpr int kRowsPerStore = 64 / kQuads;                 // rows one wave-wide store covers
  constexpr uint32_t kGroupsPerTile = kTile / kDraws;        // psi <= kTile: q <= kGroupsPerTile
  // dynamic LDS: [tables][one tile per wave][one trash word per thread]; the host picks the
  // number of waves (smmc_engine_simulate_keepdata: 4 in table mode, 12 in Gaussian mode)
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *lds_table = reinterpret_cast<float *>(lds_raw);
  const uint32_t table_words = is_table(kMode) ? k.table_len : bm_lds_words(kMode);
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  const uint32_t stride = ((k.n_periods + 1) & 1u) ? kStrideEven : kStrideOdd;  // uniform
  float *tile = lds_table + table_words + wave * (64 * kRowMax);
  float *my_row = tile + lane * stride;
  float *my_trash = lds_table + table_words + n_waves * (64 * kRowMax) + tid;
  stage_tables<kMode>(k, lds_table, blockDim.x);
  __syncthreads();
  const DrawRegs dr = make_draw_regs(k);

  const uint32_t sub = lane / kQuads, quad = lane % kQuads;  // store phase: row sub + kRowsPerStore it, columns 4 quad .. + 3
  const uint32_t n_periods = k.n_periods;
  const uint32_t row_len32 = n_periods + 1;  // the host keeps n_periods below 2^24 for keepdata
  const uint64_t row_len = row_len32;
  const uint64_t base_f = reinterpret_cast<uintptr_t>(k.d_traj) >> 2;  // float address of d_traj[0]
  const bool merge = row_len32 >= 2u * kTile;  // uniform
  // groups [kGroupsPerTile, tail_start) are interior: 0 <= period < n_periods for every lane
  const uint32_t tail_start = n_periods / kDraws;
  const bool small_rows = row_len32 <= (1u << 22);  // 64 rows of bytes fit 32-bit offsets
  // a wave takes 64 consecutive paths at a time; no workgroup-level step after the staging barrier
  const uint64_t n_wave_chunks = (k.n_paths + 63) / 64;
  for (uint64_t wc = static_cast<uint64_t>(blockIdx.x) * n_waves + wave; wc < n_wave_chunks;
       wc += static_cast<uint64_t>(gridDim.x) * n_waves) {
    const uint64_t wave_first = wc * 64;  // first path of this wave
    const uint64_t left = k.n_paths - wave_first;
    const uint32_t rows_here = left < 64 ? static_cast<uint32_t>(left) : 64u;
    const uint64_t i = wave_first + lane;
    const bool active = lane < rows_here;
    // lanes past the end still run a (discarded) path so the wave stays converged
    const uint64_t path = k.first_path + i;
    const uint32_t path_lo = static_cast<uint32_t>(path), path_hi = static_cast<uint32_t>(path >> 32);

    const uint32_t phi0 = static_cast<uint32_t>(base_f + wave_first * row_len) & (kTile - 1);  // uniform
    const uint32_t phi = (phi0 + lane * row_len32) & (kTile - 1);
    const uint32_t psi = phi + 1;             // own period = column - psi
    const uint32_t q = psi / kDraws;          // whole blocks of delay
    const uint32_t rho = psi % kDraws;        // residual shift: the row's slot offset is kDraws - rho
    const uint32_t g_next = phi + row_len32;  // column that holds values[0] of the next row
    // columns this wave has to draw: up to the last value of its most delayed row (all 32 phases
    // occur in a wave unless the row length shares a factor with the window: rows of 64 values on
    // an aligned base need two tiles, not three)
    uint32_t phi_max = phi;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t other = __shfl_xor(phi_max, off, 64);
      phi_max = other > phi_max ? other : phi_max;
    }
    const uint32_t last_col = phi_max + n_periods;
    const uint32_t n_tiles_w = last_col / kTile + 1u;  // <= n_tiles
    float *wr = my_row + kDraws;                 // own draws: slot kDraws + cb + j
    float *logical = my_row + kDraws - rho;      // logical column 0
    float *wave_base = k.d_traj + wave_first * row_len;

    // The store phase's view of the chunk, fixed over its tiles: iteration `it` of a lane handles row
    // r = sub + it * kRowsPerStore.  st_lds: where the row's four columns sit in the LDS tile;
    // st_off: byte offset from the wave's first row to those columns in the row's window 0 (can be
    // negative by up to 4 phi0 for the first row); st_span: first column the row stores << 26 |
    // number of columns it stores (0 for rows past the end of the launch).  A row goes to memory
    // from its first WHOLE window (the lane of the row before wrote the shared one) through the
    // end of its last window (which includes the next row's head), except across waves and at the
    // two ends of the launch.
    uint32_t st_lds[kQuads], st_off[kQuads], st_span[kQuads];
    {
      const uint32_t rows_left = left < 0xFFFFFFFFull ? static_cast<uint32_t>(left) : 0xFFFFFFFFu;
#pragma unroll
      for (int it = 0; it < kQuads; ++it) {
        const uint32_t r = sub + it * kRowsPerStore;
        const uint32_t tf = phi0 + r * row_len32;
        const uint32_t phi_r = tf & (kTile - 1);
        const uint32_t last = phi_r + n_periods;
        const uint32_t lo = (!merge || phi_r == 0 || r == 0) ? phi_r : static_cast<uint32_t>(kTile);
        const uint32_t hi = (!merge || r == 63 || r + 1 >= rows_left) ? last : (last | (kTile - 1));
        st_lds[it] = r * stride + (kDraws + 4u * quad - ((phi_r + 1u) & (kDraws - 1u)));
        st_off[it] = (tf - phi_r - phi0 + 4u * quad) * 4u;
        st_span[it] = r < rows_here ? (lo << 26) | (hi - lo + 1u) : 0u;
      }
    }
    float total = k.initial_capital;
    float next_head[kTile];  // the next row's first window (merge)
    logical[phi] = k.initial_capital;  // values[0]
    for (uint32_t t = 0; t < n_tiles_w; ++t) {
      const uint32_t g0 = t * kTile;
      const uint32_t grp0 = g0 / kDraws;
      const bool interior_tile = grp0 >= kGroupsPerTile && grp0 + kGroupsPerTile <= tail_start;  // uniform
      float last[kDraws];  // the tile's last group (interior tiles)
      if (interior_tile) {
        // every group of the tile is interior: straight-line code, so that the next group's
        // Philox rounds and table reads overlap this group's compounding chain (the kernel runs
        // at 2-3 waves per SIMD, LDS-limited: instruction-level parallelism has to hide latency)
#pragma unroll
        for (uint32_t cb = 0; cb < kTile; cb += kDraws) {
          float a[kDraws];
          block_multipliers<kMode, kDense>(k, dr, lds_table, path_lo, path_hi, grp0 + cb / kDraws - q, a);
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {
            total = compound<kExactDiv>(total, a[j]);
            wr[cb + j] = total;
            if (cb == kTile - kDraws) last[j] = total;
          }
        }
      } else
      for (uint32_t cb = 0; cb < kTile; cb += kDraws) {
        if (g0 + cb > last_col) break;  // uniform: nothing to draw beyond
        const uint32_t grp = (g0 + cb) / kDraws;
        float a[kDraws];
        block_multipliers<kMode, kDense>(k, dr, lds_table, path_lo, path_hi, grp - q, a);
        if (grp >= kGroupsPerTile && grp < tail_start) {  // uniform: every lane is inside its own row
          float *dst = wr + cb;
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {
            total = compound<kExactDiv>(total, a[j]);
            dst[j] = total;
          }
        } else {
          const uint32_t p0 = kDraws * (grp - q);  // wraps below zero: fails the test
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {
            const bool own = p0 + j < n_periods;
            const float next = compound<kExactDiv>(total, a[j]);
            total = own ? next : total;
            float *dst = own ? wr + cb + j : my_trash;
            *dst = total;
          }
        }
      }
      // The tile is private to this wave: order LDS writes before the row reads.
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      if (merge && t == 0) {  // uniform: every lane's first window goes to the lane of the row before
#pragma unroll
        for (uint32_t c = 0; c < kTile; ++c) next_head[c] = __shfl_down(logical[c], 1, 64);
      }
      char *base_b = reinterpret_cast<char *>(wave_base);
      const uint32_t g0_b = g0 * 4u, g_first = g0 + 4u * quad;
      if (rows_here == 64 && small_rows && g0 >= kTile && g0 + (kTile - 1) <= n_periods) {
        // interior tile: every column of every row is that row's own
#pragma unroll
        for (int it = 0; it < kQuads; ++it) {
          const float *s = tile + st_lds[it];
          const float4 v = make_float4(s[0], s[1], s[2], s[3]);
          const uint32_t boff = st_off[it] + g0_b;  // in 32 bits: the true, non-negative offset (g0 > phi0)
          *reinterpret_cast<float4 *>(base_b + boff) = v;
        }
      } else if (small_rows) {
        // a tile in which rows begin or end: column g of the row is stored iff g - lo < count
        // (unsigned: columns before lo wrap to huge values)
#pragma unroll
        for (int it = 0; it < kQuads; ++it) {
          const uint32_t count = st_span[it] & 0x03FFFFFFu, d = g_first - (st_span[it] >> 26);
          const float *s = tile + st_lds[it];
          const uint32_t boff = st_off[it] + g0_b;  // non-negative whenever the element is stored
          if (d < count && d + 3u < count) {
            *reinterpret_cast<float4 *>(base_b + boff) = make_float4(s[0], s[1], s[2], s[3]);
          } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e)
              if (d + e < count) *reinterpret_cast<float *>(base_b + (boff + 4u * e)) = s[e];
          }
        }
      } else {  // rows of more than 2^22 values: 64-bit offsets
        const uint32_t rho_mask = kDraws - 1;
        for (uint32_t r = sub; r < rows_here; r += kRowsPerStore) {
          const uint32_t phi_r = (phi0 + r * row_len32) & (kTile - 1);
          const uint64_t row_global = wave_first + r;
          const uint32_t last = phi_r + n_periods;
          const uint32_t lo = (!merge || phi_r == 0 || r == 0) ? phi_r : static_cast<uint32_t>(kTile);
          const uint32_t hi = (!merge || r == 63 || row_global + 1 >= k.n_paths) ? last : (last | (kTile - 1));
          float *row_ptr = wave_base + (static_cast<int64_t>(r) * row_len32 - phi_r);
          const float *s = tile + r * stride + (kDraws + 4u * quad - ((phi_r + 1u) & rho_mask));
          const uint32_t g = g_first;
          if (g >= lo && g + 3u <= hi) {
            *reinterpret_cast<float4 *>(row_ptr + g) = make_float4(s[0], s[1], s[2], s[3]);
          } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e)
              if (g + e >= lo && g + e <= hi) row_ptr[g + e] = s[e];
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      // This row ends in the NEXT tile: the rest of its last window is the head of the next row,
      // which that row's lane drew in ITS first window and handed over (lane 63's next row belongs
      // to another wave: that junction stays unmerged).  Written whole; the slot move below and
      // the next tile's own draws then overwrite the columns that are still this row's.
      const bool ends_next = merge && g_next / kTile == t + 1 && lane != 63;
      if (t + 3 >= n_tiles_w && ends_next) {
#pragma unroll
        for (uint32_t c = 0; c < kTile; ++c) logical[c] = next_head[c];
      }
      // slots [kTile, ...) are the next tile's slots [0, ...): the last group (from registers: all
      // of it is this row's), or whatever the general groups left there -- of which a row that ends
      // in the next tile keeps only its own columns (slot j is logical column j - kDraws + rho)
      if (interior_tile) {
#pragma unroll
        for (int j = 0; j < kDraws; ++j) my_row[j] = last[j];
      } else {
        const uint32_t keep = ends_next ? (g_next & (kTile - 1)) + kDraws - rho : static_cast<uint32_t>(kDraws);
        float up[kDraws];
#pragma unroll
        for (int j = 0; j < kDraws; ++j) up[j] = my_row[kTile + j];
#pragma unroll
        for (uint32_t j = 0; j < kDraws; ++j) {
          float *dst = j < keep ? my_row + j : my_trash;
          *dst = up[j];
        }
      }
    }
    if (active && k.d_final) k.d_final[i] = total;
  }
}

// ---- keepdata, comb form: every wave-wide store a set of WHOLE, unshared 128-byte lines ---------------
//
// keepdata_kernel above gives a wave 64 ADJACENT rows.  Adjacent rows share the line in which one ends
// and the next begins, their phases modulo a line all differ (per-lane delays, predicates, slot
// offsets), and a row of 361 values spans up to 392 columns of wave time.  Here a wave takes 64
// STREAMS of K consecutive rows whose first rows are 32 rows apart (stream l starts at row
// 2048 super + 32 l + K w): all 64 streams then start at the SAME offset phi inside a 128-byte line.
// Consequences:
//   * every piece of control is wave-uniform (SGPRs, scalar branches): the column cursor, the Philox
//     block index, row ends, tile flushes.  No lane is ever outside its stream, no predicate, no
//     per-lane delay: the draw and the step + ~2.5 VALU per stored value (20.2 in Gaussian mode; the tile
//     kernel with stream v2's draw: 39.8, this one: 33.0).
//   * a stream is stored from its first WHOLE line through the line in which its last row ends, and
//     it computes the head of the row that follows (the same counter stream: bit-identical to what
//     that row's own stream computes) to complete that line: every 128-byte line of the output is
//     written whole, once, by one wave -- also across waves and workgroups, where the tile kernel
//     leaves junction lines in two pieces.  tools/ubench_store_pattern.hip: this pattern streams at
//     6.1-6.4 TB/s, adjacent rows with shared lines at 3.8.  The extra work is <= 31 values per
//     stream (1.1 % at K = 4, P = 360).
//   * the LDS tile is column-major, [32 + D columns][64 lanes + 1]: a block's values go out as the
//     lane's own word of consecutive columns (conflict-free, no address arithmetic beyond one add per
//     block), the store phase reads 4 columns x 8 streams per 32 lanes (bank = column + stream:
//     conflict-free) and needs no per-lane state at all: stream r's line of tile t sits at
//     base + (r 32 L - phi + 32 t) floats, i.e. a scalar base plus one lane-constant offset.
// Needs n_periods to be a multiple of the draws per Philox block (a row is then whole blocks).
// Launch: rows [0, 2048 n_super) of the call; the host gives the remaining < 2048 rows to
// keepdata_kernel (whose first row's partial first line then repeats the head this kernel's last
// stream already wrote: same values).  d_final is filled by a separate gather (final_column_kernel).
constexpr int kCombMaxBlock = 1024;
constexpr int kCombColStride = 65;  // words between two columns of a tile: 64 lanes + 1
constexpr int comb_tile_words(int draws) { return (32 + draws) * kCombColStride; }

template <int kMode, bool kExactDiv, bool kDense, int kBlocksPerStep>
__global__ __launch_bounds__(kCombMaxBlock) void keepdata_comb_kernel(const KernelArgs k, const uint32_t rows_per_stream,
                                                                      const uint64_t n_wave_chunks, const uint64_t n_rows_total,
                                                                      unsigned long long *next_chunk) {
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *lds_table = reinterpret_cast<float *>(lds_raw);
  const uint32_t table_words = is_table(kMode) ? k.table_len : bm_lds_words(kMode);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n_waves = blockDim.x >> 6;
  float *tile = lds_table + table_words + wave * comb_tile_words(kDraws);
  stage_tables<kMode>(k, lds_table, blockDim.x);
  __syncthreads();
  const DrawRegs dr = make_draw_regs(k);

  const uint32_t K = rows_per_stream, waves_per_super = 32u / K;
  const uint32_t n_periods = k.n_periods, row_len = n_periods + 1u, n_blocks = n_periods / kDraws;
  const uint32_t sub = lane >> 3, quad = lane & 7u;
  const uint64_t base_f = reinterpret_cast<uintptr_t>(k.d_traj) >> 2;
  float *mine = tile + lane;                                           // column c of this lane's stream: mine[65 c]
  const float *take = tile + (4u * quad) * kCombColStride + sub;       // store phase: take[65 e + 8 it]
  const uint32_t lane_off = sub * (128u * row_len) + 16u * quad;       // bytes; row_len <= 2^20 (host)
  const uint64_t it_step = 1024ull * row_len;                          // bytes between two store iterations (8 streams)
  // One address register per store iteration, opaque to the compiler: with a single base and 32
  // immediate offsets it pairs the reads of two ITERATIONS into one ds_read2_b32 and then moves every
  // value into place for the 16-byte store (one v_mov per stored value); with a base of its own each
  // iteration pairs its own columns, and the pairs land in the store's registers.
  uint32_t take_off[8];
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    take_off[it] = 8u * it;
    asm volatile("" : "+v"(take_off[it]));
  }

  // Wave chunks are handed out by a counter (*next_chunk, zeroed by the host before the launch): a
  // wave takes the next one when it is done.  A chunk is 64 K rows, a launch a few chunks per wave
  // (6 at 1.5e6 rows of 1001 values), so a fixed round-robin left whole waves idle for the last round
  // (1.71 ms where this takes 1.5x).  Every wave leaves the loop once the counter
  // has passed the end.
  (void)n_waves;
  for (;;) {
    unsigned long long taken = 0;
    if (lane == 0) taken = atomicAdd(next_chunk, 1ull);
    const uint64_t wc = (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(taken >> 32))) << 32) |
                        __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(taken));
    if (wc >= n_wave_chunks) break;
    const uint64_t super = wc / waves_per_super;
    const uint32_t w = static_cast<uint32_t>(wc % waves_per_super);
    const uint64_t row0 = super * 2048ull + static_cast<uint64_t>(w) * K;  // first row of stream 0
    const uint32_t phi = static_cast<uint32_t>(base_f + row0 * row_len) & 31u;
    const uint32_t own = K * row_len;                                      // columns of the stream's own rows
    const uint32_t n_tiles = (phi + own + 31u) / 32u;                      // through the line its last row ends in
    // the row after stream r's last row exists for every r, unless this wave holds the call's last row
    const bool all_have_next = row0 + 32ull * 63ull + K < n_rows_total;
    uint64_t path = k.first_path + row0 + 32ull * lane;
    uint32_t path_lo = static_cast<uint32_t>(path), path_hi = static_cast<uint32_t>(path >> 32);
    char *line0 = reinterpret_cast<char *>(k.d_traj) + (static_cast<int64_t>(row0 * row_len) - phi) * 4;  // tile 0 of stream 0

    uint32_t col = phi, blk = 0, t = 0;
    float total = k.initial_capital;
    mine[col * kCombColStride] = total;  // values[0]
    col += 1;

    // Columns 0..31 of the tile are complete (one line of every stream): store them, move the columns
    // beyond down.  Returns true after the stream's last line.
    auto flush = [&]() -> bool {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      const bool first_partial = t == 0 && phi != 0;                 // streams start inside this line
      const bool last_tile = t + 1u == n_tiles;
      char *line_t = line0 + t * 128u;
      if (!first_partial && (!last_tile || all_have_next)) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const float *s = take + take_off[it];
          const float4 v = make_float4(s[0], s[kCombColStride], s[2 * kCombColStride], s[3 * kCombColStride]);
          *reinterpret_cast<float4 *>(line_t + it * it_step + lane_off) = v;
        }
      } else if (!first_partial || row0 == 0) {
        // the call's first line (stream 0 of the first wave: columns from phi on) or the line in
        // which the call's last row ends (no row follows: columns up to its last value)
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const uint32_t r = sub + 8u * it;
          const float *s = take + 8 * it;
          uint32_t lo = 0u, hi = 31u;
          if (first_partial) {
            lo = phi;
            hi = (r == 0u) ? 31u : 0u;  // hi < lo: nothing (every other stream's first line belongs to the stream before it)
          }
          if (last_tile && !(row0 + 32ull * r + K < n_rows_total)) hi = (phi + own - 1u) & 31u;
#pragma unroll
          for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t c = 4u * quad + e;
            if (c >= lo && c <= hi)
              *reinterpret_cast<float *>(line_t + it * it_step + lane_off + 4u * e) = s[e * kCombColStride];
          }
        }
      }
      if (last_tile) return true;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      // columns 32 .. col - 1 (at most kDraws of them) open the next tile
#pragma unroll
      for (int j = 0; j < kDraws; ++j) mine[j * kCombColStride] = mine[(32 + j) * kCombColStride];
      col -= 32u;
      t += 1;
      return false;
    };

    bool done = false;
    while (!done) {
      // kBlocksPerStep Philox blocks of the row are drawn together: independent instruction streams
      // for the scheduler to interleave (the kernel runs at under 4 waves per SIMD, LDS-limited);
      // their compounding chains follow one after the other.  The host guarantees that a row is a
      // whole number of steps.
      float a[kBlocksPerStep][kDraws];
      block_multipliers_multi<kMode, kDense, kBlocksPerStep, true>(k, dr, lds_table, path_lo, path_hi, blk, a);
#pragma unroll
      for (int b = 0; b < kBlocksPerStep; ++b) {
        if (done) break;
        float *dst = mine + col * kCombColStride;
#pragma unroll
        for (int j = 0; j < kDraws; ++j) {
          total = compound<kExactDiv>(total, a[b][j]);
          dst[j * kCombColStride] = total;
        }
        col += kDraws;
        if (b == kBlocksPerStep - 1) {
          blk += kBlocksPerStep;
          if (blk == n_blocks) {  // uniform: the next row (the stream's own, or the head that completes its last line)
            blk = 0;
            path += 1;
            path_lo = static_cast<uint32_t>(path);
            path_hi = static_cast<uint32_t>(path >> 32);
            total = k.initial_capital;
            mine[col * kCombColStride] = total;
            col += 1;
          }
        }
        if (col >= 32u) done = flush();  // uniform
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

// d_final[i] = last value of row i of a path-major trajectory array (the comb kernel's final values).
__global__ __launch_bounds__(kBlock) void final_column_kernel(const float *traj, uint64_t n_rows, uint32_t row_len, float *d_final) {
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_rows;
       i += static_cast<uint64_t>(gridDim.x) * kBlock)
    d_final[i] = traj[i * row_len + (row_len - 1u)];
}

// Device self-test of the divide shortcut against the compiler's IEEE divide over the
// binary32 patterns [lo, hi): *count += mismatches of div100<false>(x) vs x / 100.0f.
__global__ __launch_bounds__(kBlock) void selftest_kernel(uint32_t lo, uint32_t hi,
                                                          unsigned long long *count) {
  unsigned long long bad = 0;
  const uint64_t n = static_cast<uint64_t>(hi) - lo;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const float x = __uint_as_float(lo + static_cast<uint32_t>(i));
    if (__float_as_uint(div100<false>(x)) != __float_as_uint(x / 100.0f)) ++bad;
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, bad);
}

// Device self-test of the draws: item i takes its four "Philox" words from words[4 i ..] and writes the
// Draws<kMode, kDense>::value multipliers they give to out -- the tables staged and the registers made exactly
// as the path kernels do (stage_tables at LDS offset 0, make_draw_regs), so that every radius bin, sector and
// digit can be reached with chosen words instead of waiting for a seed that hits it.  form 0: one item per
// trip through multipliers_of_words; form 1: items 2 i, 2 i + 1 through multipliers_of_words_multi<.., 2> (a
// ragged last item is drawn with a copy of itself and stored once).
template <int kMode, bool kDense>
__global__ __launch_bounds__(kBlock) void draw_words_kernel(const KernelArgs k, const uint32_t *words, uint64_t n, int form,
                                                            float *out) {
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *lds_table = reinterpret_cast<float *>(lds_raw);
  stage_tables<kMode>(k, lds_table, kBlock);
  __syncthreads();
  const DrawRegs dr = make_draw_regs(k);
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (form == 0) {
    for (uint64_t i = first; i < n; i += stride) {
      uint32_t u[4];
      float a[kDraws];
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = words[i * 4 + j];
      multipliers_of_words<kMode, kDense>(k, dr, lds_table, u, a);
#pragma unroll
      for (int j = 0; j < kDraws; ++j) out[i * kDraws + j] = a[j];
    }
  } else {
    for (uint64_t i = first; 2 * i < n; i += stride) {
      const uint64_t item[2] = {2 * i, 2 * i + 1 < n ? 2 * i + 1 : 2 * i};
      uint32_t u[2][4];
      float a[2][kDraws];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) u[b][j] = words[item[b] * 4 + j];
      multipliers_of_words_multi<kMode, kDense, 2>(k, dr, lds_table, u, a);
#pragma unroll
      for (int j = 0; j < kDraws; ++j) out[item[0] * kDraws + j] = a[0][j];
      if (item[1] != item[0]) {
#pragma unroll
        for (int j = 0; j < kDraws; ++j) out[item[1] * kDraws + j] = a[1][j];
      }
    }
  }
}

// ---- cash flows: a withdrawal or contribution after every period's return -------------------------
//
// smmc_engine_simulate_cashflow ("Cash flows"): the draws of paths_kernel, and after each period's
//   g = (v * a) / 100             update_fund, as compound<>()
// the step, every operation a binary32 rounding of its own (__fmul_rn, __fadd_rn, __fsub_rn: nothing may fuse)
//   w = amount + g * fraction,  v' = g - w
//   live lane, v' > floor:     v = v', paid += w
//   live lane, !(v' > floor):  depleted at this period: v = 0, paid += max(g, 0), ruin_period = t  (NaN is depleted)
//   depleted lane:             nothing changes; its draws are still made, so the stream position of a path never
//                              depends on what happened to it
// Bound like paths_kernel: VALU issue.  Nine VALU instructions per period on top of the compounding chain: multiply,
// add, subtract, compare, the select of v, max, the select of what is paid, its add, the select of ruin_period.  The
// "live" flag is a lane mask in a scalar register pair and is combined with the compare on the scalar unit;
// depletion is per lane, control flow stays wave-uniform.  A depleted lane holds v = 0, so its product and
// its divide (either form: 0 * a is exact in both) stay 0; the mask, not the arithmetic, keeps it from coming back
// when a contribution (amount < 0) would lift v' above the floor.
//
// A wave walk (the skeleton above checkpoints_kernel): work split, LDS layout, the period walk and the epilogue
// pieces are its.
//
// Schedule.  kVarying = false: amount and fraction are kernel arguments, two scalar registers, no loads.
// kVarying = true: the period index is wave-uniform, so the entries of a Philox block are read with scalar loads
// through the constant address space (one wide load per array and block, the walk's prefetch: issued before the
// block's Philox rounds); the host pads both arrays to whole blocks.  No per-lane global load in the loop.
//
// Outputs.  A lane adds its final value to per-lane statistics accumulators as paths_kernel does (one partial per
// workgroup, folded by finalize_kernel; they stay per lane: a wave record per chunk would add the doubles in another
// order), one LDS add into the final-value histogram and one into the [n_periods + 1] depletion counters.
typedef const __attribute__((address_space(4))) float *const_float_ptr;  // scalar (uniform) loads

template <bool kExactDiv>
__device__ __forceinline__ void cashflow_step(float a, float amount, float fraction, float floor, uint32_t t, float &v,
                                              float &paid, uint32_t &ruin, bool &alive) {
  const float g = compound<kExactDiv>(v, a);
  const float w = __fadd_rn(amount, __fmul_rn(g, fraction));
  const float vn = __fsub_rn(g, w);
  const bool goes_on = alive && vn > floor;  // false for NaN
  const bool dies = alive && !goes_on;
  v = goes_on ? vn : 0.0f;
  paid = __fadd_rn(paid, goes_on ? w : fmaxf(g, 0.0f));  // a depleted lane: g = 0 (or NaN from 0 * inf: fmaxf gives 0)
  ruin = dies ? t : ruin;
  alive = goes_on;
}

template <int kMode, bool kExactDiv, bool kDense, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void cashflow_kernel(const KernelArgs k, const CashflowArgs c) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const WalkLds s = walk_setup<kMode>(k, lds_raw, walk_table_words<kMode>(k), k.n_periods + 1u + k.n_bins);
  uint32_t *lds_dep = s.counters;                     // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + (k.n_periods + 1u);  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float v = k.initial_capital, paid = 0.0f;
    uint32_t ruin = 0u;
    bool alive = true;
    float am[kDraws], fr[kDraws];
    walk_periods<kMode, kDense>(
        k, dr, s.table, path_lo, path_hi,
        [&](uint32_t blk) {  // the block's schedule entries (padded to whole blocks)
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {
            am[j] = kVarying ? amounts[blk * kDraws + j] : c.amount;
            fr[j] = kVarying ? fractions[blk * kDraws + j] : c.fraction;
          }
        },
        [&](int j, float a, uint32_t t) { cashflow_step<kExactDiv>(a, am[j], fr[j], c.floor, t, v, paid, ruin, alive); });
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, k.n_periods + 1u, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// d_out[i] = acc[i], and acc is left zero for the next launch (as finalize_kernel leaves the bucket accumulator).
__global__ __launch_bounds__(kBlock) void finalize_depleted_kernel(unsigned long long *acc, uint32_t n, unsigned long long *d_out) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const unsigned long long v = acc[i];
    if (v) acc[i] = 0;
    d_out[i] = v;
  }
}

// ---- excursions: what happened along a path -------------------------------------------------------
//
// smmc_engine_simulate_excursions ("Excursions"): the draws and the compounding of paths_kernel, and
// after each period's value v = v_t, every operation a binary32 rounding of its own (__fmul_rn: nothing may fuse),
// every comparison false for NaN (selects on ordered compares, never v_max / v_min: those return the other operand
// for a NaN and do not keep the sign of a zero):
//   if (v > peak) peak = v;  if (v < low) low = v
//   if (fl(v * dd_peak) < fl(dd_low * peak)) dd_peak = peak, dd_low = v, dd_period = t      the peak updated above
//   run = (v < peak) ? run + 1 : 0;  longest = max(longest, run)
//   if (first_below == 0 && v < lower) first_below = t;  if (first_reach == 0 && v >= target) first_reach = t
// and once per path drawdown = fl(fl(dd_peak - dd_low) / dd_peak), an IEEE divide outside the loop.
// Bound like paths_kernel: VALU issue.  By source 18 VALU instructions per period on top of the compounding chain:
// two compares and two selects for the extremes, the two cross products, their compare and three selects, a compare,
// an add, a select and an integer max for the time under water, a compare and a select per level.  The two "not yet
// hit" flags are lane masks in scalar register pairs, combined with the compares on the scalar unit, as
// cashflow_step's `alive`; the period index is wave-uniform; control flow stays wave-uniform.
//
// A wave walk (the skeleton above checkpoints_kernel).  Outputs: up to eight coalesced 256-byte stores per wave chunk;
// TWO records (final value, drawdown), each reduced over the wave per chunk (wave_record) and added to the wave's
// partial in LDS (wave_record_add), left as one partial per workgroup (k.partials, x.dd_partials; finalize_kernel
// folds each); one LDS add per lane into each of two histograms and of two [n_periods + 1] first-passage counter
// arrays.
struct ExcursionLane {
  float peak, low, dd_peak, dd_low;
  uint32_t dd_period, run, longest, first_below, first_reach;
};

template <bool kExactDiv>
__device__ __forceinline__ void excursion_step(float a, float lower, float target, uint32_t t, float &v, ExcursionLane &s,
                                               bool &no_below, bool &no_reach) {
  v = compound<kExactDiv>(v, a);
  s.peak = v > s.peak ? v : s.peak;
  s.low = v < s.low ? v : s.low;
  const bool deeper = __fmul_rn(v, s.dd_peak) < __fmul_rn(s.dd_low, s.peak);  // strict; false for NaN
  s.dd_peak = deeper ? s.peak : s.dd_peak;
  s.dd_low = deeper ? v : s.dd_low;
  s.dd_period = deeper ? t : s.dd_period;
  s.run = v < s.peak ? s.run + 1u : 0u;
  s.longest = s.longest > s.run ? s.longest : s.run;
  const bool hit_below = no_below && v < lower;
  const bool hit_reach = no_reach && v >= target;
  s.first_below = hit_below ? t : s.first_below;
  s.first_reach = hit_reach ? t : s.first_reach;
  no_below = no_below && !hit_below;
  no_reach = no_reach && !hit_reach;
}

// The wave's values v are added to the wave's own partial record in LDS: wave_record's totals, then one
// read-modify-write by lane 0.  Two records' accumulators in registers (20 per lane) would cost the Gaussian kernel
// its eighth wave per SIMD; here they cost none.  The order is fixed: a wave's chunks ascending.
__device__ __forceinline__ void wave_record_add(BlockPartial *part, float v, bool active, uint32_t lane, float below_threshold,
                                                float lo, float hi, double inv, uint32_t n_bins, uint32_t *lds_hist) {
  const WaveRecord r = wave_record(v, active, below_threshold, lo, hi, inv, n_bins, lds_hist);
  if (lane == 0) {
    BlockPartial t = *part;
    t.sum += r.sum;
    t.sumsq += r.sumsq;
    t.count += r.count;
    t.below += r.below;
    t.underflow += r.under;
    t.overflow += r.over;
    t.min = fminf(t.min, r.min);
    t.max = fmaxf(t.max, r.max);
    *part = t;
  }
}

template <int kMode, bool kExactDiv, bool kDense>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void excursions_kernel(const KernelArgs k, const ExcursionArgs x) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t n_at = k.n_periods + 1u;
  const WalkLds s = walk_setup<kMode>(k, lds_raw, walk_table_words<kMode>(k), 2u * n_at + 2u * k.n_bins);  // wave_part: [2][kW]
  uint32_t *lds_below_at = s.counters;           // [n_periods + 1]
  uint32_t *lds_reach_at = lds_below_at + n_at;  // [n_periods + 1]
  uint32_t *lds_hist = lds_reach_at + n_at;      // [n_bins], the final values
  uint32_t *lds_dd_hist = lds_hist + k.n_bins;   // [n_bins], the drawdowns

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_dd_stats = x.dd_partials != nullptr;
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dd_hist = want_dd_stats && k.n_bins != 0;
  const bool want_below_at = x.d_below_at != nullptr, want_reach_at = x.d_reach_at != nullptr;
  const uint32_t lane = s.lane;
  BlockPartial *part = s.wave_part + s.wave, *dd_part = s.wave_part + kW + s.wave;  // this wave's own, until the barrier
  if (lane == 0) {
    partial_identity(*part);
    partial_identity(*dd_part);
  }
  const DrawRegs dr = make_draw_regs(k);

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float v = k.initial_capital;
    ExcursionLane e = {v, v, v, v, 0u, 0u, 0u, 0u, 0u};
    bool no_below = true, no_reach = true;
    walk_periods<kMode, kDense>(
        k, dr, s.table, path_lo, path_hi, [](uint32_t) {},
        [&](int, float a, uint32_t t) { excursion_step<kExactDiv>(a, x.lower, x.target, t, v, e, no_below, no_reach); });
    const float drawdown = __fdiv_rn(__fsub_rn(e.dd_peak, e.dd_low), e.dd_peak);  // the path's one IEEE divide
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (x.d_peak) x.d_peak[i] = e.peak;
      if (x.d_low) x.d_low[i] = e.low;
      if (x.d_drawdown) x.d_drawdown[i] = drawdown;
      if (x.d_drawdown_period) x.d_drawdown_period[i] = e.dd_period;
      if (x.d_underwater) x.d_underwater[i] = e.longest;
      if (x.d_first_below) x.d_first_below[i] = e.first_below;
      if (x.d_first_reach) x.d_first_reach[i] = e.first_reach;
      if (want_below_at) atomicAdd(&lds_below_at[e.first_below], 1u);  // first_* <= n_periods
      if (want_reach_at) atomicAdd(&lds_reach_at[e.first_reach], 1u);
    }
    if (want_stats)  // uniform: the whole wave
      wave_record_add(part, v, active, lane, k.below_threshold, k.hist_lo, k.hist_hi, k.hist_inv, want_hist ? k.n_bins : 0u, lds_hist);
    if (want_dd_stats)
      wave_record_add(dd_part, drawdown, active, lane, x.drawdown_threshold, 0.0f, 1.0f, x.dd_hist_inv, want_dd_hist ? k.n_bins : 0u,
                      lds_dd_hist);
  });

  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (threadIdx.x == 0) {
    if (want_stats) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
    if (want_dd_stats) fold_wave_partials<kW>(s.wave_part + kW, &x.dd_partials[blockIdx.x]);
  }
  // two arrays share a loop, as before the kernels shared a skeleton (flush_counters takes one array)
  for (uint32_t b = threadIdx.x; b < n_at; b += kGroup) {
    const uint32_t nb = lds_below_at[b], nr = lds_reach_at[b];
    if (want_below_at && nb) atomicAdd(&x.d_below_at[b], static_cast<unsigned long long>(nb));
    if (want_reach_at && nr) atomicAdd(&x.d_reach_at[b], static_cast<unsigned long long>(nr));
  }
  for (uint32_t b = threadIdx.x; b < k.n_bins; b += kGroup) {
    const uint32_t nf = lds_hist[b], nd = lds_dd_hist[b];
    if (want_hist && nf) atomicAdd(&k.d_hist[b], static_cast<unsigned long long>(nf));
    if (want_dd_hist && nd) atomicAdd(&x.d_dd_hist[b], static_cast<unsigned long long>(nd));
  }
}

// ---- cash-flow sweeps: up to eight constant schedules on the same paths ----------------------------
//
// smmc_engine_simulate_cashflow_sweep (csrc/smmc_sweep.cpp; include/smmc.h and DESIGN.md, "Cash-flow sweeps", state
// the contract): scenario sc of a sweep is cashflow_kernel<..., kVarying = false> with (amount, fraction, floor)[sc].
// The draw of a period depends on (seed, path id, period) alone, so ONE block_multipliers per Philox block serves
// all scenarios; per draw an unrolled loop makes the kS cashflow_steps, each on its own v, paid, ruin and `alive`
// (a lane mask in a scalar register pair, as in cashflow_kernel).  The 3 kS parameters are kernel arguments, scalar
// registers; the loop loads nothing beyond the draw's gathers; control flow stays wave-uniform.
//
// kS is 2, 4 or 8: the host pads a request to the next of them with copies of its last scenario, and c.n says how
// many are real -- a padded scenario is stepped (the loop is unrolled at kS) and nothing of it is ever stored,
// counted or recorded.
//
// Records.  kS per-lane records would take 10 kS registers; instead every chunk's values are reduced over the wave
// (wave_record) and added to the wave's partial of that scenario in LDS (wave_record_add), as excursions_kernel does
// for its two records (hence this kernel's place behind it): some 70 VALU per wave, chunk and scenario beside the 13 per lane and period of the step.
// The order is fixed (a wave's chunks ascending, waves in order, workgroups in finalize's order), but it is not
// cashflow_kernel's: the two double sums of a scenario differ from the single call's in the last places.
//
// LDS (walk_setup): [draw tables][c.n][n_periods + 1] depletion counters][c.n][n_bins] buckets][pad][kS][kW] partials].
// Epilogue: thread sc folds scenario sc's kW partials into k.partials[sc][workgroup]; both counter arrays go to
// the accumulator with flush_counters, scenario-major like the outputs.
template <int kMode, bool kExactDiv, bool kDense, int kS>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void cashflow_sweep_kernel(const KernelArgs k, const SweepArgs c) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  static_assert(kS >= 1 && kS <= SMMC_MAX_SWEEP, "1 .. SMMC_MAX_SWEEP scenarios");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t n_at = k.n_periods + 1u;
  const WalkLds s = walk_setup<kMode>(k, lds_raw, walk_table_words<kMode>(k), c.n * (n_at + k.n_bins));  // wave_part: [kS][kW]
  uint32_t *lds_dep = s.counters;             // [c.n][n_periods + 1]
  uint32_t *lds_hist = lds_dep + c.n * n_at;  // [c.n][n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  const uint32_t lane = s.lane;
  BlockPartial *part = s.wave_part + s.wave;  // scenario sc: part[sc * kW], this wave's own until the barrier
  if (lane == 0) {
#pragma unroll
    for (int sc = 0; sc < kS; ++sc) partial_identity(part[sc * kW]);
  }
  const DrawRegs dr = make_draw_regs(k);

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float v[kS], paid[kS];
    uint32_t ruin[kS];
    bool alive[kS];
#pragma unroll
    for (int sc = 0; sc < kS; ++sc) {
      v[sc] = k.initial_capital;
      paid[sc] = 0.0f;
      ruin[sc] = 0u;
      alive[sc] = true;
    }
    walk_periods<kMode, kDense>(
        k, dr, s.table, path_lo, path_hi, [](uint32_t) {},
        [&](int, float a, uint32_t t) {
#pragma unroll
          for (int sc = 0; sc < kS; ++sc)
            cashflow_step<kExactDiv>(a, c.amount[sc], c.fraction[sc], c.floor[sc], t, v[sc], paid[sc], ruin[sc], alive[sc]);
        });
#pragma unroll
    for (int sc = 0; sc < kS; ++sc) {
      if (static_cast<uint32_t>(sc) >= c.n) continue;  // uniform: a padded scenario leaves nothing
      const size_t at = static_cast<size_t>(sc) * k.n_paths + i;
      if (active) {
        if (k.d_final) k.d_final[at] = v[sc];
        if (c.d_paid) c.d_paid[at] = paid[sc];
        if (c.d_ruin_period) c.d_ruin_period[at] = ruin[sc];
        if (want_dep) atomicAdd(&lds_dep[sc * n_at + ruin[sc]], 1u);  // ruin <= n_periods
      }
      if (want_stats)  // uniform: the whole wave
        wave_record_add(part + sc * kW, v[sc], active, lane, k.below_threshold, k.hist_lo, k.hist_hi, k.hist_inv,
                        want_hist ? k.n_bins : 0u, lds_hist + sc * k.n_bins);
    }
  });

  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x < c.n)
    fold_wave_partials<kW>(s.wave_part + threadIdx.x * kW, &k.partials[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, c.n * n_at, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, c.n * k.n_bins, k.d_hist);
}

// ---- portfolios: jointly drawn assets, weights, periodic rebalancing ------------------------------
//
// smmc_engine_simulate_portfolio (csrc/smmc_portfolio.cpp; include/smmc.h and DESIGN.md, "Portfolios", state the
// contract).  A lane carries K holdings; a period draws K multipliers jointly, compounds each holding with
// compound<>() and, every R periods, sets the holdings to the weights' shares of their sum.  R and the period index
// are wave-uniform: the rebalance is a uniform branch behind a scalar countdown (no modulo in the loop).  A wave walk:
// work split, LDS carving, the block walk (walk_blocks) and the epilogue pieces are the skeleton's; the record of the
// final values is formed as cashflow_kernel forms it (LaneRecord).  Bound like its siblings: VALU issue.
//
// Table mode.  The asset table sits at LDS address 0, one row per month padded to 1, 2 or 4 words
// (portfolio_row_words), so a row is ONE ds_read_b32 / b64 / b128 at index << 2 | 3 | 4; the row indices are
// block_starts' with table_len = n_rows -- the indices SMMC_MODE_TABLE draws -- and one Philox block serves D periods of
// all assets.
// Gaussian mode.  K Philox blocks per four periods, (blk, id lo, id hi, 1 + 2 j): they differ in a compile-time word
// only, so the scalarised first rounds of philox4x32_10<kPhiloxUniformBlock> apply to each, and philox4x32_10_multi interleaves the K
// chains.  The v3 tables are staged once with gauss_std = 1.0f, the draw's additive term is 0.0f (the host sets both):
// multipliers_of_words_multi then yields STANDARD normals, and the multiplier is the contract's chain of fused
// multiply-adds over L's row, j = 0 upwards from s_k.  The additions of V_t are __fadd_rn, the weight products
// __fmul_rn: nothing may be re-associated or contracted.
// The row at LDS byte address `at`, a multiple of the row's 4, 8 or 16 bytes.
template <int K>
__device__ __forceinline__ void load_asset_row_at(uint32_t at, float (&a)[K]) {
  static_assert(K >= 1 && K <= SMMC_MAX_ASSETS, "1 .. 4 assets");
  if constexpr (K == 1) {
    a[0] = lds_load_at<float>(at);
  } else if constexpr (K == 2) {
    const f32x2_t r = lds_load_at<f32x2_t>(at);
    a[0] = r.x;
    a[1] = r.y;
  } else {
    const f32x4_t r = lds_load_at<f32x4_t>(at);
    a[0] = r.x;
    a[1] = r.y;
    a[2] = r.z;
    if constexpr (K == 4) a[3] = r.w;
  }
}
template <int K>
__device__ __forceinline__ void load_asset_row(uint32_t row, float (&a)[K]) {
  load_asset_row_at<K>(row << (K == 1 ? 2 : K == 2 ? 3 : 4), a);
}

// The multipliers a[j][k] of asset k at draw j of Philox block `blk` (wave-uniform) of a path.
template <int kMode, bool kDense, int K>
__device__ __forceinline__ void portfolio_multipliers(const KernelArgs &k, const PortfolioArgs &p, const DrawRegs &dr,
                                                      const float *lds_table, uint32_t path_lo, uint32_t path_hi, uint32_t blk,
                                                      float (&a)[Draws<kMode, kDense>::value][K]) {
  constexpr int kDraws = Draws<kMode, kDense>::value;
  if constexpr (is_table(kMode)) {
    uint32_t row[kDraws];
    block_starts<kDense>(k, dr, path_lo, path_hi, blk, row);
#pragma unroll
    for (int j = 0; j < kDraws; ++j) load_asset_row<K>(row[j], a[j]);
  } else {
    uint32_t u[K][4];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      u[i][0] = blk;
      u[i][1] = path_lo;
      u[i][2] = path_hi;
      u[i][3] = 1u + 2u * static_cast<uint32_t>(i);
    }
    philox4x32_10_multi<K, true>(u, k.key0, k.key1, dr);
    float z[K][kDraws];  // standard normals: the tables are staged at scale 1, dr.shift100 is 0
    multipliers_of_words_multi<SMMC_MODE_GAUSSIAN, false, K>(k, dr, lds_table, u, z);
#pragma unroll
    for (int j = 0; j < kDraws; ++j)
#pragma unroll
      for (int i = 0; i < K; ++i) {
        float acc = p.shift100[i];
#pragma unroll
        for (int m = 0; m <= i; ++m) acc = __builtin_fmaf(p.factor[i * SMMC_MAX_ASSETS + m], z[m][j], acc);
        a[j][i] = acc;
      }
  }
}

template <int K>
__device__ __forceinline__ float portfolio_value(const float (&h)[K]) {  // ((h_0 + h_1) + h_2) + h_3
  float v = h[0];
#pragma unroll
  for (int i = 1; i < K; ++i) v = __fadd_rn(v, h[i]);
  return v;
}

template <int kMode, bool kExactDiv, bool kDense, int K>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void portfolio_kernel(const KernelArgs k, const PortfolioArgs p) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  if constexpr (is_table(kMode)) staged.table_len = k.table_len * portfolio_row_words(K);
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, walk_table_words<kMode>(staged), k.n_bins);
  uint32_t *lds_hist = s.counters;  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends (n_periods < 2^31)
    float a[kDraws][K];
    walk_blocks<kDraws>(
        k.n_periods,
        [&](uint32_t blk) { portfolio_multipliers<kMode, kDense, K>(k, p, dr, s.table, path_lo, path_hi, blk, a); },
        [&](int j, uint32_t t) {
#pragma unroll
          for (int x = 0; x < K; ++x) h[x] = compound<kExactDiv>(h[x], a[j][x]);
          if (--until == 0u) {  // uniform: t mod every == 0
            until = every;
            if (t != k.n_periods) {  // the final value and holdings are formed before any rebalance at P
              const float v = portfolio_value<K>(h);
#pragma unroll
              for (int x = 0; x < K; ++x) h[x] = __fmul_rn(v, p.weights[x]);
            }
          }
        });
    const float v = portfolio_value<K>(h);
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (p.d_holdings) {
#pragma unroll
        for (int x = 0; x < K; ++x) p.d_holdings[static_cast<uint64_t>(x) * k.n_paths + i] = h[x];
      }
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- portfolio cash flows: a schedule on a rebalanced portfolio ------------------------------------
//
// smmc_engine_simulate_portfolio_cashflow (csrc/smmc_portfolio_cashflow.cpp; include/smmc.h and DESIGN.md, "Portfolio
// cash flows", state the contract): portfolio_kernel's K holdings and joint draws with cashflow_kernel's step on their
// sum after every period's return, every operation a binary32 rounding of its own:
//   h_k = (h_k * a_k) / 100 for every asset;  g = ((h_0 + h_1) + h_2) + h_3
//   w = amount + g * fraction,  vn = g - w
//   live lane, vn > floor:     paid += w, v = vn, and h_k = vn * w_k at a rebalance, else h_k -= w * w_k
//   live lane, !(vn > floor):  depleted at this period: every h_k = 0, v = 0, paid += max(g, 0), ruin_period = t
//   depleted lane:             nothing changes; its draws are still made
// The rebalance stays the uniform branch behind portfolio_kernel's scalar countdown, "live" is cashflow_kernel's lane
// mask combined with the compare, control flow is wave-uniform.  A depleted lane's holdings are SET to 0 every period
// (the select that also applies the step), so a product 0 * inf cannot carry a NaN along.  Bound like its parents:
// VALU issue.  By source, on top of the K compounding chains: K - 1 adds (g), multiply, add, subtract, compare (w, vn,
// live), K multiplies and K subtracts (or K multiplies at a rebalance), K + 1 selects (h_k, v), max, select, add
// (paid), select (ruin_period): 4 K + 8.
//
// LDS: the asset table (or the v3 draw tables at scale 1) at address 0, then the [n_periods + 1] depletion counters,
// then the [n_bins] buckets.  Schedule: as cashflow_kernel -- kernel arguments when constant, else one block's entries
// through the constant address space, issued before the block's draws; no per-lane global load in the loop.
// One period of that recurrence for one strategy: the draw's K multipliers a, the strategy's weights, flow and floor,
// its state h, v, paid, ruin, `alive` (a lane mask) and `until`, the scalar countdown to its next rebalance (`every` = 0:
// the countdown never ends).  portfolio_cashflow_kernel makes one per draw, allocation_sweep_kernel one per draw and
// scenario.
template <bool kExactDiv, int K>
__device__ __forceinline__ void portfolio_cashflow_step(const float (&a)[K], const float (&weights)[SMMC_MAX_ASSETS], float amount,
                                                        float fraction, float floor, uint32_t every, uint32_t n_periods, uint32_t t,
                                                        float (&h)[K], float &v, float &paid, uint32_t &ruin, bool &alive,
                                                        uint32_t &until) {
#pragma unroll
  for (int y = 0; y < K; ++y) h[y] = compound<kExactDiv>(h[y], a[y]);
  const float g = portfolio_value<K>(h);
  const float w = __fadd_rn(amount, __fmul_rn(g, fraction));
  const float vn = __fsub_rn(g, w);
  const bool goes_on = alive && vn > floor;  // false for NaN
  const bool dies = alive && !goes_on;
  float hn[K];
  bool rebalance = false;
  if (--until == 0u) {  // uniform: t mod every == 0
    until = every;
    rebalance = t != n_periods;  // the final holdings are formed before any rebalance at P
  }
  if (rebalance) {
#pragma unroll
    for (int y = 0; y < K; ++y) hn[y] = __fmul_rn(vn, weights[y]);
  } else {  // the flow settles at the target weights
#pragma unroll
    for (int y = 0; y < K; ++y) hn[y] = __fsub_rn(h[y], __fmul_rn(w, weights[y]));
  }
#pragma unroll
  for (int y = 0; y < K; ++y) h[y] = goes_on ? hn[y] : 0.0f;
  v = goes_on ? vn : 0.0f;
  // a depleted lane: g = 0 (or NaN from 0 * inf: fmaxf gives 0), and paid + 0 is paid (paid is never -0)
  paid = __fadd_rn(paid, goes_on ? w : fmaxf(g, 0.0f));
  ruin = dies ? t : ruin;
  alive = goes_on;
}

template <int kMode, bool kExactDiv, bool kDense, int K, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void portfolio_cashflow_kernel(const KernelArgs k, const PortfolioCashflowArgs x) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  const CashflowArgs &c = x.c;
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  if constexpr (is_table(kMode)) staged.table_len = k.table_len * portfolio_row_words(K);
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, walk_table_words<kMode>(staged), k.n_periods + 1u + k.n_bins);
  uint32_t *lds_dep = s.counters;                     // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + (k.n_periods + 1u);  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    float v = 0.0f, paid = 0.0f;  // v: set by the first period (n_periods >= 1)
    uint32_t ruin = 0u;
    bool alive = true;
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends
    float a[kDraws][K];
    float am[kDraws], fr[kDraws];
    walk_blocks<kDraws>(
        k.n_periods,
        [&](uint32_t blk) {
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {  // the block's schedule entries (padded to whole blocks)
            am[j] = kVarying ? amounts[blk * kDraws + j] : c.amount;
            fr[j] = kVarying ? fractions[blk * kDraws + j] : c.fraction;
          }
          portfolio_multipliers<kMode, kDense, K>(k, p, dr, s.table, path_lo, path_hi, blk, a);
        },
        [&](int j, uint32_t t) {
          portfolio_cashflow_step<kExactDiv, K>(a[j], p.weights, am[j], fr[j], c.floor, every, k.n_periods, t, h, v, paid, ruin, alive,
                                                until);
        });
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, k.n_periods + 1u, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- block-bootstrap plans: portfolio cash flows on runs of consecutive months ---------------------
//
// smmc_engine_simulate_portfolio_cashflow_blocks (csrc/smmc_portfolio_cashflow_blocks.cpp; include/smmc.h and DESIGN.md,
// "Block-bootstrap plans", state the contract): portfolio_cashflow_kernel's recurrence -- the same
// portfolio_cashflow_step, called, not restated -- on rows drawn as blocks_kernel draws its entries.  Block b of a path
// starts at the row block_starts draws for it at period b (one Philox block per kDraws blocks, that is per kDraws L
// periods), and period t reads row (s_{(t-1) div L} + (t-1) mod L) mod n_rows.  Table mode only; a family of its own:
// portfolio_cashflow_kernel and blocks_kernel compile to what they compiled to before.
//
// Rows.  The asset table is staged with portfolio_cashflow_blocks_rows(n_rows) = n_rows + 7 rows, staged row i holding
// table row i mod n_rows, so that a run walks in segments of up to kBlockSeg = 8 periods from ONE per-lane byte address
// with the period in the instruction's offset field: one ds_read_b32 / b64 / b128 per period (K = 1, 2, 3 .. 4), no
// address arithmetic and no wrap test per period.  A segment that begins at row s < n_rows reads rows s .. s + 7 at the
// most, all below n_rows + 7.  Between segments the address advances by (8 mod n_rows) rows and wraps once (it stays below
// 2 n_rows rows), as block_run does.  The block's last 1 .. 7 periods and the last block, cut by P, read only the rows of
// their own periods (a uniform test per period of the tail).
//
// Control flow is wave-uniform: the period t, the block's and the segment's ends and the rebalance countdown are scalars,
// only the start row differs per lane.  The kDraws starts of a Philox block stay in registers; block b takes start
// b mod kDraws through a chain of selects on a scalar condition (no indexed register file access, no scratch), so the
// step is instantiated for the eight periods of a segment and the seven of a tail, not once more per draw.
//
// Schedule (kVarying): entry t - 1 is read for period t with the wave-uniform index through the constant address space,
// only for periods that exist (t <= P <= stride): a segment that begins off a multiple of 8 reads nothing past what
// cashflow_stage_schedule staged.
//
// LDS: [n_rows + 7 padded rows][n_periods + 1 depletion counters][n_bins buckets][pad][the waves' partials]
// (portfolio_cashflow_blocks_lds_bytes).
template <bool kExactDiv, bool kDense, int K, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(SMMC_MODE_TABLE))
void portfolio_cashflow_blocks_kernel(const KernelArgs k, const PortfolioCashflowBlocksArgs x) {
  constexpr int kMode = SMMC_MODE_TABLE;
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  constexpr uint32_t kRowWords = portfolio_row_words(K), kRowBytes = 4u * kRowWords;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  const CashflowArgs &c = x.c;
  const uint32_t n_rows = k.table_len;
  const uint32_t staged_words = portfolio_cashflow_blocks_rows(n_rows) * kRowWords;
  {  // the circular extension: staged rows n_rows .. n_rows + 6 (walk_setup stages the n_rows before them, and ends with the barrier)
    float *lds = reinterpret_cast<float *>(lds_raw);
    for (uint32_t i = n_rows * kRowWords + threadIdx.x; i < staged_words; i += kGroup)
      lds[i] = k.table_a[((i / kRowWords) % n_rows) * kRowWords + i % kRowWords];
  }
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  staged.table_len = n_rows * kRowWords;
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, staged_words, k.n_periods + 1u + k.n_bins);
  uint32_t *lds_dep = s.counters;                     // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + (k.n_periods + 1u);  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;
  const uint32_t P = k.n_periods, L = x.block_len;
  const uint32_t table_bytes = n_rows * kRowBytes;
  const uint32_t step_bytes = (static_cast<uint32_t>(kBlockSeg) % n_rows) * kRowBytes;  // what an address advances by between segments

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    float v = 0.0f, paid = 0.0f;  // v: set by the first period (n_periods >= 1)
    uint32_t ruin = 0u;
    bool alive = true;
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends
    uint32_t start[kDraws];
    uint32_t t = 0u;  // periods done; the block in hand covers periods t + 1 .. t + len
    // period t + j + 1 of the run in hand, on the row at `at` + j rows
    auto period = [&](uint32_t at, int j) {
      float a[K];
      load_asset_row_at<K>(at + static_cast<uint32_t>(j) * kRowBytes, a);
      const float am = kVarying ? amounts[t + j] : c.amount;
      const float fr = kVarying ? fractions[t + j] : c.fraction;
      portfolio_cashflow_step<kExactDiv, K>(a, p.weights, am, fr, c.floor, every, P, t + j + 1u, h, v, paid, ruin, alive, until);
    };
    for (uint32_t b = 0; t < P; ++b) {  // block b; everything but `at` is wave-uniform
      const uint32_t d = b % kDraws;
      if (d == 0u) block_starts<kDense>(k, dr, path_lo, path_hi, b / kDraws, start);
      uint32_t row = start[0];
#pragma unroll
      for (int j = 1; j < kDraws; ++j) row = d == static_cast<uint32_t>(j) ? start[j] : row;
      uint32_t at = row * kRowBytes;  // < table_bytes
      const uint32_t left = P - t;
      uint32_t rem = left < L ? left : L;  // the last block is cut by P
      for (; rem >= static_cast<uint32_t>(kBlockSeg); rem -= kBlockSeg) {
#pragma unroll
        for (int j = 0; j < kBlockSeg; ++j) period(at, j);
        t += kBlockSeg;
        at += step_bytes;  // < 2 table_bytes
        at = at >= table_bytes ? at - table_bytes : at;
      }
      if (rem) {  // the block's last 1 .. 7 periods
#pragma unroll
        for (int j = 0; j < kBlockSeg - 1; ++j)
          if (static_cast<uint32_t>(j) < rem) period(at, j);
        t += rem;
      }
    }
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, k.n_periods + 1u, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- stationary-bootstrap plans: portfolio cash flows on runs of geometric length -------------------
//
// smmc_engine_simulate_portfolio_cashflow_stationary (csrc/smmc_portfolio_cashflow_stationary.cpp; include/smmc.h and
// DESIGN.md, "Stationary-bootstrap plans", state the contract): portfolio_cashflow_kernel's recurrence -- the same
// portfolio_cashflow_step, called, not restated -- on rows chosen as stationary_kernel chooses its entries: the same
// stationary_index, renewal_field, kRenewTag and kRenewSeg, called, not restated.  Table mode only; a family of its own:
// portfolio_cashflow_kernel, portfolio_cashflow_blocks_kernel and stationary_kernel compile to what they compiled to before.
//
// Rows.  One plain copy of the asset table at LDS address 0, one row per month padded to 1, 2 or 4 words
// (load_asset_row): the wrap at n_rows is stationary_index's select, so nothing is staged beyond the last row.
//
// Segments.  A path is walked in segments of kRenewSeg = 8 periods.  stationary_rows takes the segment's eight
// candidates -- one block_starts<true> block for a dense table; blocks 2 g and 2 g + 1 for a four-draw one, the second
// only if the segment has more than four periods -- and one block of renewal fields, and forms the segment's row
// indices BEFORE the first step: candidates and fields are dead when the holdings' chains begin.  Then eight times
// load_asset_row and portfolio_cashflow_step; the path's last 1 .. 7 periods under a wave-uniform test per period.  A
// depleted lane keeps drawing and walking its index: nothing of a path depends on another path's state.
//
// Control flow is wave-uniform: the period, the segment's end and the rebalance countdown are scalars, the row is a
// per-lane select.  Both Philox counters are wave-uniform in word 0: philox4x32_10<kPhiloxUniformBlock> for both blocks.
//
// Schedule (kVarying): entry t - 1 is read for period t with the wave-uniform index through the constant address space,
// only for periods that exist (t <= P <= stride), as portfolio_cashflow_blocks_kernel does.
//
// LDS: [n_rows padded rows][n_periods + 1 depletion counters][n_bins buckets][pad][the waves' partials]
// (portfolio_cashflow_geometric_lds_bytes).
//
// The row indices of periods 8 g .. 8 g + n - 1 (0-based) of a path, n = 8 (kFull) or the path's last 1 .. 7
// (wave-uniform); idx: the index of the period before, left at that of the segment's last period.
// The gathering of candidates and fields repeats stationary_segment's (stationary bootstrap, above) line for line, so
// that stationary_kernel keeps its instructions: the two copies must change together.
template <bool kDense, bool kFull>
__device__ __forceinline__ void stationary_rows(const KernelArgs &k, uint32_t q, const DrawRegs &dr, uint32_t path_lo, uint32_t path_hi,
                                                uint32_t g, uint32_t n, uint32_t &idx, uint32_t (&row)[kRenewSeg]) {
  uint32_t c[kRenewSeg];
  if constexpr (kDense) {
    block_starts<true>(k, dr, path_lo, path_hi, g, c);
  } else {  // four candidates per block of the table stream: blocks 2 g and 2 g + 1 (g < 2^29)
    uint32_t lo[4], hi[4] = {0u, 0u, 0u, 0u};
    block_starts<false>(k, dr, path_lo, path_hi, 2u * g, lo);
    if (kFull || n > 4u) block_starts<false>(k, dr, path_lo, path_hi, 2u * g + 1u, hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = lo[j];
      c[4 + j] = hi[j];
    }
  }
  uint32_t f[4];
  philox4x32_10<kPhiloxUniformBlock>(g, path_lo, path_hi, kRenewTag, k.key0, k.key1, dr, f);
#pragma unroll
  for (int j = 0; j < kRenewSeg; ++j) {
    if (kFull || static_cast<uint32_t>(j) < n) {  // row[j] of a period that does not exist is left unset and never read
      idx = stationary_index(idx, c[j], renewal_field(f, j), q, k.table_len, j == 0 && g == 0u);
      row[j] = idx;
    }
  }
}

template <bool kExactDiv, bool kDense, int K, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(SMMC_MODE_TABLE))
void portfolio_cashflow_stationary_kernel(const KernelArgs k, const PortfolioCashflowStationaryArgs x) {
  constexpr int kMode = SMMC_MODE_TABLE;
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  const CashflowArgs &c = x.c;
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  staged.table_len = k.table_len * portfolio_row_words(K);
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, staged.table_len, k.n_periods + 1u + k.n_bins);
  uint32_t *lds_dep = s.counters;                     // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + (k.n_periods + 1u);  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;
  const uint32_t P = k.n_periods, q = x.renew_q16;
  const uint32_t full = P / kRenewSeg, rem = P - full * kRenewSeg;

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    float v = 0.0f, paid = 0.0f;  // v: set by the first period (n_periods >= 1)
    uint32_t ruin = 0u;
    bool alive = true;
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends
    uint32_t idx = 0u;       // the row of the period before; period 0 takes its candidate
    uint32_t row[kRenewSeg];
    // period t0 + j + 1 (1-based) on row[j]
    auto period = [&](uint32_t t0, int j) {
      float a[K];
      load_asset_row<K>(row[j], a);
      const float am = kVarying ? amounts[t0 + j] : c.amount;
      const float fr = kVarying ? fractions[t0 + j] : c.fraction;
      portfolio_cashflow_step<kExactDiv, K>(a, p.weights, am, fr, c.floor, every, P, t0 + j + 1u, h, v, paid, ruin, alive, until);
    };
    for (uint32_t g = 0; g < full; ++g) {
      stationary_rows<kDense, true>(k, q, dr, path_lo, path_hi, g, kRenewSeg, idx, row);
#pragma unroll
      for (int j = 0; j < kRenewSeg; ++j) period(g * kRenewSeg, j);
    }
    if (rem) {  // wave-uniform: the path's last 1 .. 7 periods
      stationary_rows<kDense, false>(k, q, dr, path_lo, path_hi, full, rem, idx, row);
#pragma unroll
      for (int j = 0; j < kRenewSeg - 1; ++j)
        if (static_cast<uint32_t>(j) < rem) period(full * kRenewSeg, j);
    }
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, k.n_periods + 1u, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- regime-switching plans: portfolio cash flows under a two-state law ------------------------------
//
// smmc_engine_simulate_portfolio_cashflow_regimes (csrc/smmc_portfolio_cashflow_regimes.cpp; include/smmc.h and
// DESIGN.md, "Regime-switching plans", state the contract): portfolio_cashflow_kernel's Gaussian path -- the same K
// chains of standard normals, the same portfolio_cashflow_step, called, not restated -- with the multipliers of the regime
// the path is in this period, and regimes_kernel's state: the same fields (kRegimeTag, kRegimeSeg, renewal_field), the
// same update.  Gaussian mode only; a family of its own: portfolio_cashflow_kernel and regimes_kernel compile to what
// they compiled to before.
//
// Fields.  One block of fields serves kRegimeSeg = 8 periods, two draw blocks: walk_blocks' block index is wave-uniform,
// so "even block" is a scalar test.  markov_states draws the field block there and forms all eight states at once -- also
// those of periods past the last, which nothing reads --, so the four field words are dead before the K normal chains
// start; the states live on as lane masks, the second draw block of the segment moves its four to the front.
//
// Multipliers.  Per period and asset, s_k and the row of L are selects of kernel arguments on the lane's state, then the
// parent's chain of fused multiply-adds: K + K (K + 1) / 2 selects per period on top of the parent's.  Forming both
// regimes' multipliers and selecting K of them would double the half-rate FMAs for the full-rate selects saved.
//
// Control flow is wave-uniform: the state is data, the rebalance the scalar countdown.  LDS: the parent's Gaussian
// layout (portfolio_cashflow_markov_lds_bytes).
//
// The states of periods 8 g .. 8 g + 7 of a path; `state`: that of the period before, left at that of the segment's last.
__device__ __forceinline__ void markov_states(const KernelArgs &k, const PortfolioCashflowMarkovArgs &x, const DrawRegs &dr,
                                              uint32_t path_lo, uint32_t path_hi, uint32_t g, bool &state, bool (&s)[kRegimeSeg]) {
  uint32_t f[4];
  philox4x32_10<kPhiloxUniformBlock>(g, path_lo, path_hi, kRegimeTag, k.key0, k.key1, dr, f);
  // period 0 comes from "regime 0" (the state's initial value) with start1_q16 in leave_q16[0]'s place: a scalar select
  const uint32_t q0 = g == 0u ? x.start1_q16 : x.leave_q16[0];
#pragma unroll
  for (int j = 0; j < kRegimeSeg; ++j) {
    const uint32_t q = state ? x.leave_q16[1] : (j == 0 ? q0 : x.leave_q16[0]);
    state = state != (renewal_field(f, j) < q);
    s[j] = state;
  }
}

// The multipliers a[j][i] of asset i at draw j of Philox block `blk` (wave-uniform) of a path whose state at draw j is s[j]:
// portfolio_multipliers' normals, the chain over the row of the state's factor from the state's shift.
template <int K>
__device__ __forceinline__ void markov_multipliers(const KernelArgs &k, const PortfolioCashflowMarkovArgs &x, const DrawRegs &dr,
                                                   const float *lds_table, uint32_t path_lo, uint32_t path_hi, uint32_t blk,
                                                   const bool (&s)[kRegimeSeg], float (&a)[4][K]) {
  uint32_t u[K][4];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    u[i][0] = blk;
    u[i][1] = path_lo;
    u[i][2] = path_hi;
    u[i][3] = 1u + 2u * static_cast<uint32_t>(i);
  }
  philox4x32_10_multi<K, true>(u, k.key0, k.key1, dr);
  float z[K][4];  // standard normals: the tables are staged at scale 1, dr.shift100 is 0
  multipliers_of_words_multi<SMMC_MODE_GAUSSIAN, false, K>(k, dr, lds_table, u, z);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float acc = s[j] ? x.shift100[1][i] : x.shift100[0][i];
#pragma unroll
      for (int m = 0; m <= i; ++m) {
        const float l = s[j] ? x.factor[1][i * SMMC_MAX_ASSETS + m] : x.factor[0][i * SMMC_MAX_ASSETS + m];
        acc = __builtin_fmaf(l, z[m][j], acc);
      }
      a[j][i] = acc;
    }
}

// No amdgpu_waves_per_eu: nothing measured asks for one.
template <bool kExactDiv, int K, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(SMMC_MODE_GAUSSIAN))
void portfolio_cashflow_regimes_kernel(const KernelArgs k, const PortfolioCashflowMarkovArgs x) {
  constexpr int kMode = SMMC_MODE_GAUSSIAN;
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = 4;
  static_assert(kRegimeSeg == 2 * kDraws, "a block of fields serves two blocks of normals");
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  const CashflowArgs &c = x.c;
  const WalkLds s = walk_setup<kMode>(k, lds_raw, walk_table_words<kMode>(k), k.n_periods + 1u + k.n_bins);
  uint32_t *lds_dep = s.counters;                     // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + (k.n_periods + 1u);  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    float v = 0.0f, paid = 0.0f;  // v: set by the first period (n_periods >= 1)
    uint32_t ruin = 0u;
    bool alive = true;
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends
    bool state = false;      // the regime of the period before; period 0 takes start1_q16
    bool st[kRegimeSeg];     // the states of this draw block's periods in st[0 .. 3]
    float a[kDraws][K];
    float am[kDraws], fr[kDraws];
    walk_blocks<kDraws>(
        k.n_periods,
        [&](uint32_t blk) {
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {  // the block's schedule entries (padded to whole blocks)
            am[j] = kVarying ? amounts[blk * kDraws + j] : c.amount;
            fr[j] = kVarying ? fractions[blk * kDraws + j] : c.fraction;
          }
          if ((blk & 1u) == 0u) {  // wave-uniform: the segment's first draw block
            markov_states(k, x, dr, path_lo, path_hi, blk >> 1, state, st);
          } else {
#pragma unroll
            for (int j = 0; j < kDraws; ++j) st[j] = st[kDraws + j];
          }
          markov_multipliers<K>(k, x, dr, s.table, path_lo, path_hi, blk, st, a);
        },
        [&](int j, uint32_t t) {
          portfolio_cashflow_step<kExactDiv, K>(a[j], p.weights, am[j], fr[j], c.floor, every, k.n_periods, t, h, v, paid, ruin, alive,
                                                until);
        });
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, k.n_periods + 1u, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- portfolio cash-flow checkpoints: the plan's value distribution at chosen periods ---------------
//
// smmc_engine_simulate_portfolio_cashflow_checkpoints (csrc/smmc_portfolio_cashflow_checkpoints.cpp; include/smmc.h and
// DESIGN.md, "Portfolio cash-flow checkpoints", state the contract): portfolio_cashflow_kernel's path -- the same draws,
// the same portfolio_cashflow_step, called, not restated -- with checkpoints_kernel's records of `v` after chosen
// periods.  A family of its own: portfolio_cashflow_kernel compiles to what it compiled to before.
//
// Where the checkpoint test sits.  The sorted periods are kernel arguments read with scalar loads, `next_p`, the next
// one, lives in an SGPR, and the period index t is wave-uniform, so the test is ONE scalar compare and branch per
// period behind the step (checkpoints_kernel tests once per Philox block and pays with a second copy of the block that
// keeps the prefix values; here v is in its register after every step anyway, and a second copy of the unrolled steps
// would double the loop's code).  A period that is no checkpoint runs the parent's vector instructions and no other.
// A record (checkpoint_record) is taken for every lane of the chunk with `active` as its mask; a depleted lane
// contributes its 0.
//
// What persists over a wave's trips: lane k's CheckpointAcc, the LaneRecord of the final values, the LDS counters.
// Per path: `until`, `ck` and `next_p` start again, and the schedule is read from its first entry (blk = 0).
//
// LDS, stated once more on the host side (portfolio_cashflow_checkpoints_lds_bytes):
//   [front: the asset table or the v3 draw tables at address 0; after the walk and a barrier the waves' checkpoint
//           partials [kW][x.n] -- checkpoint_front_words() reserves the larger of the two]
//   [n_periods + 1 depletion counters][n_bins final buckets][x.n][n_bins] checkpoint buckets]   (u32, zeroed by walk_setup)
//   [pad to 8 bytes][kW BlockPartial: the waves' LaneRecord partials]
template <int kMode, bool kExactDiv, bool kDense, int K, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void portfolio_cashflow_checkpoints_kernel(const KernelArgs k, const PortfolioCashflowCheckpointsArgs x) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  const CashflowArgs &c = x.c;
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  if constexpr (is_table(kMode)) staged.table_len = k.table_len * portfolio_row_words(K);
  const uint32_t n_at = k.n_periods + 1u, ck_words = x.n * k.n_bins;
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, checkpoint_front_words(walk_table_words<kMode>(staged), kW, x.n),
                                      n_at + k.n_bins + ck_words);
  uint32_t *lds_dep = s.counters;          // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + n_at;     // [n_bins]
  uint32_t *lds_ck = lds_hist + k.n_bins;  // [x.n][n_bins]
  const uint32_t lane = s.lane, wave = s.wave;

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  CheckpointAcc acc;
  acc.sum = acc.sumsq = 0.0;
  acc.count = acc.below = acc.under = acc.over = 0u;
  acc.min = __builtin_inff();
  acc.max = -__builtin_inff();
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    float v = 0.0f, paid = 0.0f;  // v: set by the first period (n_periods >= 1)
    uint32_t ruin = 0u;
    bool alive = true;
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends
    uint32_t ck = 0u, next_p = x.periods[0];  // uniform: the next checkpoint and its period
    float a[kDraws][K];
    float am[kDraws], fr[kDraws];
    walk_blocks<kDraws>(
        k.n_periods,
        [&](uint32_t blk) {
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {  // the block's schedule entries (padded to whole blocks)
            am[j] = kVarying ? amounts[blk * kDraws + j] : c.amount;
            fr[j] = kVarying ? fractions[blk * kDraws + j] : c.fraction;
          }
          portfolio_multipliers<kMode, kDense, K>(k, p, dr, s.table, path_lo, path_hi, blk, a);
        },
        [&](int j, uint32_t t) {
          portfolio_cashflow_step<kExactDiv, K>(a[j], p.weights, am[j], fr[j], c.floor, every, k.n_periods, t, h, v, paid, ruin, alive,
                                                until);
          if (t == next_p) {  // uniform; ck < x.n here: next_p is 0xffffffff once none is left
            checkpoint_record(k, ck, v, active, lane, lds_ck, acc);
            ++ck;
            next_p = ck < x.n ? x.periods[ck] : 0xffffffffu;
          }
        });
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // every wave is through with the draw tables; the waves' partials are written, their LDS adds complete
  BlockPartial *part = reinterpret_cast<BlockPartial *>(lds_raw);  // [kW][x.n], over the tables
  if (lane < x.n) {
    BlockPartial q;
    q.sum = acc.sum;
    q.sumsq = acc.sumsq;
    q.count = acc.count;
    q.below = acc.below;
    q.underflow = acc.under;
    q.overflow = acc.over;
    q.min = acc.min;
    q.max = acc.max;
    part[wave * x.n + lane] = q;
  }
  __syncthreads();
  if (threadIdx.x < x.n) {  // thread k: checkpoint k's partials in wave order
    BlockPartial t = part[threadIdx.x];
    for (uint32_t w = 1; w < kW; ++w) partial_add(t, part[w * x.n + threadIdx.x]);
    x.ck_partials[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = t;
  }
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, n_at, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
  if (ck_words) flush_counters<kGroup>(lds_ck, ck_words, x.d_ck_hist);
}

// ---- real cash flows: the schedule in money of period 0, indexed by a jointly drawn inflation series ----
//
// smmc_engine_simulate_real_cashflow (csrc/smmc_real_cashflow.cpp; include/smmc.h and DESIGN.md, "Real cash flows",
// state the contract): portfolio_cashflow_kernel's K holdings and step on a joint law of K + 1 series.  Series K is
// inflation in percent per period: it compounds a price index I from 1.0f as a holding compounds, on every lane,
// depleted or not, and the period's nominal amount and floor are fl(amount * I) and fl(floor * I) with the index AFTER
// that period's inflation:
//   h_k = (h_k * a_k) / 100 for k < K;  I = (I * a_K) / 100;  g = (h_0 + h_1) + h_2
//   w = amount * I + g * fraction,  vn = g - w,  live while vn > floor * I;  the two branches are the parent's
// The draw is portfolio_multipliers<kMode, kDense, K + 1>: table rows are K + 1 wide in LDS (one ds_read_b64 / b128 per
// period), a Gaussian period takes K + 1 Philox chains.  The step is a sibling of portfolio_cashflow_step, not a
// parameter of it: the parent's and the sweep's instruction sequences stay what they are.  After the loop
// final_real = v / I is ONE IEEE division (__fdiv_rn, whatever kExactDiv says) and feeds the record.  By source, on top
// of the parent's step of the same K: the index chain (multiply and the divide), one multiply for the amount and one
// for the floor.  LDS layout, schedule loads and epilogue are the parent's.
template <bool kExactDiv, int K>
__device__ __forceinline__ void real_cashflow_step(const float (&a)[K + 1], const float (&weights)[SMMC_MAX_ASSETS], float amount,
                                                   float fraction, float floor, uint32_t every, uint32_t n_periods, uint32_t t,
                                                   float (&h)[K], float &index, float &v, float &paid, uint32_t &ruin, bool &alive,
                                                   uint32_t &until) {
#pragma unroll
  for (int y = 0; y < K; ++y) h[y] = compound<kExactDiv>(h[y], a[y]);
  index = compound<kExactDiv>(index, a[K]);
  const float g = portfolio_value<K>(h);
  const float w = __fadd_rn(__fmul_rn(amount, index), __fmul_rn(g, fraction));
  const float vn = __fsub_rn(g, w);
  const bool goes_on = alive && vn > __fmul_rn(floor, index);  // false for NaN
  const bool dies = alive && !goes_on;
  float hn[K];
  bool rebalance = false;
  if (--until == 0u) {  // uniform: t mod every == 0
    until = every;
    rebalance = t != n_periods;  // the final holdings are formed before any rebalance at P
  }
  if (rebalance) {
#pragma unroll
    for (int y = 0; y < K; ++y) hn[y] = __fmul_rn(vn, weights[y]);
  } else {  // the flow settles at the target weights
#pragma unroll
    for (int y = 0; y < K; ++y) hn[y] = __fsub_rn(h[y], __fmul_rn(w, weights[y]));
  }
#pragma unroll
  for (int y = 0; y < K; ++y) h[y] = goes_on ? hn[y] : 0.0f;
  v = goes_on ? vn : 0.0f;
  // a depleted lane: g = 0 (or NaN from 0 * inf: fmaxf gives 0), and paid + 0 is paid (paid is never -0)
  paid = __fadd_rn(paid, goes_on ? w : fmaxf(g, 0.0f));
  ruin = dies ? t : ruin;
  alive = goes_on;
}

template <int kMode, bool kExactDiv, bool kDense, int K, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void real_cashflow_kernel(const KernelArgs k, const RealCashflowArgs x) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  static_assert(K >= 1 && K + 1 <= SMMC_MAX_ASSETS, "K invested assets and the inflation series");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;  // the law of K + 1 series; weights[K] is 0 and never read
  const CashflowArgs &c = x.c;
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  if constexpr (is_table(kMode)) staged.table_len = k.table_len * portfolio_row_words(K + 1);
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, walk_table_words<kMode>(staged), k.n_periods + 1u + k.n_bins);
  uint32_t *lds_dep = s.counters;                     // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + (k.n_periods + 1u);  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    float index = 1.0f;
    float v = 0.0f, paid = 0.0f;  // v: set by the first period (n_periods >= 1)
    uint32_t ruin = 0u;
    bool alive = true;
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends
    float a[kDraws][K + 1];
    float am[kDraws], fr[kDraws];
    walk_blocks<kDraws>(
        k.n_periods,
        [&](uint32_t blk) {
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {  // the block's schedule entries (padded to whole blocks)
            am[j] = kVarying ? amounts[blk * kDraws + j] : c.amount;
            fr[j] = kVarying ? fractions[blk * kDraws + j] : c.fraction;
          }
          portfolio_multipliers<kMode, kDense, K + 1>(k, p, dr, s.table, path_lo, path_hi, blk, a);
        },
        [&](int j, uint32_t t) {
          real_cashflow_step<kExactDiv, K>(a[j], p.weights, am[j], fr[j], c.floor, every, k.n_periods, t, h, index, v, paid, ruin,
                                           alive, until);
        });
    const float v_real = __fdiv_rn(v, index);
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (x.d_final_real) x.d_final_real[i] = v_real;
      if (x.d_index) x.d_index[i] = index;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v_real, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, k.n_periods + 1u, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- guardrails: a withdrawal that a review rule adjusts per path -----------------------------------
//
// smmc_engine_simulate_guardrails (csrc/smmc_guardrails.cpp; include/smmc.h and DESIGN.md, "Guardrails", state the
// contract): portfolio_cashflow_kernel's holdings, draws and depletion with the amount in force `cur` as per-lane state.
// Every period takes w = cur (no fraction); after every E-th period a live lane that goes on reviews it:
//   c = cur * index;  c > vn * upper: c *= cut, a cut;  else c < vn * lower: c *= raise, a raise
//   cur = min(max(c, amount_min), amount_max);  lowest = min(lowest, cur)
// The amount differs per path, which is the case the parent's divide proof sends to the IEEE divide: the chains are
// compound<true> always, there is no fast form.  The step is a SIBLING of portfolio_cashflow_step: the parent's, the
// checkpoint kernel's and the sweep's instruction sequences stay what they are.  The review sits behind a second scalar
// countdown beside the rebalance countdown (`until_review`; E = 0: it never ends), a wave-uniform branch: a period
// without a review is the parent's step less the two instructions of w = amount + g * fraction.  By source, on top of
// the K compounding chains: 4 K + 6 VALU in an ordinary period; a review adds 16 (three multiplies and two compares of
// the bands, two selects of the factor and its multiply, max, min, select (cur), min (lowest), two selects and two adds
// of the per-path counts); the per-period counts are two ballots and population counts on the scalar unit and one LDS
// add each from lane 0.  `counts`: the lane's path is below n_paths (a lane beyond it runs a path and counts nothing).
struct GuardrailsLane {  // a lane's state beside the holdings
  float v, paid, cur, lowest;
  uint32_t ruin, cuts, raises;
  bool alive;
};
template <int K>
__device__ __forceinline__ void guardrails_step(const float (&a)[K], const GuardrailsArgs &x, uint32_t n_periods, uint32_t t, bool counts,
                                                uint32_t lane, uint32_t *lds_cuts, uint32_t *lds_raises, float (&h)[K],
                                                GuardrailsLane &s, uint32_t &until, uint32_t &until_review) {
  const float (&weights)[SMMC_MAX_ASSETS] = x.p.weights;
#pragma unroll
  for (int y = 0; y < K; ++y) h[y] = compound<true>(h[y], a[y]);
  const float g = portfolio_value<K>(h);
  const float w = s.cur;
  const float vn = __fsub_rn(g, w);
  const bool goes_on = s.alive && vn > x.floor;  // false for NaN
  const bool dies = s.alive && !goes_on;
  float hn[K];
  bool rebalance = false;
  if (--until == 0u) {  // uniform: t mod R == 0
    until = x.p.rebalance_every;
    rebalance = t != n_periods;  // the final holdings are formed before any rebalance at P
  }
  if (rebalance) {
#pragma unroll
    for (int y = 0; y < K; ++y) hn[y] = __fmul_rn(vn, weights[y]);
  } else {  // the flow settles at the target weights
#pragma unroll
    for (int y = 0; y < K; ++y) hn[y] = __fsub_rn(h[y], __fmul_rn(w, weights[y]));
  }
#pragma unroll
  for (int y = 0; y < K; ++y) h[y] = goes_on ? hn[y] : 0.0f;
  s.v = goes_on ? vn : 0.0f;
  // a depleted lane: g = 0 (or NaN from 0 * inf: fmaxf gives 0), and paid + 0 is paid (paid is never -0)
  s.paid = __fadd_rn(s.paid, goes_on ? w : fmaxf(g, 0.0f));
  s.ruin = dies ? t : s.ruin;
  s.alive = goes_on;
  if (--until_review == 0u) {  // uniform: t mod E == 0
    until_review = x.review_every;
    if (t != n_periods) {  // no review after the last period: nothing would be taken at the new amount
      float c = __fmul_rn(s.cur, x.index);
      const bool cut = goes_on && c > __fmul_rn(vn, x.upper);            // false for NaN
      const bool raise = goes_on && !cut && c < __fmul_rn(vn, x.lower);  // false for NaN
      c = __fmul_rn(c, cut ? x.cut : raise ? x.raise : 1.0f);            // c * 1.0f is c
      c = fminf(fmaxf(c, x.amount_min), x.amount_max);
      s.cur = goes_on ? c : s.cur;
      s.lowest = fminf(s.lowest, s.cur);
      s.cuts += cut ? 1u : 0u;
      s.raises += raise ? 1u : 0u;
      const uint32_t n_cut = ballot_count(cut && counts), n_raise = ballot_count(raise && counts);  // wave-uniform
      if (lds_cuts && n_cut && lane == 0u) atomicAdd(&lds_cuts[t], n_cut);
      if (lds_raises && n_raise && lane == 0u) atomicAdd(&lds_raises[t], n_raise);
    }
  }
}

template <int kMode, bool kDense, int K>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void guardrails_kernel(const KernelArgs k, const GuardrailsArgs x) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  if constexpr (is_table(kMode)) staged.table_len = k.table_len * portfolio_row_words(K);
  const uint32_t n_at = k.n_periods + 1u;
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, walk_table_words<kMode>(staged), 3u * n_at + k.n_bins);
  uint32_t *lds_dep = s.counters;          // [n_periods + 1]
  uint32_t *lds_cuts = lds_dep + n_at;     // [n_periods + 1], [0] stays 0
  uint32_t *lds_raises = lds_cuts + n_at;  // [n_periods + 1], [0] stays 0
  uint32_t *lds_hist = lds_raises + n_at;  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = x.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    GuardrailsLane st;
    st.v = 0.0f;  // set by the first period (n_periods >= 1)
    st.paid = 0.0f;
    st.cur = st.lowest = x.amount;
    st.ruin = st.cuts = st.raises = 0u;
    st.alive = true;
    uint32_t until = p.rebalance_every;  // periods until the next rebalance; with R == 0 the countdown never ends
    uint32_t until_review = x.review_every;  // and until the next review, likewise
    float a[kDraws][K];
    walk_blocks<kDraws>(
        k.n_periods, [&](uint32_t blk) { portfolio_multipliers<kMode, kDense, K>(k, p, dr, s.table, path_lo, path_hi, blk, a); },
        [&](int j, uint32_t t) {
          guardrails_step<K>(a[j], x, k.n_periods, t, active, s.lane, x.d_cuts_at ? lds_cuts : nullptr,
                             x.d_raises_at ? lds_raises : nullptr, h, st, until, until_review);
        });
    if (active) {
      if (k.d_final) k.d_final[i] = st.v;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (x.d_paid) x.d_paid[i] = st.paid;
      if (x.d_ruin_period) x.d_ruin_period[i] = st.ruin;
      if (x.d_amount_last) x.d_amount_last[i] = st.cur;
      if (x.d_amount_lowest) x.d_amount_lowest[i] = st.lowest;
      if (x.d_cuts) x.d_cuts[i] = st.cuts;
      if (x.d_raises) x.d_raises[i] = st.raises;
      if (want_dep) atomicAdd(&lds_dep[st.ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, st.v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, n_at, x.d_depleted);
  if (x.d_cuts_at) flush_counters<kGroup>(lds_cuts, n_at, x.d_cuts_at);
  if (x.d_raises_at) flush_counters<kGroup>(lds_raises, n_at, x.d_raises_at);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- glide paths: target weights that change along a plan -------------------------------------------
//
// smmc_engine_simulate_glide (csrc/smmc_glide.cpp; include/smmc.h and DESIGN.md, "Glide paths", state the contract):
// portfolio_cashflow_kernel's path -- the same draws, the same portfolio_cashflow_step, called, not restated -- with the
// weights the step trades at held in an array of the kernel's own, `w`, instead of the kernel argument.  A family of
// its own: portfolio_cashflow_kernel compiles to what it compiled to before.
//
// The changes lie flattened in x.table (GlideEntry, smmc_internal.h), in the order they take effect.  A third scalar
// countdown beside the rebalance countdown, `left`, starts at x.first = after[0] (0: it never ends) and is decremented
// before the step of every period; when it hits 0 the next entry is read through the constant address space -- one
// scalar load of 32 bytes at a uniform address --, its weights go into `w` and its `next` into the countdown.  The
// branch is wave-uniform (everything it depends on is a kernel argument or came through a scalar load), the weights
// stay in scalar registers, and there is no per-lane global load and no LDS traffic for it: a period without a change is
// the parent's step and a scalar decrement and compare.  Per chunk of the wave walk the weights go back to p.weights,
// the countdown to x.first and the entry index to 0: a wave's second chunk starts from stage 0 again.
typedef const __attribute__((address_space(4))) GlideEntry *const_glide_ptr;  // scalar (uniform) loads

template <int kMode, bool kExactDiv, bool kDense, int K, bool kVarying>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void glide_kernel(const KernelArgs k, const GlideArgs x) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  static_assert(K >= 2, "one asset has one legal weight vector: the host launches portfolio_cashflow_kernel");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  const CashflowArgs &c = x.c;
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  if constexpr (is_table(kMode)) staged.table_len = k.table_len * portfolio_row_words(K);
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, walk_table_words<kMode>(staged), k.n_periods + 1u + k.n_bins);
  uint32_t *lds_dep = s.counters;                     // [n_periods + 1]
  uint32_t *lds_hist = lds_dep + (k.n_periods + 1u);  // [n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = c.d_depleted != nullptr;
  LaneRecord rec;
  const DrawRegs dr = make_draw_regs(k);
  const uint32_t every = p.rebalance_every;
  const const_float_ptr amounts = (const_float_ptr)(c.schedule);
  const const_float_ptr fractions = amounts + c.stride;
  const const_glide_ptr changes = (const_glide_ptr)(x.table);

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[K];
#pragma unroll
    for (int a = 0; a < K; ++a) h[a] = __fmul_rn(k.initial_capital, p.weights[a]);
    float v = 0.0f, paid = 0.0f;  // v: set by the first period (n_periods >= 1)
    uint32_t ruin = 0u;
    bool alive = true;
    uint32_t until = every;  // periods until the next rebalance; with every == 0 the countdown never ends
    // the chunk starts from stage 0: the weights of the request, the countdown to the first change, the first entry
    float w[SMMC_MAX_ASSETS];
#pragma unroll
    for (int y = 0; y < SMMC_MAX_ASSETS; ++y) w[y] = p.weights[y];
    uint32_t left = x.first;  // periods until the next change; with first == 0 the countdown never ends
    uint32_t stage = 0u;      // the entry the next change reads
    float a[kDraws][K];
    float am[kDraws], fr[kDraws];
    walk_blocks<kDraws>(
        k.n_periods,
        [&](uint32_t blk) {
#pragma unroll
          for (int j = 0; j < kDraws; ++j) {  // the block's schedule entries (padded to whole blocks)
            am[j] = kVarying ? amounts[blk * kDraws + j] : c.amount;
            fr[j] = kVarying ? fractions[blk * kDraws + j] : c.fraction;
          }
          portfolio_multipliers<kMode, kDense, K>(k, p, dr, s.table, path_lo, path_hi, blk, a);
        },
        [&](int j, uint32_t t) {
          if (--left == 0u) {  // uniform: a change takes effect with the trade at the end of this period
#pragma unroll
            for (int y = 0; y < K; ++y) w[y] = changes[stage].weights[y];
            left = changes[stage].next;
            ++stage;
          }
          portfolio_cashflow_step<kExactDiv, K>(a[j], w, am[j], fr[j], c.floor, every, k.n_periods, t, h, v, paid, ruin, alive, until);
        });
    if (active) {
      if (k.d_final) k.d_final[i] = v;
      if (p.d_holdings) {
#pragma unroll
        for (int y = 0; y < K; ++y) p.d_holdings[static_cast<uint64_t>(y) * k.n_paths + i] = h[y];
      }
      if (c.d_paid) c.d_paid[i] = paid;
      if (c.d_ruin_period) c.d_ruin_period[i] = ruin;
      if (want_dep) atomicAdd(&lds_dep[ruin], 1u);  // ruin <= n_periods
    }
    if (want_stats && active) rec.add(k, v, want_hist, lds_hist);
  });

  if (want_stats) rec.store(s);
  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x == 0) fold_wave_partials<kW>(s.wave_part, &k.partials[blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, k.n_periods + 1u, c.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, k.n_bins, k.d_hist);
}

// ---- allocation sweeps: up to eight portfolio strategies on one set of draws ------------------------
//
// smmc_engine_simulate_allocation_sweep (csrc/smmc_allocation_sweep.cpp; include/smmc.h and DESIGN.md, "Allocation
// sweeps", state the contract): scenario sc of a sweep is portfolio_cashflow_kernel<..., kVarying = false> with
// (weights, rebalance_every, amount, fraction, floor)[sc] on the law of x.p.  The joint draw of a period depends on (seed,
// path id, period, law) alone, so ONE portfolio_multipliers per Philox block serves all scenarios; per draw an unrolled
// loop makes the kS portfolio_cashflow_steps, each on its own h[K], v, paid, ruin, `alive` (a lane mask in a scalar
// register pair) and its own scalar rebalance countdown -- the scenarios may differ in R, every countdown is
// wave-uniform, and so is all control flow.  The (K + 4) kS parameters are kernel arguments; the loop loads nothing
// beyond the draw's gathers.  By source a scenario and period cost the parent's step: K compounding chains and 4 K + 8.
//
// kS is 4 or 8: the host pads a request to the next of them with copies of its last scenario, and x.n says how many are
// real -- a padded scenario is stepped and nothing of it is ever stored, counted or recorded, as in
// cashflow_sweep_kernel.  Records, LDS and epilogue are that kernel's too: wave_record_add into per-wave, per-scenario
// partials, [asset table or v3 draw tables][x.n][n_periods + 1] depletion][x.n][n_bins] buckets][pad][kS][kW] partials],
// thread sc folds scenario sc's partials into k.partials[sc][workgroup], flush_counters takes both counter arrays.
template <int kMode, bool kExactDiv, bool kDense, int K, int kS>
__global__ __launch_bounds__(64 * walk_waves(kMode))
void allocation_sweep_kernel(const KernelArgs k, const AllocationSweepArgs x) {
  static_assert(counter_v3(kMode), "counter stream v3 only");
  static_assert(kS == 4 || kS == 8, "two widths");
  constexpr uint32_t kW = walk_waves(kMode);
  constexpr uint32_t kGroup = 64u * kW;
  constexpr int kDraws = Draws<kMode, kDense>::value;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const PortfolioArgs &p = x.p;
  KernelArgs staged = k;  // what walk_setup stages: whole rows (k.table_len stays the number of rows, for the draw)
  if constexpr (is_table(kMode)) staged.table_len = k.table_len * portfolio_row_words(K);
  const uint32_t n_at = k.n_periods + 1u;
  const WalkLds s = walk_setup<kMode>(staged, lds_raw, walk_table_words<kMode>(staged), x.n * (n_at + k.n_bins));  // wave_part: [kS][kW]
  uint32_t *lds_dep = s.counters;             // [x.n][n_periods + 1]
  uint32_t *lds_hist = lds_dep + x.n * n_at;  // [x.n][n_bins]

  const bool want_stats = k.partials != nullptr;  // all uniform
  const bool want_hist = want_stats && k.n_bins != 0;
  const bool want_dep = x.d_depleted != nullptr;
  const uint32_t lane = s.lane;
  BlockPartial *part = s.wave_part + s.wave;  // scenario sc: part[sc * kW], this wave's own until the barrier
  if (lane == 0) {
#pragma unroll
    for (int sc = 0; sc < kS; ++sc) partial_identity(part[sc * kW]);
  }
  const DrawRegs dr = make_draw_regs(k);

  wave_chunks<kMode>(k, s, [&](uint64_t i, bool active, uint32_t path_lo, uint32_t path_hi) {
    float h[kS][K], v[kS], paid[kS];
    uint32_t ruin[kS], until[kS];
    bool alive[kS];
#pragma unroll
    for (int sc = 0; sc < kS; ++sc) {
#pragma unroll
      for (int y = 0; y < K; ++y) h[sc][y] = __fmul_rn(k.initial_capital, x.weights[sc][y]);
      v[sc] = 0.0f;  // set by the first period (n_periods >= 1)
      paid[sc] = 0.0f;
      ruin[sc] = 0u;
      alive[sc] = true;
      until[sc] = x.rebalance_every[sc];
    }
    float a[kDraws][K];
    walk_blocks<kDraws>(
        k.n_periods, [&](uint32_t blk) { portfolio_multipliers<kMode, kDense, K>(k, p, dr, s.table, path_lo, path_hi, blk, a); },
        [&](int j, uint32_t t) {
#pragma unroll
          for (int sc = 0; sc < kS; ++sc)
            portfolio_cashflow_step<kExactDiv, K>(a[j], x.weights[sc], x.amount[sc], x.fraction[sc], x.floor[sc], x.rebalance_every[sc],
                                                  k.n_periods, t, h[sc], v[sc], paid[sc], ruin[sc], alive[sc], until[sc]);
        });
#pragma unroll
    for (int sc = 0; sc < kS; ++sc) {
      if (static_cast<uint32_t>(sc) >= x.n) continue;  // uniform: a padded scenario leaves nothing
      const size_t at = static_cast<size_t>(sc) * k.n_paths + i;
      if (active) {
        if (k.d_final) k.d_final[at] = v[sc];
        if (p.d_holdings) {
#pragma unroll
          for (int y = 0; y < K; ++y) p.d_holdings[(static_cast<size_t>(sc) * K + y) * k.n_paths + i] = h[sc][y];
        }
        if (x.d_paid) x.d_paid[at] = paid[sc];
        if (x.d_ruin_period) x.d_ruin_period[at] = ruin[sc];
        if (want_dep) atomicAdd(&lds_dep[sc * n_at + ruin[sc]], 1u);  // ruin <= n_periods
      }
      if (want_stats)  // uniform: the whole wave
        wave_record_add(part + sc * kW, v[sc], active, lane, k.below_threshold, k.hist_lo, k.hist_hi, k.hist_inv,
                        want_hist ? k.n_bins : 0u, lds_hist + sc * k.n_bins);
    }
  });

  __syncthreads();  // the waves' partials are written and their LDS adds complete
  if (want_stats && threadIdx.x < x.n)
    fold_wave_partials<kW>(s.wave_part + threadIdx.x * kW, &k.partials[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x]);
  if (want_dep) flush_counters<kGroup>(lds_dep, x.n * n_at, x.d_depleted);
  if (want_hist) flush_counters<kGroup>(lds_hist, x.n * k.n_bins, k.d_hist);
}

}  // namespace

hipError_t launch_selftest(uint32_t lo, uint32_t hi, unsigned long long *d_count, uint32_t grid,
                           hipStream_t stream) {
  hipLaunchKernelGGL(selftest_kernel, dim3(grid), dim3(kBlock), 0, stream, lo, hi, d_count);
  return hipGetLastError();
}

// `table_len` is 0 in Gaussian mode, where the Box-Muller tables take the table's place.
// `table_len` is 0 in Gaussian mode; `stream` (2 | 3) then picks the Box-Muller table set
static size_t draw_table_words(uint32_t table_len, int stream) {
  return table_len ? table_len : (stream == 2 ? kBmFloats : kBm3LdsWords);
}
size_t paths_lds_bytes(uint32_t table_len, uint32_t n_bins, int stream) {
  // [draw tables][histogram][pad to 8 bytes][red_scratch: 4 kWaves doubles][wave_part: kWaves BlockPartial], the
  // last two once per 256-thread half of the workgroup (paths_halves)
  const size_t words = (draw_table_words(table_len, stream) + n_bins + 1u) & ~static_cast<size_t>(1);
  const size_t halves = paths_halves(table_len ? SMMC_MODE_TABLE : (stream == 2 ? kModeGaussianV2 : SMMC_MODE_GAUSSIAN));
  return words * 4u + halves * (4u * kWaves * sizeof(double) + kWaves * sizeof(BlockPartial));
}
bool table_is_dense(uint32_t table_len);
// keepdata_kernel: tables + per wave 64 rows of (tile 16 | 32 columns + kDraws more slots, at the
// larger of the two strides) + one trash word per thread
size_t keepdata_lds_bytes(uint32_t table_len, int tile, int waves, int stream) {
  const size_t table_words = draw_table_words(table_len, stream);
  const int draws = (table_len && table_is_dense(table_len)) ? 8 : 4;
  const int row = keepdata_row_words(tile, draws);
  return (table_words + static_cast<size_t>(waves) * 64 * (row + 1)) * 4u;
}
// Static LDS of the kernels that read their draw tables through absolute LDS addresses: must be 0.
hipError_t static_lds_bytes(size_t *bytes) {
  *bytes = 0;
  const void *kernels[] = {
      reinterpret_cast<const void *>(paths_kernel<SMMC_MODE_GAUSSIAN, kDivFast, false>),
      reinterpret_cast<const void *>(paths_kernel<SMMC_MODE_GAUSSIAN, kDivExact, false>),
      reinterpret_cast<const void *>(paths_kernel<SMMC_MODE_GAUSSIAN, kDivChecked, false>),
      reinterpret_cast<const void *>(paths_hi_kernel<SMMC_MODE_GAUSSIAN, kDivFast, false>),
      reinterpret_cast<const void *>(paths_hi_kernel<SMMC_MODE_GAUSSIAN, kDivExact, false>),
      reinterpret_cast<const void *>(paths_hi_kernel<SMMC_MODE_GAUSSIAN, kDivChecked, false>),
      reinterpret_cast<const void *>(keepdata_kernel<SMMC_MODE_GAUSSIAN, false, false, 32>),
      reinterpret_cast<const void *>(keepdata_kernel<SMMC_MODE_GAUSSIAN, true, false, 32>),
      reinterpret_cast<const void *>(keepdata_kernel<SMMC_MODE_GAUSSIAN, false, false, 16>),
      reinterpret_cast<const void *>(keepdata_kernel<SMMC_MODE_GAUSSIAN, true, false, 16>),
      reinterpret_cast<const void *>(keepdata_comb_kernel<SMMC_MODE_GAUSSIAN, false, false, 1>),
      reinterpret_cast<const void *>(keepdata_comb_kernel<SMMC_MODE_GAUSSIAN, true, false, 1>),
      reinterpret_cast<const void *>(keepdata_comb_kernel<SMMC_MODE_GAUSSIAN, false, false, 2>),
      reinterpret_cast<const void *>(keepdata_comb_kernel<SMMC_MODE_GAUSSIAN, true, false, 2>),
      reinterpret_cast<const void *>(checkpoints_kernel<SMMC_MODE_GAUSSIAN, false, false>),
      reinterpret_cast<const void *>(checkpoints_kernel<SMMC_MODE_GAUSSIAN, true, false>),
      reinterpret_cast<const void *>(cashflow_kernel<SMMC_MODE_GAUSSIAN, false, false, false>),
      reinterpret_cast<const void *>(cashflow_kernel<SMMC_MODE_GAUSSIAN, true, false, false>),
      reinterpret_cast<const void *>(cashflow_kernel<SMMC_MODE_GAUSSIAN, false, false, true>),
      reinterpret_cast<const void *>(cashflow_kernel<SMMC_MODE_GAUSSIAN, true, false, true>),
      reinterpret_cast<const void *>(excursions_kernel<SMMC_MODE_GAUSSIAN, false, false>),
      reinterpret_cast<const void *>(excursions_kernel<SMMC_MODE_GAUSSIAN, true, false>),
      reinterpret_cast<const void *>(draw_words_kernel<SMMC_MODE_GAUSSIAN, false>),
#define SMMC_SWEEP_KERNELS(S)                                                                                               \
  reinterpret_cast<const void *>(cashflow_sweep_kernel<SMMC_MODE_GAUSSIAN, false, false, S>),                                \
      reinterpret_cast<const void *>(cashflow_sweep_kernel<SMMC_MODE_GAUSSIAN, true, false, S>)
      SMMC_SWEEP_KERNELS(2), SMMC_SWEEP_KERNELS(4), SMMC_SWEEP_KERNELS(8),
#undef SMMC_SWEEP_KERNELS
#define SMMC_PORTFOLIO_KERNELS(K) /* both modes: the asset table is read through absolute addresses too */                  \
  reinterpret_cast<const void *>(portfolio_kernel<SMMC_MODE_GAUSSIAN, false, false, K>),                                     \
      reinterpret_cast<const void *>(portfolio_kernel<SMMC_MODE_GAUSSIAN, true, false, K>),                                  \
      reinterpret_cast<const void *>(portfolio_kernel<SMMC_MODE_TABLE, false, true, K>),                                     \
      reinterpret_cast<const void *>(portfolio_kernel<SMMC_MODE_TABLE, true, true, K>),                                      \
      reinterpret_cast<const void *>(portfolio_kernel<SMMC_MODE_TABLE, false, false, K>),                                    \
      reinterpret_cast<const void *>(portfolio_kernel<SMMC_MODE_TABLE, true, false, K>)
      SMMC_PORTFOLIO_KERNELS(1), SMMC_PORTFOLIO_KERNELS(2), SMMC_PORTFOLIO_KERNELS(3), SMMC_PORTFOLIO_KERNELS(4),
#undef SMMC_PORTFOLIO_KERNELS
#define SMMC_PORTFOLIO_CASHFLOW_KERNELS(K, V)                                                                               \
  reinterpret_cast<const void *>(portfolio_cashflow_kernel<SMMC_MODE_GAUSSIAN, false, false, K, V>),                         \
      reinterpret_cast<const void *>(portfolio_cashflow_kernel<SMMC_MODE_GAUSSIAN, true, false, K, V>),                      \
      reinterpret_cast<const void *>(portfolio_cashflow_kernel<SMMC_MODE_TABLE, false, true, K, V>),                         \
      reinterpret_cast<const void *>(portfolio_cashflow_kernel<SMMC_MODE_TABLE, true, true, K, V>),                          \
      reinterpret_cast<const void *>(portfolio_cashflow_kernel<SMMC_MODE_TABLE, false, false, K, V>),                        \
      reinterpret_cast<const void *>(portfolio_cashflow_kernel<SMMC_MODE_TABLE, true, false, K, V>)
      SMMC_PORTFOLIO_CASHFLOW_KERNELS(1, false), SMMC_PORTFOLIO_CASHFLOW_KERNELS(2, false),
      SMMC_PORTFOLIO_CASHFLOW_KERNELS(3, false), SMMC_PORTFOLIO_CASHFLOW_KERNELS(4, false),
      SMMC_PORTFOLIO_CASHFLOW_KERNELS(1, true), SMMC_PORTFOLIO_CASHFLOW_KERNELS(2, true),
      SMMC_PORTFOLIO_CASHFLOW_KERNELS(3, true), SMMC_PORTFOLIO_CASHFLOW_KERNELS(4, true),
#undef SMMC_PORTFOLIO_CASHFLOW_KERNELS
#define SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(K, V) /* table mode only */                                                  \
  reinterpret_cast<const void *>(portfolio_cashflow_blocks_kernel<false, true, K, V>),                                       \
      reinterpret_cast<const void *>(portfolio_cashflow_blocks_kernel<true, true, K, V>),                                    \
      reinterpret_cast<const void *>(portfolio_cashflow_blocks_kernel<false, false, K, V>),                                  \
      reinterpret_cast<const void *>(portfolio_cashflow_blocks_kernel<true, false, K, V>)
      SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(1, false), SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(2, false),
      SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(3, false), SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(4, false),
      SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(1, true), SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(2, true),
      SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(3, true), SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS(4, true),
#undef SMMC_PORTFOLIO_CASHFLOW_BLOCKS_KERNELS
#define SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(K, V) /* table mode only */                                               \
  reinterpret_cast<const void *>(portfolio_cashflow_stationary_kernel<false, true, K, V>),                                   \
      reinterpret_cast<const void *>(portfolio_cashflow_stationary_kernel<true, true, K, V>),                                \
      reinterpret_cast<const void *>(portfolio_cashflow_stationary_kernel<false, false, K, V>),                              \
      reinterpret_cast<const void *>(portfolio_cashflow_stationary_kernel<true, false, K, V>)
      SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(1, false), SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(2, false),
      SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(3, false), SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(4, false),
      SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(1, true), SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(2, true),
      SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(3, true), SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS(4, true),
#undef SMMC_PORTFOLIO_CASHFLOW_STATIONARY_KERNELS
#define SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(K, V) /* Gaussian mode only */                                              \
  reinterpret_cast<const void *>(portfolio_cashflow_regimes_kernel<false, K, V>),                                            \
      reinterpret_cast<const void *>(portfolio_cashflow_regimes_kernel<true, K, V>)
      SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(1, false), SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(2, false),
      SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(3, false), SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(4, false),
      SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(1, true), SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(2, true),
      SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(3, true), SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS(4, true),
#undef SMMC_PORTFOLIO_CASHFLOW_REGIMES_KERNELS
#define SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(K, V)                                                                  \
  reinterpret_cast<const void *>(portfolio_cashflow_checkpoints_kernel<SMMC_MODE_GAUSSIAN, false, false, K, V>),             \
      reinterpret_cast<const void *>(portfolio_cashflow_checkpoints_kernel<SMMC_MODE_GAUSSIAN, true, false, K, V>),          \
      reinterpret_cast<const void *>(portfolio_cashflow_checkpoints_kernel<SMMC_MODE_TABLE, false, true, K, V>),             \
      reinterpret_cast<const void *>(portfolio_cashflow_checkpoints_kernel<SMMC_MODE_TABLE, true, true, K, V>),              \
      reinterpret_cast<const void *>(portfolio_cashflow_checkpoints_kernel<SMMC_MODE_TABLE, false, false, K, V>),            \
      reinterpret_cast<const void *>(portfolio_cashflow_checkpoints_kernel<SMMC_MODE_TABLE, true, false, K, V>)
      SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(1, false), SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(2, false),
      SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(3, false), SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(4, false),
      SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(1, true), SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(2, true),
      SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(3, true), SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS(4, true),
#undef SMMC_PORTFOLIO_CASHFLOW_CHECKPOINTS_KERNELS
#define SMMC_REAL_CASHFLOW_KERNELS(K, V)                                                                                    \
  reinterpret_cast<const void *>(real_cashflow_kernel<SMMC_MODE_GAUSSIAN, false, false, K, V>),                              \
      reinterpret_cast<const void *>(real_cashflow_kernel<SMMC_MODE_GAUSSIAN, true, false, K, V>),                           \
      reinterpret_cast<const void *>(real_cashflow_kernel<SMMC_MODE_TABLE, false, true, K, V>),                              \
      reinterpret_cast<const void *>(real_cashflow_kernel<SMMC_MODE_TABLE, true, true, K, V>),                               \
      reinterpret_cast<const void *>(real_cashflow_kernel<SMMC_MODE_TABLE, false, false, K, V>),                             \
      reinterpret_cast<const void *>(real_cashflow_kernel<SMMC_MODE_TABLE, true, false, K, V>)
      SMMC_REAL_CASHFLOW_KERNELS(1, false), SMMC_REAL_CASHFLOW_KERNELS(2, false), SMMC_REAL_CASHFLOW_KERNELS(3, false),
      SMMC_REAL_CASHFLOW_KERNELS(1, true), SMMC_REAL_CASHFLOW_KERNELS(2, true), SMMC_REAL_CASHFLOW_KERNELS(3, true),
#undef SMMC_REAL_CASHFLOW_KERNELS
#define SMMC_GUARDRAILS_KERNELS(K)                                                                                          \
  reinterpret_cast<const void *>(guardrails_kernel<SMMC_MODE_GAUSSIAN, false, K>),                                           \
      reinterpret_cast<const void *>(guardrails_kernel<SMMC_MODE_TABLE, true, K>),                                           \
      reinterpret_cast<const void *>(guardrails_kernel<SMMC_MODE_TABLE, false, K>)
      SMMC_GUARDRAILS_KERNELS(1), SMMC_GUARDRAILS_KERNELS(2), SMMC_GUARDRAILS_KERNELS(3), SMMC_GUARDRAILS_KERNELS(4),
#undef SMMC_GUARDRAILS_KERNELS
#define SMMC_GLIDE_KERNELS(K, V)                                                                                            \
  reinterpret_cast<const void *>(glide_kernel<SMMC_MODE_GAUSSIAN, false, false, K, V>),                                      \
      reinterpret_cast<const void *>(glide_kernel<SMMC_MODE_GAUSSIAN, true, false, K, V>),                                   \
      reinterpret_cast<const void *>(glide_kernel<SMMC_MODE_TABLE, false, true, K, V>),                                      \
      reinterpret_cast<const void *>(glide_kernel<SMMC_MODE_TABLE, true, true, K, V>),                                       \
      reinterpret_cast<const void *>(glide_kernel<SMMC_MODE_TABLE, false, false, K, V>),                                     \
      reinterpret_cast<const void *>(glide_kernel<SMMC_MODE_TABLE, true, false, K, V>)
      SMMC_GLIDE_KERNELS(2, false), SMMC_GLIDE_KERNELS(3, false), SMMC_GLIDE_KERNELS(4, false),
      SMMC_GLIDE_KERNELS(2, true), SMMC_GLIDE_KERNELS(3, true), SMMC_GLIDE_KERNELS(4, true),
#undef SMMC_GLIDE_KERNELS
#define SMMC_ALLOCATION_SWEEP_KERNELS(K, S)                                                                               \
  reinterpret_cast<const void *>(allocation_sweep_kernel<SMMC_MODE_GAUSSIAN, false, false, K, S>),                           \
      reinterpret_cast<const void *>(allocation_sweep_kernel<SMMC_MODE_GAUSSIAN, true, false, K, S>),                        \
      reinterpret_cast<const void *>(allocation_sweep_kernel<SMMC_MODE_TABLE, false, true, K, S>),                           \
      reinterpret_cast<const void *>(allocation_sweep_kernel<SMMC_MODE_TABLE, true, true, K, S>),                            \
      reinterpret_cast<const void *>(allocation_sweep_kernel<SMMC_MODE_TABLE, false, false, K, S>),                          \
      reinterpret_cast<const void *>(allocation_sweep_kernel<SMMC_MODE_TABLE, true, false, K, S>)
      SMMC_ALLOCATION_SWEEP_KERNELS(1, 4), SMMC_ALLOCATION_SWEEP_KERNELS(2, 4), SMMC_ALLOCATION_SWEEP_KERNELS(3, 4),
      SMMC_ALLOCATION_SWEEP_KERNELS(4, 4), SMMC_ALLOCATION_SWEEP_KERNELS(1, 8), SMMC_ALLOCATION_SWEEP_KERNELS(2, 8),
      SMMC_ALLOCATION_SWEEP_KERNELS(3, 8), SMMC_ALLOCATION_SWEEP_KERNELS(4, 8),
#undef SMMC_ALLOCATION_SWEEP_KERNELS
  };
  for (const void *kernel : kernels) {
    hipFuncAttributes attr;
    hipError_t err = hipFuncGetAttributes(&attr, kernel);
    if (err != hipSuccess) return err;
    if (attr.sharedSizeBytes > *bytes) *bytes = attr.sharedSizeBytes;
  }
  return hipSuccess;
}

size_t bm_tables_bytes(int stream) { return (stream == 2 ? kBmFloats : kBm3Floats) * sizeof(float); }

// Launches above 64 KiB of dynamic LDS (a 16384-entry table plus a large histogram) need
// the opt-in limit raised for that kernel; CDNA4 has 160 KiB per CU.
template <typename Kernel>
static hipError_t allow_lds(Kernel kernel, size_t lds) {
  if (lds <= 60u * 1024u) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             static_cast<int>(lds));
}

// `grid` counts 256-thread virtual blocks (one partial each); a workgroup holds paths_halves(kMode) of them
template <int kMode, int kDiv, bool kDense>
static hipError_t launch_paths_variant(const KernelArgs &a, uint32_t grid, size_t lds, hipStream_t stream) {
  constexpr uint32_t kHalves = paths_halves(kMode);
  hipError_t err = allow_lds(paths_kernel<kMode, kDiv, kDense>, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((paths_kernel<kMode, kDiv, kDense>), dim3((grid + kHalves - 1) / kHalves), dim3(kBlock * kHalves), lds,
                     stream, a, grid);
  return hipGetLastError();
}

template <int kMode, bool kDense>
static hipError_t launch_paths_mode(const KernelArgs &a, int div, uint32_t grid, size_t lds, hipStream_t stream) {
  switch (div) {
    case SMMC_DIV_FAST: return launch_paths_variant<kMode, kDivFast, kDense>(a, grid, lds, stream);
    case SMMC_DIV_CHECKED: return launch_paths_variant<kMode, kDivChecked, kDense>(a, grid, lds, stream);
    default: return launch_paths_variant<kMode, kDivExact, kDense>(a, grid, lds, stream);
  }
}

// paths_hi_kernel in paths_kernel's place: same grid, workgroup and LDS
template <int kMode, int kDiv, bool kDense>
static hipError_t launch_paths_hi_variant(const KernelArgs &a, uint32_t grid, size_t lds, hipStream_t stream) {
  constexpr uint32_t kHalves = paths_halves(kMode);
  hipError_t err = allow_lds(paths_hi_kernel<kMode, kDiv, kDense>, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((paths_hi_kernel<kMode, kDiv, kDense>), dim3((grid + kHalves - 1) / kHalves), dim3(kBlock * kHalves), lds,
                     stream, a, grid);
  return hipGetLastError();
}

template <int kMode, bool kDense>
static hipError_t launch_paths_hi_mode(const KernelArgs &a, int div, uint32_t grid, size_t lds, hipStream_t stream) {
  switch (div) {
    case SMMC_DIV_FAST: return launch_paths_hi_variant<kMode, kDivFast, kDense>(a, grid, lds, stream);
    case SMMC_DIV_CHECKED: return launch_paths_hi_variant<kMode, kDivChecked, kDense>(a, grid, lds, stream);
    default: return launch_paths_hi_variant<kMode, kDivExact, kDense>(a, grid, lds, stream);
  }
}

bool table_is_dense(uint32_t table_len) { return table_len <= kDenseMaxTable; }

template <int kMode, bool kDense>
static hipError_t launch_draw_words_variant(const KernelArgs &a, const uint32_t *d_words, uint64_t n, int form, float *d_out,
                                            uint32_t grid, hipStream_t stream) {
  const size_t lds = draw_table_words(a.table_len, a.stream) * 4u;  // the tables alone, at LDS offset 0
  hipError_t err = allow_lds(draw_words_kernel<kMode, kDense>, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((draw_words_kernel<kMode, kDense>), dim3(grid), dim3(kBlock), lds, stream, a, d_words, n, form, d_out);
  return hipGetLastError();
}

// draw_words_kernel on n items (n >= 1): d_words n x 4, d_out n x keepdata_draws(a.table_len).  The mode ladder is
// launch_paths's, so `dense` is decided by the same rule.
hipError_t launch_draw_words(const KernelArgs &a, const uint32_t *d_words, uint64_t n, int form, float *d_out, uint32_t grid,
                             hipStream_t stream) {
  if (!n || !grid || (form != 0 && form != 1)) return hipErrorInvalidValue;
  if (a.mode != SMMC_MODE_TABLE)
    return a.stream == 2 ? launch_draw_words_variant<kModeGaussianV2, false>(a, d_words, n, form, d_out, grid, stream)
                         : launch_draw_words_variant<SMMC_MODE_GAUSSIAN, false>(a, d_words, n, form, d_out, grid, stream);
  if (a.stream == 2)
    return table_is_dense(a.table_len) ? launch_draw_words_variant<kModeTableV2, true>(a, d_words, n, form, d_out, grid, stream)
                                       : launch_draw_words_variant<kModeTableV2, false>(a, d_words, n, form, d_out, grid, stream);
  return table_is_dense(a.table_len) ? launch_draw_words_variant<SMMC_MODE_TABLE, true>(a, d_words, n, form, d_out, grid, stream)
                                     : launch_draw_words_variant<SMMC_MODE_TABLE, false>(a, d_words, n, form, d_out, grid, stream);
}

hipError_t launch_paths(const KernelArgs &a, int div, uint32_t grid, size_t lds_bytes, hipStream_t stream) {
  if (paths_form(a))  // every path of the launch has the same id bits 63..32: stream v3, Gaussian or a dense table
    return a.mode != SMMC_MODE_TABLE ? launch_paths_hi_mode<SMMC_MODE_GAUSSIAN, false>(a, div, grid, lds_bytes, stream)
                                     : launch_paths_hi_mode<SMMC_MODE_TABLE, true>(a, div, grid, lds_bytes, stream);
  if (a.mode != SMMC_MODE_TABLE)
    return a.stream == 2 ? launch_paths_mode<kModeGaussianV2, false>(a, div, grid, lds_bytes, stream)
                         : launch_paths_mode<SMMC_MODE_GAUSSIAN, false>(a, div, grid, lds_bytes, stream);
  if (a.stream == 2)
    return table_is_dense(a.table_len) ? launch_paths_mode<kModeTableV2, true>(a, div, grid, lds_bytes, stream)
                                       : launch_paths_mode<kModeTableV2, false>(a, div, grid, lds_bytes, stream);
  return table_is_dense(a.table_len) ? launch_paths_mode<SMMC_MODE_TABLE, true>(a, div, grid, lds_bytes, stream)
                                     : launch_paths_mode<SMMC_MODE_TABLE, false>(a, div, grid, lds_bytes, stream);
}

hipError_t launch_finalize(const BlockPartial *partials, uint32_t n_partials, smmc_stats *d_stats,
                           uint32_t n_bins, hipStream_t stream, unsigned long long *hist_acc, uint32_t spread) {
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kFinalizeBlock), 0, stream, partials, n_partials, d_stats,
                     n_bins, hist_acc, spread);
  return hipGetLastError();
}

template <int kMode, bool kDense, int kTile>
static hipError_t launch_keepdata_tile(const KernelArgs &a, bool exact_div, uint32_t grid, uint32_t block,
                                        size_t lds, hipStream_t stream) {
  hipError_t err = exact_div ? allow_lds(keepdata_kernel<kMode, true, kDense, kTile>, lds)
                             : allow_lds(keepdata_kernel<kMode, false, kDense, kTile>, lds);
  if (err != hipSuccess) return err;
  if (exact_div)
    hipLaunchKernelGGL((keepdata_kernel<kMode, true, kDense, kTile>), dim3(grid), dim3(block), lds, stream, a);
  else
    hipLaunchKernelGGL((keepdata_kernel<kMode, false, kDense, kTile>), dim3(grid), dim3(block), lds, stream, a);
  return hipGetLastError();
}

template <int kMode, bool kDense>
static hipError_t launch_keepdata_mode(const KernelArgs &a, bool exact_div, int tile, int waves, uint32_t grid,
                                       hipStream_t stream) {
  const size_t lds = keepdata_lds_bytes(a.table_len, tile, waves, a.stream);
  const uint32_t block = static_cast<uint32_t>(waves) * 64u;
  if (waves < 1 || block > static_cast<uint32_t>(kKeepdataMaxBlock)) return hipErrorInvalidValue;
  switch (tile) {
    case 16: return launch_keepdata_tile<kMode, kDense, 16>(a, exact_div, grid, block, lds, stream);
    case 32: return launch_keepdata_tile<kMode, kDense, 32>(a, exact_div, grid, block, lds, stream);
    default: return hipErrorInvalidValue;
  }
}

size_t keepdata_comb_lds_bytes(uint32_t table_len, int waves, int stream) {
  const size_t table_words = draw_table_words(table_len, stream);
  const int draws = (table_len && table_is_dense(table_len)) ? 8 : 4;
  return (table_words + static_cast<size_t>(waves) * comb_tile_words(draws)) * 4u;
}
uint32_t keepdata_draws(uint32_t table_len) { return (table_len && table_is_dense(table_len)) ? 8u : 4u; }

template <int kMode, bool kDense, int kBlocksPerStep>
static hipError_t launch_comb_variant(const KernelArgs &a, bool exact_div, uint32_t rows_per_stream, uint64_t n_wave_chunks,
                                      uint64_t n_rows_total, int waves, uint32_t grid, unsigned long long *next_chunk,
                                      hipStream_t stream) {
  const size_t lds = keepdata_comb_lds_bytes(a.table_len, waves, a.stream);
  const uint32_t block = static_cast<uint32_t>(waves) * 64u;
  if (waves < 1 || block > static_cast<uint32_t>(kCombMaxBlock)) return hipErrorInvalidValue;
  hipError_t err = exact_div ? allow_lds(keepdata_comb_kernel<kMode, true, kDense, kBlocksPerStep>, lds)
                             : allow_lds(keepdata_comb_kernel<kMode, false, kDense, kBlocksPerStep>, lds);
  if (err != hipSuccess) return err;
  if (exact_div)
    hipLaunchKernelGGL((keepdata_comb_kernel<kMode, true, kDense, kBlocksPerStep>), dim3(grid), dim3(block), lds, stream, a,
                       rows_per_stream, n_wave_chunks, n_rows_total, next_chunk);
  else
    hipLaunchKernelGGL((keepdata_comb_kernel<kMode, false, kDense, kBlocksPerStep>), dim3(grid), dim3(block), lds, stream, a,
                       rows_per_stream, n_wave_chunks, n_rows_total, next_chunk);
  return hipGetLastError();
}

template <int kMode, bool kDense>
static hipError_t launch_comb_mode(const KernelArgs &a, bool exact_div, int blocks_per_step, uint32_t rows_per_stream,
                                   uint64_t n_wave_chunks, uint64_t n_rows_total, int waves, uint32_t grid,
                                   unsigned long long *next_chunk, hipStream_t stream) {
  return blocks_per_step == 2 ? launch_comb_variant<kMode, kDense, 2>(a, exact_div, rows_per_stream, n_wave_chunks, n_rows_total,
                                                                      waves, grid, next_chunk, stream)
                              : launch_comb_variant<kMode, kDense, 1>(a, exact_div, rows_per_stream, n_wave_chunks, n_rows_total,
                                                                      waves, grid, next_chunk, stream);
}

// blocks_per_step: 1 or 2 (2 needs n_periods / draws per block to be even)
hipError_t launch_keepdata_comb(const KernelArgs &a, bool exact_div, int blocks_per_step, uint32_t rows_per_stream,
                                uint64_t n_wave_chunks, uint64_t n_rows_total, int waves, uint32_t grid,
                                unsigned long long *next_chunk, hipStream_t stream) {
  hipError_t err = hipMemsetAsync(next_chunk, 0, sizeof(unsigned long long), stream);
  if (err != hipSuccess) return err;
  if (a.mode != SMMC_MODE_TABLE)
    return a.stream == 2 ? launch_comb_mode<kModeGaussianV2, false>(a, exact_div, blocks_per_step, rows_per_stream, n_wave_chunks,
                                                                    n_rows_total, waves, grid, next_chunk, stream)
                         : launch_comb_mode<SMMC_MODE_GAUSSIAN, false>(a, exact_div, blocks_per_step, rows_per_stream, n_wave_chunks,
                                                                       n_rows_total, waves, grid, next_chunk, stream);
  if (a.stream == 2)
    return table_is_dense(a.table_len)
               ? launch_comb_mode<kModeTableV2, true>(a, exact_div, blocks_per_step, rows_per_stream, n_wave_chunks, n_rows_total,
                                                      waves, grid, next_chunk, stream)
               : launch_comb_mode<kModeTableV2, false>(a, exact_div, blocks_per_step, rows_per_stream, n_wave_chunks, n_rows_total,
                                                       waves, grid, next_chunk, stream);
  return table_is_dense(a.table_len)
             ? launch_comb_mode<SMMC_MODE_TABLE, true>(a, exact_div, blocks_per_step, rows_per_stream, n_wave_chunks, n_rows_total,
                                                       waves, grid, next_chunk, stream)
             : launch_comb_mode<SMMC_MODE_TABLE, false>(a, exact_div, blocks_per_step, rows_per_stream, n_wave_chunks, n_rows_total,
                                                        waves, grid, next_chunk, stream);
}

hipError_t launch_final_column(const float *traj, uint64_t n_rows, uint32_t row_len, float *d_final, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(final_column_kernel, dim3(grid), dim3(kBlock), 0, stream, traj, n_rows, row_len, d_final);
  return hipGetLastError();
}

hipError_t launch_keepdata(const KernelArgs &a, bool exact_div, int tile, int waves, uint32_t grid,
                           hipStream_t stream) {
  if (a.mode != SMMC_MODE_TABLE)
    return a.stream == 2 ? launch_keepdata_mode<kModeGaussianV2, false>(a, exact_div, tile, waves, grid, stream)
                         : launch_keepdata_mode<SMMC_MODE_GAUSSIAN, false>(a, exact_div, tile, waves, grid, stream);
  if (a.stream == 2)
    return table_is_dense(a.table_len) ? launch_keepdata_mode<kModeTableV2, true>(a, exact_div, tile, waves, grid, stream)
                                       : launch_keepdata_mode<kModeTableV2, false>(a, exact_div, tile, waves, grid, stream);
  return table_is_dense(a.table_len) ? launch_keepdata_mode<SMMC_MODE_TABLE, true>(a, exact_div, tile, waves, grid, stream)
                                     : launch_keepdata_mode<SMMC_MODE_TABLE, false>(a, exact_div, tile, waves, grid, stream);
}

// ---- the wave-walk kernels: checkpoints, cash flows, excursions ----

static_assert(wave_walk_group_paths(SMMC_MODE_TABLE) == 64u * walk_waves(SMMC_MODE_TABLE) &&
                  wave_walk_group_paths(SMMC_MODE_GAUSSIAN) == 64u * walk_waves(SMMC_MODE_GAUSSIAN),
              "smmc_internal.h states the workgroup sizes the kernels are compiled for");

// walk_setup's layout: [draw tables][counter_words u32 counters][pad to 8 bytes][partials_per_wave BlockPartial per wave]
static size_t wave_walk_lds_bytes(int32_t mode, uint32_t table_len, size_t counter_words, uint32_t partials_per_wave) {
  const bool table = mode == SMMC_MODE_TABLE;
  const size_t words = (static_cast<size_t>(table ? table_len : bm_lds_words(SMMC_MODE_GAUSSIAN)) + counter_words + 1u) & ~static_cast<size_t>(1);
  return words * 4u + partials_per_wave * static_cast<size_t>(wave_walk_group_paths(mode) / 64u) * sizeof(BlockPartial);
}

// One ladder for the three: Gaussian | dense table | four-draw table, times exact | fast divide.  `Family` names a
// kernel's instantiations: Family::get<kMode, kExactDiv, kDense>(x) is the one to launch for the arguments x.
template <typename Args>
using WalkKernel = void (*)(const KernelArgs, const Args);
template <typename Family, bool kExactDiv, typename Args>
static WalkKernel<Args> wave_walk_kernel(const KernelArgs &a, const Args &x) {
  if (a.mode != SMMC_MODE_TABLE) return Family::template get<SMMC_MODE_GAUSSIAN, kExactDiv, false>(x);
  return table_is_dense(a.table_len) ? Family::template get<SMMC_MODE_TABLE, kExactDiv, true>(x)
                                     : Family::template get<SMMC_MODE_TABLE, kExactDiv, false>(x);
}
template <typename Family, typename Args>
static hipError_t launch_wave_walk(const KernelArgs &a, const Args &x, bool exact_div, uint32_t grid, size_t lds, hipStream_t stream) {
  const WalkKernel<Args> kernel = exact_div ? wave_walk_kernel<Family, true>(a, x) : wave_walk_kernel<Family, false>(a, x);
  const hipError_t err = allow_lds(kernel, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(wave_walk_group_paths(a.mode)), lds, stream, a, x);
  return hipGetLastError();
}

size_t checkpoints_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_checkpoints, uint32_t n_bins) {
  const bool table = mode == SMMC_MODE_TABLE;
  const uint32_t front = checkpoint_front_words(table ? table_len : bm_lds_words(SMMC_MODE_GAUSSIAN),
                                                walk_waves(table ? SMMC_MODE_TABLE : SMMC_MODE_GAUSSIAN), n_checkpoints);
  return (static_cast<size_t>(front) + static_cast<size_t>(n_checkpoints) * n_bins) * 4u;
}

struct CheckpointsFamily {
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<CheckpointArgs> get(const CheckpointArgs &) { return checkpoints_kernel<kMode, kExactDiv, kDense>; }
};
// a.partials: n_checkpoints x grid entries ([checkpoint][workgroup]); a.d_hist: n_checkpoints x a.n_bins zeroed counters
hipError_t launch_checkpoints(const KernelArgs &a, const uint32_t *periods, uint32_t n_checkpoints, bool exact_div, uint32_t grid,
                              hipStream_t stream) {
  if (n_checkpoints < 1 || n_checkpoints > SMMC_MAX_CHECKPOINTS || a.stream == 2) return hipErrorInvalidValue;
  CheckpointArgs c;
  c.n = n_checkpoints;
  for (uint32_t i = 0; i < SMMC_MAX_CHECKPOINTS; ++i) c.periods[i] = i < n_checkpoints ? periods[i] : 0xffffffffu;
  return launch_wave_walk<CheckpointsFamily>(a, c, exact_div, grid, checkpoints_lds_bytes(a.mode, a.table_len, n_checkpoints, a.n_bins), stream);
}

hipError_t launch_finalize_checkpoints(const BlockPartial *partials, uint32_t n_partials, uint32_t n_checkpoints, void *d_records,
                                       uint32_t n_bins, unsigned long long *hist_acc, hipStream_t stream) {
  hipLaunchKernelGGL(finalize_checkpoints_kernel, dim3(n_checkpoints), dim3(kCheckpointFinalizeBlock), 0, stream, partials,
                     n_partials, static_cast<unsigned char *>(d_records), n_bins, hist_acc);
  return hipGetLastError();
}

// ---- cash flows ----

size_t cashflow_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_periods, uint32_t n_bins) {
  // counters: depletion [n_periods + 1], histogram [n_bins]; one partial per wave
  return wave_walk_lds_bytes(mode, table_len, static_cast<size_t>(n_periods) + 1u + n_bins, 1u);
}

struct CashflowFamily {
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<CashflowArgs> get(const CashflowArgs &c) {
    return c.schedule ? cashflow_kernel<kMode, kExactDiv, kDense, true> : cashflow_kernel<kMode, kExactDiv, kDense, false>;
  }
};
hipError_t launch_cashflow(const KernelArgs &a, const CashflowArgs &c, bool exact_div, uint32_t grid, hipStream_t stream) {
  if (a.stream == 2 || a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (c.schedule && (c.stride % 8u != 0u || c.stride < a.n_periods)) return hipErrorInvalidValue;
  return launch_wave_walk<CashflowFamily>(a, c, exact_div, grid, cashflow_lds_bytes(a.mode, a.table_len, a.n_periods, a.n_bins), stream);
}

hipError_t launch_finalize_depleted(unsigned long long *acc, uint32_t n, unsigned long long *d_out, hipStream_t stream) {
  hipLaunchKernelGGL(finalize_depleted_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, acc, n, d_out);
  return hipGetLastError();
}

// ---- cash-flow sweeps ----

size_t cashflow_sweep_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_periods, uint32_t n_bins, uint32_t n_scenarios) {
  // counters: per scenario depletion [n_periods + 1] and histogram [n_bins]; sweep_width(n_scenarios) partials per wave
  return wave_walk_lds_bytes(mode, table_len, static_cast<size_t>(n_scenarios) * (static_cast<size_t>(n_periods) + 1u + n_bins),
                             sweep_width(n_scenarios));
}

struct SweepFamily {
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<SweepArgs> get(const SweepArgs &c) {
    switch (sweep_width(c.n)) {
      case 2: return cashflow_sweep_kernel<kMode, kExactDiv, kDense, 2>;
      case 4: return cashflow_sweep_kernel<kMode, kExactDiv, kDense, 4>;
      default: return cashflow_sweep_kernel<kMode, kExactDiv, kDense, 8>;
    }
  }
};
// a.d_final, c.d_paid, c.d_ruin_period: [c.n][a.n_paths]; a.partials: [c.n][grid]; a.d_hist: [c.n][a.n_bins] and
// c.d_depleted: [c.n][a.n_periods + 1] counters, zero before the launch.  The entries of c from c.n up to
// sweep_width(c.n) must be copies of entry c.n - 1.
hipError_t launch_cashflow_sweep(const KernelArgs &a, const SweepArgs &c, bool exact_div, uint32_t grid, hipStream_t stream) {
  if (a.stream == 2 || a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (c.n < 1 || c.n > SMMC_MAX_SWEEP) return hipErrorInvalidValue;
  if (static_cast<uint64_t>(c.n) * (static_cast<uint64_t>(a.n_periods) + 1u + a.n_bins) > SMMC_MAX_SWEEP_COUNTERS) return hipErrorInvalidValue;
  return launch_wave_walk<SweepFamily>(a, c, exact_div, grid, cashflow_sweep_lds_bytes(a.mode, a.table_len, a.n_periods, a.n_bins, c.n),
                                       stream);
}

hipError_t launch_finalize_sweep(const BlockPartial *partials, uint32_t n_partials, uint32_t n_scenarios, void *d_records,
                                 uint32_t n_bins, unsigned long long *hist_acc, hipStream_t stream) {
  hipLaunchKernelGGL(finalize_checkpoints_kernel, dim3(n_scenarios), dim3(kCheckpointFinalizeBlock), 0, stream, partials, n_partials,
                     static_cast<unsigned char *>(d_records), n_bins, hist_acc);
  return hipGetLastError();
}

// ---- block bootstrap ----

size_t blocks_lds_bytes(uint32_t table_len, uint32_t n_bins, bool wide) {
  // paths_lds_bytes with the staged copies in the table's place
  const size_t words = (static_cast<size_t>(blocks_table_words(table_len, wide)) + n_bins + 1u) & ~static_cast<size_t>(1);
  return words * 4u + 4u * kWaves * sizeof(double) + kWaves * sizeof(BlockPartial);
}

template <int kDiv, bool kDense, bool kWide>
static hipError_t launch_blocks_variant(const KernelArgs &a, uint32_t block_len, uint32_t grid, size_t lds, hipStream_t stream) {
  hipError_t err = allow_lds(blocks_kernel<kDiv, kDense, kWide>, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((blocks_kernel<kDiv, kDense, kWide>), dim3(grid), dim3(kBlock), lds, stream, a, grid, block_len);
  return hipGetLastError();
}

template <bool kDense, bool kWide>
static hipError_t launch_blocks_layout(const KernelArgs &a, uint32_t block_len, int div, uint32_t grid, size_t lds, hipStream_t stream) {
  switch (div) {
    case SMMC_DIV_FAST: return launch_blocks_variant<kDivFast, kDense, kWide>(a, block_len, grid, lds, stream);
    case SMMC_DIV_CHECKED: return launch_blocks_variant<kDivChecked, kDense, kWide>(a, block_len, grid, lds, stream);
    default: return launch_blocks_variant<kDivExact, kDense, kWide>(a, block_len, grid, lds, stream);
  }
}

hipError_t launch_blocks(const KernelArgs &a, uint32_t block_len, bool wide, int div, uint32_t grid, hipStream_t stream) {
  if (a.mode != SMMC_MODE_TABLE || a.stream != 3 || !a.table_len || !block_len) return hipErrorInvalidValue;
  const size_t lds = blocks_lds_bytes(a.table_len, a.partials ? a.n_bins : 0u, wide);
  if (!table_is_dense(a.table_len))
    return wide ? launch_blocks_layout<false, true>(a, block_len, div, grid, lds, stream)
                : launch_blocks_layout<false, false>(a, block_len, div, grid, lds, stream);
  return wide ? launch_blocks_layout<true, true>(a, block_len, div, grid, lds, stream)
              : launch_blocks_layout<true, false>(a, block_len, div, grid, lds, stream);
}

// ---- stationary bootstrap ----

size_t stationary_lds_bytes(uint32_t table_len, uint32_t n_bins) {
  // paths_lds_bytes in table mode: one plain copy of the table in front of the histogram
  const size_t words = (static_cast<size_t>(table_len) + n_bins + 1u) & ~static_cast<size_t>(1);
  return words * 4u + 4u * kWaves * sizeof(double) + kWaves * sizeof(BlockPartial);
}

template <int kDiv, bool kDense>
static hipError_t launch_stationary_variant(const KernelArgs &a, uint32_t renew_q16, uint32_t grid, size_t lds, hipStream_t stream) {
  hipError_t err = allow_lds(stationary_kernel<kDiv, kDense>, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((stationary_kernel<kDiv, kDense>), dim3(grid), dim3(kBlock), lds, stream, a, grid, renew_q16);
  return hipGetLastError();
}

template <bool kDense>
static hipError_t launch_stationary_layout(const KernelArgs &a, uint32_t renew_q16, int div, uint32_t grid, size_t lds, hipStream_t stream) {
  switch (div) {
    case SMMC_DIV_FAST: return launch_stationary_variant<kDivFast, kDense>(a, renew_q16, grid, lds, stream);
    case SMMC_DIV_CHECKED: return launch_stationary_variant<kDivChecked, kDense>(a, renew_q16, grid, lds, stream);
    default: return launch_stationary_variant<kDivExact, kDense>(a, renew_q16, grid, lds, stream);
  }
}

hipError_t launch_stationary(const KernelArgs &a, uint32_t renew_q16, int div, uint32_t grid, hipStream_t stream) {
  if (a.mode != SMMC_MODE_TABLE || a.stream != 3 || !a.table_len || renew_q16 > SMMC_RENEW_Q16_ONE) return hipErrorInvalidValue;
  const size_t lds = stationary_lds_bytes(a.table_len, a.partials ? a.n_bins : 0u);
  return table_is_dense(a.table_len) ? launch_stationary_layout<true>(a, renew_q16, div, grid, lds, stream)
                                     : launch_stationary_layout<false>(a, renew_q16, div, grid, lds, stream);
}

// ---- regime-switching Gaussian paths ----

size_t regimes_lds_bytes(uint32_t n_bins) {
  // paths_lds_bytes in Gaussian mode, one 256-thread workgroup: the v3 draw tables in front of the histogram
  const size_t words = (static_cast<size_t>(bm_lds_words(SMMC_MODE_GAUSSIAN)) + n_bins + 1u) & ~static_cast<size_t>(1);
  return words * 4u + 4u * kWaves * sizeof(double) + kWaves * sizeof(BlockPartial);
}

template <int kDiv>
static hipError_t launch_regimes_variant(const KernelArgs &a, const RegimeArgs &r, uint32_t grid, size_t lds, hipStream_t stream) {
  hipError_t err = allow_lds(regimes_kernel<kDiv>, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((regimes_kernel<kDiv>), dim3(grid), dim3(kBlock), lds, stream, a, grid, r);
  return hipGetLastError();
}

hipError_t launch_regimes(const KernelArgs &a, const RegimeArgs &r, int div, uint32_t grid, hipStream_t stream) {
  if (a.mode != SMMC_MODE_GAUSSIAN || a.stream != 3 || a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f) return hipErrorInvalidValue;
  if (r.leave_q16[0] > SMMC_REGIME_Q16_ONE || r.leave_q16[1] > SMMC_REGIME_Q16_ONE || r.start1_q16 > SMMC_REGIME_Q16_ONE)
    return hipErrorInvalidValue;
  const size_t lds = regimes_lds_bytes(a.partials ? a.n_bins : 0u);
  switch (div) {
    case SMMC_DIV_FAST: return launch_regimes_variant<kDivFast>(a, r, grid, lds, stream);
    case SMMC_DIV_CHECKED: return launch_regimes_variant<kDivChecked>(a, r, grid, lds, stream);
    default: return launch_regimes_variant<kDivExact>(a, r, grid, lds, stream);
  }
}

// ---- excursions ----

size_t excursions_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_periods, uint32_t n_bins) {
  // counters: first_below and first_reach [n_periods + 1] each, the histograms of the final values and of the
  // drawdowns [n_bins] each; two partials per wave
  return wave_walk_lds_bytes(mode, table_len, 2u * (static_cast<size_t>(n_periods) + 1u) + 2u * static_cast<size_t>(n_bins), 2u);
}

struct ExcursionsFamily {
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<ExcursionArgs> get(const ExcursionArgs &) { return excursions_kernel<kMode, kExactDiv, kDense>; }
};
hipError_t launch_excursions(const KernelArgs &a, const ExcursionArgs &x, bool exact_div, uint32_t grid, hipStream_t stream) {
  if (a.stream == 2 || a.n_periods == 0 || a.n_periods > SMMC_MAX_EXCURSION_PERIODS) return hipErrorInvalidValue;
  return launch_wave_walk<ExcursionsFamily>(a, x, exact_div, grid, excursions_lds_bytes(a.mode, a.table_len, a.n_periods, a.n_bins), stream);
}

// ---- portfolios ----

size_t portfolio_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_bins) {
  // the padded rows in the table's place; counters: the histogram [n_bins]; one partial per wave
  return wave_walk_lds_bytes(mode, n_rows * portfolio_row_words(n_assets), n_bins, 1u);
}

struct PortfolioFamily {
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<PortfolioArgs> get(const PortfolioArgs &p) {
    switch (p.n_assets) {
      case 1: return portfolio_kernel<kMode, kExactDiv, kDense, 1>;
      case 2: return portfolio_kernel<kMode, kExactDiv, kDense, 2>;
      case 3: return portfolio_kernel<kMode, kExactDiv, kDense, 3>;
      default: return portfolio_kernel<kMode, kExactDiv, kDense, 4>;
    }
  }
};
hipError_t launch_portfolio(const KernelArgs &a, const PortfolioArgs &p, bool exact_div, uint32_t grid, hipStream_t stream) {
  if (a.stream != 3 || p.n_assets < 1 || p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.mode == SMMC_MODE_TABLE ? (!a.table_len || !a.table_a) : (a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f)) return hipErrorInvalidValue;
  return launch_wave_walk<PortfolioFamily>(a, p, exact_div, grid, portfolio_lds_bytes(a.mode, a.table_len, p.n_assets, a.n_bins), stream);
}

// ---- portfolio cash flows ----

size_t portfolio_cashflow_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins) {
  // the padded rows in the table's place; counters: depletion [n_periods + 1], histogram [n_bins]; one partial per wave
  return wave_walk_lds_bytes(mode, n_rows * portfolio_row_words(n_assets), static_cast<size_t>(n_periods) + 1u + n_bins, 1u);
}

struct PortfolioCashflowFamily {
  template <int kMode, bool kExactDiv, bool kDense, int K>
  static WalkKernel<PortfolioCashflowArgs> schedule(const PortfolioCashflowArgs &x) {
    return x.c.schedule ? portfolio_cashflow_kernel<kMode, kExactDiv, kDense, K, true>
                        : portfolio_cashflow_kernel<kMode, kExactDiv, kDense, K, false>;
  }
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<PortfolioCashflowArgs> get(const PortfolioCashflowArgs &x) {
    switch (x.p.n_assets) {
      case 1: return schedule<kMode, kExactDiv, kDense, 1>(x);
      case 2: return schedule<kMode, kExactDiv, kDense, 2>(x);
      case 3: return schedule<kMode, kExactDiv, kDense, 3>(x);
      default: return schedule<kMode, kExactDiv, kDense, 4>(x);
    }
  }
};
hipError_t launch_portfolio_cashflow(const KernelArgs &a, const PortfolioCashflowArgs &x, bool exact_div, uint32_t grid,
                                     hipStream_t stream) {
  if (a.stream != 3 || x.p.n_assets < 1 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.mode == SMMC_MODE_TABLE ? (!a.table_len || !a.table_a) : (a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f)) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.c.schedule && (x.c.stride % 8u != 0u || x.c.stride < a.n_periods)) return hipErrorInvalidValue;
  return launch_wave_walk<PortfolioCashflowFamily>(
      a, x, exact_div, grid, portfolio_cashflow_lds_bytes(a.mode, a.table_len, x.p.n_assets, a.n_periods, a.n_bins), stream);
}

// ---- block-bootstrap plans ----

size_t portfolio_cashflow_blocks_lds_bytes(uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins) {
  // the parent's layout with the circularly extended rows in the table's place
  return wave_walk_lds_bytes(SMMC_MODE_TABLE, portfolio_cashflow_blocks_rows(n_rows) * portfolio_row_words(n_assets),
                             static_cast<size_t>(n_periods) + 1u + n_bins, 1u);
}

struct PortfolioCashflowBlocksFamily {  // table mode only: its own ladder, dense | four-draw table times exact | fast divide
  template <bool kExactDiv, bool kDense, int K>
  static WalkKernel<PortfolioCashflowBlocksArgs> schedule(const PortfolioCashflowBlocksArgs &x) {
    return x.c.schedule ? portfolio_cashflow_blocks_kernel<kExactDiv, kDense, K, true>
                        : portfolio_cashflow_blocks_kernel<kExactDiv, kDense, K, false>;
  }
  template <bool kExactDiv, bool kDense>
  static WalkKernel<PortfolioCashflowBlocksArgs> assets(const PortfolioCashflowBlocksArgs &x) {
    switch (x.p.n_assets) {
      case 1: return schedule<kExactDiv, kDense, 1>(x);
      case 2: return schedule<kExactDiv, kDense, 2>(x);
      case 3: return schedule<kExactDiv, kDense, 3>(x);
      default: return schedule<kExactDiv, kDense, 4>(x);
    }
  }
  static WalkKernel<PortfolioCashflowBlocksArgs> get(const KernelArgs &a, const PortfolioCashflowBlocksArgs &x, bool exact_div) {
    if (table_is_dense(a.table_len)) return exact_div ? assets<true, true>(x) : assets<false, true>(x);
    return exact_div ? assets<true, false>(x) : assets<false, false>(x);
  }
};
hipError_t launch_portfolio_cashflow_blocks(const KernelArgs &a, const PortfolioCashflowBlocksArgs &x, bool exact_div, uint32_t grid,
                                            hipStream_t stream) {
  if (a.stream != 3 || a.mode != SMMC_MODE_TABLE || !a.table_len || !a.table_a || !x.block_len) return hipErrorInvalidValue;
  if (x.p.n_assets < 1 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.c.schedule && x.c.stride < a.n_periods) return hipErrorInvalidValue;
  const size_t lds = portfolio_cashflow_blocks_lds_bytes(a.table_len, x.p.n_assets, a.n_periods, a.n_bins);
  const WalkKernel<PortfolioCashflowBlocksArgs> kernel = PortfolioCashflowBlocksFamily::get(a, x, exact_div);
  const hipError_t err = allow_lds(kernel, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(wave_walk_group_paths(SMMC_MODE_TABLE)), lds, stream, a, x);
  return hipGetLastError();
}

// ---- stationary-bootstrap plans ----

size_t portfolio_cashflow_geometric_lds_bytes(uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins) {
  // the parent's table-mode layout: one plain copy of the padded rows, the wrap is the draw's select
  return wave_walk_lds_bytes(SMMC_MODE_TABLE, n_rows * portfolio_row_words(n_assets), static_cast<size_t>(n_periods) + 1u + n_bins, 1u);
}

struct PortfolioCashflowStationaryFamily {  // table mode only: its own ladder, dense | four-draw table times exact | fast divide
  template <bool kExactDiv, bool kDense, int K>
  static WalkKernel<PortfolioCashflowStationaryArgs> schedule(const PortfolioCashflowStationaryArgs &x) {
    return x.c.schedule ? portfolio_cashflow_stationary_kernel<kExactDiv, kDense, K, true>
                        : portfolio_cashflow_stationary_kernel<kExactDiv, kDense, K, false>;
  }
  template <bool kExactDiv, bool kDense>
  static WalkKernel<PortfolioCashflowStationaryArgs> assets(const PortfolioCashflowStationaryArgs &x) {
    switch (x.p.n_assets) {
      case 1: return schedule<kExactDiv, kDense, 1>(x);
      case 2: return schedule<kExactDiv, kDense, 2>(x);
      case 3: return schedule<kExactDiv, kDense, 3>(x);
      default: return schedule<kExactDiv, kDense, 4>(x);
    }
  }
  static WalkKernel<PortfolioCashflowStationaryArgs> get(const KernelArgs &a, const PortfolioCashflowStationaryArgs &x, bool exact_div) {
    if (table_is_dense(a.table_len)) return exact_div ? assets<true, true>(x) : assets<false, true>(x);
    return exact_div ? assets<true, false>(x) : assets<false, false>(x);
  }
};
hipError_t launch_portfolio_cashflow_geometric(const KernelArgs &a, const PortfolioCashflowStationaryArgs &x, bool exact_div, uint32_t grid,
                                                hipStream_t stream) {
  if (a.stream != 3 || a.mode != SMMC_MODE_TABLE || !a.table_len || !a.table_a || x.renew_q16 > SMMC_RENEW_Q16_ONE) return hipErrorInvalidValue;
  if (x.p.n_assets < 1 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.c.schedule && x.c.stride < a.n_periods) return hipErrorInvalidValue;
  const size_t lds = portfolio_cashflow_geometric_lds_bytes(a.table_len, x.p.n_assets, a.n_periods, a.n_bins);
  const WalkKernel<PortfolioCashflowStationaryArgs> kernel = PortfolioCashflowStationaryFamily::get(a, x, exact_div);
  const hipError_t err = allow_lds(kernel, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(wave_walk_group_paths(SMMC_MODE_TABLE)), lds, stream, a, x);
  return hipGetLastError();
}

// ---- regime-switching plans ----

size_t portfolio_cashflow_markov_lds_bytes(uint32_t n_periods, uint32_t n_bins) {
  // the parent's Gaussian layout: the v3 draw tables; counters: depletion [n_periods + 1], histogram [n_bins]; one partial per wave
  return wave_walk_lds_bytes(SMMC_MODE_GAUSSIAN, 0u, static_cast<size_t>(n_periods) + 1u + n_bins, 1u);
}

struct PortfolioCashflowMarkovFamily {  // Gaussian mode only: its own ladder, exact | fast divide
  template <bool kExactDiv, int K>
  static WalkKernel<PortfolioCashflowMarkovArgs> schedule(const PortfolioCashflowMarkovArgs &x) {
    return x.c.schedule ? portfolio_cashflow_regimes_kernel<kExactDiv, K, true> : portfolio_cashflow_regimes_kernel<kExactDiv, K, false>;
  }
  template <bool kExactDiv>
  static WalkKernel<PortfolioCashflowMarkovArgs> get(const PortfolioCashflowMarkovArgs &x) {
    switch (x.p.n_assets) {
      case 1: return schedule<kExactDiv, 1>(x);
      case 2: return schedule<kExactDiv, 2>(x);
      case 3: return schedule<kExactDiv, 3>(x);
      default: return schedule<kExactDiv, 4>(x);
    }
  }
};
hipError_t launch_portfolio_cashflow_markov(const KernelArgs &a, const PortfolioCashflowMarkovArgs &x, bool exact_div, uint32_t grid,
                                            hipStream_t stream) {
  if (a.stream != 3 || a.mode != SMMC_MODE_GAUSSIAN || a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f) return hipErrorInvalidValue;
  if (x.p.n_assets < 1 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (x.leave_q16[0] > SMMC_REGIME_Q16_ONE || x.leave_q16[1] > SMMC_REGIME_Q16_ONE || x.start1_q16 > SMMC_REGIME_Q16_ONE)
    return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.c.schedule && (x.c.stride % 8u != 0u || x.c.stride < a.n_periods)) return hipErrorInvalidValue;
  const size_t lds = portfolio_cashflow_markov_lds_bytes(a.n_periods, a.n_bins);
  const WalkKernel<PortfolioCashflowMarkovArgs> kernel =
      exact_div ? PortfolioCashflowMarkovFamily::get<true>(x) : PortfolioCashflowMarkovFamily::get<false>(x);
  const hipError_t err = allow_lds(kernel, lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(wave_walk_group_paths(SMMC_MODE_GAUSSIAN)), lds, stream, a, x);
  return hipGetLastError();
}

// ---- portfolio cash-flow checkpoints ----

size_t portfolio_cashflow_checkpoints_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins,
                                                uint32_t n_checkpoints) {
  // the kernel's layout: [front: the padded rows or the draw tables, later the checkpoint partials [waves][n_checkpoints]]
  // [depletion [n_periods + 1]][final buckets [n_bins]][checkpoint buckets [n_checkpoints][n_bins]][pad to 8 bytes]
  // [one LaneRecord partial per wave]
  const bool table = mode == SMMC_MODE_TABLE;
  const uint32_t waves = walk_waves(table ? SMMC_MODE_TABLE : SMMC_MODE_GAUSSIAN);
  const uint32_t front = checkpoint_front_words(table ? n_rows * portfolio_row_words(n_assets) : bm_lds_words(SMMC_MODE_GAUSSIAN), waves, n_checkpoints);
  const size_t counters = static_cast<size_t>(n_periods) + 1u + n_bins + static_cast<size_t>(n_checkpoints) * n_bins;
  return ((front + counters + 1u) & ~static_cast<size_t>(1)) * 4u + waves * sizeof(BlockPartial);
}

struct PortfolioCashflowCheckpointsFamily {
  template <int kMode, bool kExactDiv, bool kDense, int K>
  static WalkKernel<PortfolioCashflowCheckpointsArgs> schedule(const PortfolioCashflowCheckpointsArgs &x) {
    return x.c.schedule ? portfolio_cashflow_checkpoints_kernel<kMode, kExactDiv, kDense, K, true>
                        : portfolio_cashflow_checkpoints_kernel<kMode, kExactDiv, kDense, K, false>;
  }
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<PortfolioCashflowCheckpointsArgs> get(const PortfolioCashflowCheckpointsArgs &x) {
    switch (x.p.n_assets) {
      case 1: return schedule<kMode, kExactDiv, kDense, 1>(x);
      case 2: return schedule<kMode, kExactDiv, kDense, 2>(x);
      case 3: return schedule<kMode, kExactDiv, kDense, 3>(x);
      default: return schedule<kMode, kExactDiv, kDense, 4>(x);
    }
  }
};
// The entries of x.periods from x.n on must be 0xffffffff.
hipError_t launch_portfolio_cashflow_checkpoints(const KernelArgs &a, const PortfolioCashflowCheckpointsArgs &x, bool exact_div, uint32_t grid,
                                                 hipStream_t stream) {
  if (a.stream != 3 || x.p.n_assets < 1 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.mode == SMMC_MODE_TABLE ? (!a.table_len || !a.table_a) : (a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f)) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.c.schedule && (x.c.stride % 8u != 0u || x.c.stride < a.n_periods)) return hipErrorInvalidValue;
  if (x.n < 1 || x.n > SMMC_MAX_CHECKPOINTS || !x.ck_partials) return hipErrorInvalidValue;
  if (static_cast<uint64_t>(x.n) * a.n_bins > SMMC_MAX_CHECKPOINT_BINS || (a.n_bins && !x.d_ck_hist)) return hipErrorInvalidValue;
  for (uint32_t i = 0; i < x.n; ++i)  // every record is of a period the walk reaches, in the order it reaches them
    if (x.periods[i] < 1 || x.periods[i] > a.n_periods || (i && x.periods[i] <= x.periods[i - 1])) return hipErrorInvalidValue;
  return launch_wave_walk<PortfolioCashflowCheckpointsFamily>(
      a, x, exact_div, grid, portfolio_cashflow_checkpoints_lds_bytes(a.mode, a.table_len, x.p.n_assets, a.n_periods, a.n_bins, x.n), stream);
}

// ---- real cash flows ----

struct RealCashflowFamily {
  template <int kMode, bool kExactDiv, bool kDense, int K>
  static WalkKernel<RealCashflowArgs> schedule(const RealCashflowArgs &x) {
    return x.c.schedule ? real_cashflow_kernel<kMode, kExactDiv, kDense, K, true> : real_cashflow_kernel<kMode, kExactDiv, kDense, K, false>;
  }
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<RealCashflowArgs> get(const RealCashflowArgs &x) {
    switch (x.p.n_assets) {  // the law's width: K invested assets and the inflation series
      case 2: return schedule<kMode, kExactDiv, kDense, 1>(x);
      case 3: return schedule<kMode, kExactDiv, kDense, 2>(x);
      default: return schedule<kMode, kExactDiv, kDense, 3>(x);
    }
  }
};
hipError_t launch_real_cashflow(const KernelArgs &a, const RealCashflowArgs &x, bool exact_div, uint32_t grid, hipStream_t stream) {
  if (a.stream != 3 || x.p.n_assets < 2 || x.p.n_assets > SMMC_MAX_ASSETS || x.p.weights[x.p.n_assets - 1] != 0.0f) return hipErrorInvalidValue;
  if (a.mode == SMMC_MODE_TABLE ? (!a.table_len || !a.table_a) : (a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f)) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.c.schedule && (x.c.stride % 8u != 0u || x.c.stride < a.n_periods)) return hipErrorInvalidValue;
  // LDS: the parent's layout with rows of the law's width
  return launch_wave_walk<RealCashflowFamily>(
      a, x, exact_div, grid, portfolio_cashflow_lds_bytes(a.mode, a.table_len, x.p.n_assets, a.n_periods, a.n_bins), stream);
}

// ---- guardrails ----

size_t guardrails_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins) {
  // the padded rows in the table's place; counters: depletion, cuts and raises [n_periods + 1] each, histogram [n_bins];
  // one partial per wave
  return wave_walk_lds_bytes(mode, n_rows * portfolio_row_words(n_assets), 3u * (static_cast<size_t>(n_periods) + 1u) + n_bins, 1u);
}

struct GuardrailsFamily {  // one divide, the IEEE one: both rungs of the ladder's divide are the same kernel
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<GuardrailsArgs> get(const GuardrailsArgs &x) {
    switch (x.p.n_assets) {
      case 1: return guardrails_kernel<kMode, kDense, 1>;
      case 2: return guardrails_kernel<kMode, kDense, 2>;
      case 3: return guardrails_kernel<kMode, kDense, 3>;
      default: return guardrails_kernel<kMode, kDense, 4>;
    }
  }
};
hipError_t launch_guardrails(const KernelArgs &a, const GuardrailsArgs &x, uint32_t grid, hipStream_t stream) {
  if (a.stream != 3 || x.p.n_assets < 1 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.mode == SMMC_MODE_TABLE ? (!a.table_len || !a.table_a) : (a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f)) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  return launch_wave_walk<GuardrailsFamily>(a, x, true, grid, guardrails_lds_bytes(a.mode, a.table_len, x.p.n_assets, a.n_periods, a.n_bins),
                                            stream);
}

// ---- glide paths ----

struct GlideFamily {  // K = 2, 3, 4: one asset is the parent's launch (csrc/smmc_glide.cpp)
  template <int kMode, bool kExactDiv, bool kDense, int K>
  static WalkKernel<GlideArgs> schedule(const GlideArgs &x) {
    return x.c.schedule ? glide_kernel<kMode, kExactDiv, kDense, K, true> : glide_kernel<kMode, kExactDiv, kDense, K, false>;
  }
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<GlideArgs> get(const GlideArgs &x) {
    switch (x.p.n_assets) {
      case 2: return schedule<kMode, kExactDiv, kDense, 2>(x);
      case 3: return schedule<kMode, kExactDiv, kDense, 3>(x);
      default: return schedule<kMode, kExactDiv, kDense, 4>(x);
    }
  }
};
hipError_t launch_glide(const KernelArgs &a, const GlideArgs &x, bool exact_div, uint32_t grid, hipStream_t stream) {
  if (a.stream != 3 || x.p.n_assets < 2 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.mode == SMMC_MODE_TABLE ? (!a.table_len || !a.table_a) : (a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f)) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.c.schedule && (x.c.stride % 8u != 0u || x.c.stride < a.n_periods)) return hipErrorInvalidValue;
  if (!x.table || reinterpret_cast<uintptr_t>(x.table) % sizeof(GlideEntry) != 0u || x.first > a.n_periods) return hipErrorInvalidValue;
  return launch_wave_walk<GlideFamily>(a, x, exact_div, grid,
                                       portfolio_cashflow_lds_bytes(a.mode, a.table_len, x.p.n_assets, a.n_periods, a.n_bins), stream);
}

// ---- allocation sweeps ----

size_t allocation_sweep_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins,
                                  uint32_t n_scenarios) {
  // the padded rows in the table's place; counters: per scenario depletion [n_periods + 1] and histogram [n_bins];
  // allocation_sweep_width(n_scenarios) partials per wave
  return wave_walk_lds_bytes(mode, n_rows * portfolio_row_words(n_assets),
                             static_cast<size_t>(n_scenarios) * (static_cast<size_t>(n_periods) + 1u + n_bins),
                             allocation_sweep_width(n_scenarios));
}

struct AllocationSweepFamily {
  template <int kMode, bool kExactDiv, bool kDense, int K>
  static WalkKernel<AllocationSweepArgs> width(const AllocationSweepArgs &x) {
    return allocation_sweep_width(x.n) == 4u ? allocation_sweep_kernel<kMode, kExactDiv, kDense, K, 4>
                                             : allocation_sweep_kernel<kMode, kExactDiv, kDense, K, 8>;
  }
  template <int kMode, bool kExactDiv, bool kDense>
  static WalkKernel<AllocationSweepArgs> get(const AllocationSweepArgs &x) {
    switch (x.p.n_assets) {
      case 1: return width<kMode, kExactDiv, kDense, 1>(x);
      case 2: return width<kMode, kExactDiv, kDense, 2>(x);
      case 3: return width<kMode, kExactDiv, kDense, 3>(x);
      default: return width<kMode, kExactDiv, kDense, 4>(x);
    }
  }
};
// The entries of x from x.n up to allocation_sweep_width(x.n) must be copies of entry x.n - 1.
hipError_t launch_allocation_sweep(const KernelArgs &a, const AllocationSweepArgs &x, bool exact_div, uint32_t grid, hipStream_t stream) {
  if (a.stream != 3 || x.p.n_assets < 1 || x.p.n_assets > SMMC_MAX_ASSETS) return hipErrorInvalidValue;
  if (a.mode == SMMC_MODE_TABLE ? (!a.table_len || !a.table_a) : (a.gauss_std != 1.0f || a.gauss_shift100 != 0.0f)) return hipErrorInvalidValue;
  if (a.n_periods == 0 || a.n_periods > SMMC_MAX_CASHFLOW_PERIODS) return hipErrorInvalidValue;
  if (x.n < 1 || x.n > SMMC_MAX_SWEEP) return hipErrorInvalidValue;
  if (static_cast<uint64_t>(x.n) * (static_cast<uint64_t>(a.n_periods) + 1u + a.n_bins) > SMMC_MAX_SWEEP_COUNTERS) return hipErrorInvalidValue;
  return launch_wave_walk<AllocationSweepFamily>(
      a, x, exact_div, grid, allocation_sweep_lds_bytes(a.mode, a.table_len, x.p.n_assets, a.n_periods, a.n_bins, x.n), stream);
}

}  // namespace smmc
