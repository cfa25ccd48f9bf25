// smmc_blocks.cpp -- smmc_engine_simulate_blocks, its _to_host form and smmc_engine_blocks_divide_kind
// (include/smmc.h): table paths drawn in runs of consecutive months, the circular block bootstrap.
//
// A translation unit of its own, as smmc_cashflow.cpp and smmc_excursions.cpp: smmc_capi.cpp owns struct smmc_engine
// and never calls into this file; what is needed of an engine comes through smmc_host.h.  It keeps no state per
// engine: the partials and the bucket accumulator are the engine's, used as smmc_engine_simulate uses them; the
// stream refusal, the timed launch and the HIP check are the shared host_require_v3, host_timed_launch and SMMC_HIP.
// The reference resamples single months (src/simulations.cpp:240-252); it has no block draw.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "smmc_host.h"
#include "smmc_internal.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

int check_blocks(const smmc_engine *e, const smmc_sim *sim, const smmc_blocks *b) {
  const int rc = smmc::host_check_sim(e, sim);
  return rc ? rc : smmc::blocks_check(sim, b);
}

constexpr size_t kLdsPerCU = 160u * 1024u;  // CDNA4
constexpr const char *kLdsHolds = "table, its circular extension and the histogram";

// The LDS layout of a request; asked before any device work.
struct Plan {
  bool wide;
  size_t lds;
};
int plan(const smmc::EngineView &view, const smmc::KernelArgs &a, uint32_t n_bins, Plan *p) {
  // The four shifted copies (16-byte reads) while eight workgroups per CU -- eight waves per SIMD -- still fit beside
  // each other; larger tables keep one copy and the 4-byte reads.  SMMC_BLOCKS_READ=b32 | b128 asks for one form (the
  // measurements of profiles/blocks/ are taken that way); b128 still yields where the copies do not fit at all.
  const size_t wide = smmc::blocks_lds_bytes(a.table_len, n_bins, true), narrow = smmc::blocks_lds_bytes(a.table_len, n_bins, false);
  p->wide = 8u * wide <= kLdsPerCU;
  if (const char *env = std::getenv("SMMC_BLOCKS_READ")) {
    if (!std::strcmp(env, "b32")) p->wide = false;
    else if (!std::strcmp(env, "b128")) p->wide = wide + 2048 <= view.max_lds;
    else if (*env) return host_fail(SMMC_ERR_INVALID, "SMMC_BLOCKS_READ is '%s': b32 or b128", env);
  }
  p->lds = p->wide ? wide : narrow;
  return SMMC_OK;  // whether it fits: host_check_lds, in host_enqueue_paths and before the _to_host pipeline
}

struct Launch {  // what launch_blocks takes beside the kernel arguments
  uint32_t block_len;
  bool wide;
};

// host_enqueue_paths with blocks_kernel.  Device must be current.
int enqueue_blocks(smmc_engine *e, const smmc_sim *s, const smmc_blocks *b, float *d_final, float *d_chunk_mean, float *d_chunk_var,
                   void *d_stats) {
  Plan p = {false, 0};
  const int rc = s->n_paths ? plan(smmc::engine_view(e), smmc::host_make_args(e, s), d_stats ? s->n_bins : 0u, &p) : SMMC_OK;
  if (rc) return rc;
  const Launch l = {b->block_len, p.wide};
  const smmc::PathLaunch w = {"launch_blocks",
                              [](const smmc::KernelArgs &a, int div, uint32_t grid, hipStream_t stream, const void *ctx) {
                                const Launch *l = static_cast<const Launch *>(ctx);
                                return smmc::launch_blocks(a, l->block_len, l->wide, div, grid, stream);
                              },
                              &l, p.lds, kLdsHolds};
  return smmc::host_enqueue_paths(e, s, w, d_final, d_chunk_mean, d_chunk_var, d_stats);
}

}  // namespace

// The enqueue this unit lends (smmc_host.h, "lend"): every statement around the launch of a path kernel, once.
int smmc::host_enqueue_paths(smmc_engine *e, const smmc_sim *s, const PathLaunch &w, float *d_final, float *d_chunk_mean,
                             float *d_chunk_var, void *d_stats) {
  const EngineView view = engine_view(e);
  KernelArgs a = host_make_args(e, s);
  a.d_final = d_final;
  a.d_chunk_mean = d_chunk_mean;
  a.d_chunk_var = d_chunk_var;
  const uint64_t n_chunks = (s->n_paths + kBlock - 1) / kBlock;
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(n_chunks, view.max_grid));
  int rc = grid ? host_check_lds(view, w.lds, w.lds_holds) : SMMC_OK;  // nothing is launched for n_paths == 0
  if (rc) return rc;
  ZeroLease lease;
  if (d_stats) {  // no memset: finalize_kernel writes the whole record and leaves the accumulator zero again
    a.partials = view.d_partials;
    if (s->n_bins) {
      rc = engine_acc_lease(e, &lease);
      if (rc) return rc;
      a.d_hist = lease.acc();
    }
  }
  a.clock_probe = view.clock_probe;
  if (grid > 0) {
    const int div = host_divide_kind(e, s, true, &a.chk_lo, &a.chk_hi);
    rc = host_timed_launch(e, w.name, [&] { return w.launch(a, div, grid, view.stream, w.ctx); });
    if (rc) return rc;
  }
  if (d_stats) {
    SMMC_HIP(launch_finalize(view.d_partials, grid, static_cast<smmc_stats *>(d_stats), s->n_bins, view.stream, lease.acc(),
                             s->n_bins ? 1u : 0u));
    lease.finalize_queued();
  }
  return SMMC_OK;
}

// What this unit refuses about `blocks`, the mode and the stream of a checked sim (smmc_host.h, "lend").
int smmc::blocks_check(const smmc_sim *sim, const smmc_blocks *b) {
  if (!b) return host_fail(SMMC_ERR_INVALID, "the smmc_blocks argument is NULL");
  if (b->struct_size != sizeof(smmc_blocks))
    return host_fail(SMMC_ERR_INVALID, "smmc_blocks.struct_size is %u, this library expects %zu", b->struct_size, sizeof(smmc_blocks));
  if (sim->mode != SMMC_MODE_TABLE)
    return host_fail(SMMC_ERR_INVALID, "the block bootstrap resamples the returns table: mode must be SMMC_MODE_TABLE (got %d)", sim->mode);
  const int rc = smmc::host_require_v3(sim, "the block bootstrap supports");
  if (rc) return rc;
  if (b->block_len == 0) return host_fail(SMMC_ERR_INVALID, "block_len is 0: a block holds at least one period");
  if (b->kind != SMMC_BLOCKS_CIRCULAR)
    return host_fail(SMMC_ERR_INVALID, "smmc_blocks.kind is %u: SMMC_BLOCKS_CIRCULAR (0) is the only kind", b->kind);
  if (b->reserved != 0) return host_fail(SMMC_ERR_INVALID, "smmc_blocks.reserved is %u, it must be 0", b->reserved);
  return SMMC_OK;
}

extern "C" {

int smmc_engine_simulate_blocks(smmc_engine *e, const smmc_sim *sim, const smmc_blocks *blocks, float *d_final, float *d_chunk_mean,
                                float *d_chunk_var, void *d_stats) {
  int rc = check_blocks(e, sim, blocks);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(d_final) | reinterpret_cast<uintptr_t>(d_chunk_mean) | reinterpret_cast<uintptr_t>(d_chunk_var)) & 3u)
    return host_fail(SMMC_ERR_INVALID, "d_final, d_chunk_mean and d_chunk_var must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_stats) & 7u) return host_fail(SMMC_ERR_INVALID, "d_stats must be 8-byte aligned");
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  return enqueue_blocks(e, sim, blocks, d_final, d_chunk_mean, d_chunk_var, d_stats);
}

int smmc_engine_simulate_blocks_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_blocks *blocks, float *host_final,
                                        float *host_chunk_mean, float *host_chunk_var, volatile int64_t *progress, smmc_stats *stats,
                                        uint64_t *hist) {
  int rc = check_blocks(e, sim, blocks);
  if (rc) return rc;
  Plan p;  // refuse before the pipeline allocates anything
  rc = sim->n_paths ? plan(smmc::engine_view(e), smmc::host_make_args(e, sim), (stats || hist) ? sim->n_bins : 0u, &p) : SMMC_OK;
  if (!rc && sim->n_paths) rc = smmc::host_check_lds(smmc::engine_view(e), p.lds, kLdsHolds);
  if (rc) return rc;
  return smmc::host_simulate_to_host(
      e, sim, host_final, host_chunk_mean, host_chunk_var, progress, stats, hist,
      [](smmc_engine *eng, const smmc_sim *part, float *d_final, float *d_cm, float *d_cv, void *d_rec, const void *ctx) {
        return enqueue_blocks(eng, part, static_cast<const smmc_blocks *>(ctx), d_final, d_cm, d_cv, d_rec);
      },
      blocks);
}

int smmc_engine_blocks_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_blocks *blocks) {
  const int rc = check_blocks(e, sim, blocks);
  if (rc) return rc;
  // the bounds on a product come from the table's extremes, the capital and n_periods, not from the order of the
  // draws: smmc_engine_divide_kind's proof as it is, the checked window included
  float lo, hi;
  return smmc::host_divide_kind(e, sim, true, &lo, &hi);
}

}  // extern "C"
