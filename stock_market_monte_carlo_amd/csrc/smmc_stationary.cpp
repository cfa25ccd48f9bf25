// smmc_stationary.cpp -- smmc_engine_simulate_stationary, its _to_host form and smmc_engine_stationary_divide_kind
// (include/smmc.h): table paths in runs of geometric length, the stationary bootstrap of Politis and Romano.
//
// A translation unit of its own, as smmc_blocks.cpp: it holds the LDS need and the three entries; the checks of `st`
// are stationary_check (smmc_host.h), shared with smmc_portfolio_cashflow_stationary.cpp.
// The run -- kernel arguments, grid, accumulator lease, divide, timed launch, fold -- is smmc_blocks.cpp's, lent through
// smmc_host.h (host_enqueue_paths) with launch_stationary as its kernel; the _to_host form is host_simulate_to_host
// around the same enqueue.  It keeps no state per engine.  The reference resamples single months
// (src/simulations.cpp:240-252); it has no run of consecutive months.
#include <hip/hip_runtime_api.h>

#include "smmc_host.h"
#include "smmc_internal.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

constexpr const char *kLdsHolds = "table and histogram";

int check_stationary(const smmc_engine *e, const smmc_sim *sim, const smmc_stationary *st) {
  const int rc = smmc::host_check_sim(e, sim);
  return rc ? rc : smmc::stationary_check(sim, st);
}

// What a launch for these outputs asks of LDS: one plain copy of the table and the histogram, if a record is wanted.
size_t lds_need(const smmc_engine *e, const smmc_sim *sim, bool record) {
  return smmc::stationary_lds_bytes(smmc::host_make_args(e, sim).table_len, record ? sim->n_bins : 0u);
}

// host_enqueue_paths with stationary_kernel.  Device must be current.
int enqueue_stationary(smmc_engine *e, const smmc_sim *s, const smmc_stationary *st, float *d_final, float *d_chunk_mean,
                       float *d_chunk_var, void *d_stats) {
  const smmc::PathLaunch w = {"launch_stationary",
                              [](const smmc::KernelArgs &a, int div, uint32_t grid, hipStream_t stream, const void *ctx) {
                                return smmc::launch_stationary(a, static_cast<const smmc_stationary *>(ctx)->renew_q16, div, grid, stream);
                              },
                              st, lds_need(e, s, d_stats != nullptr), kLdsHolds};
  return smmc::host_enqueue_paths(e, s, w, d_final, d_chunk_mean, d_chunk_var, d_stats);
}

}  // namespace

extern "C" {

int smmc_engine_simulate_stationary(smmc_engine *e, const smmc_sim *sim, const smmc_stationary *st, float *d_final, float *d_chunk_mean,
                                    float *d_chunk_var, void *d_stats) {
  const int rc = check_stationary(e, sim, st);
  if (rc) return rc;
  if (smmc::host_misaligned({d_final, d_chunk_mean, d_chunk_var}, 4))
    return host_fail(SMMC_ERR_INVALID, "d_final, d_chunk_mean and d_chunk_var must be 4-byte aligned");
  if (smmc::host_misaligned({d_stats}, 8)) return host_fail(SMMC_ERR_INVALID, "d_stats must be 8-byte aligned");
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  return enqueue_stationary(e, sim, st, d_final, d_chunk_mean, d_chunk_var, d_stats);
}

int smmc_engine_simulate_stationary_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_stationary *st, float *host_final,
                                            float *host_chunk_mean, float *host_chunk_var, volatile int64_t *progress, smmc_stats *stats,
                                            uint64_t *hist) {
  int rc = check_stationary(e, sim, st);
  if (rc) return rc;
  // refuse before the pipeline allocates anything
  rc = sim->n_paths ? smmc::host_check_lds(smmc::engine_view(e), lds_need(e, sim, stats || hist), kLdsHolds) : SMMC_OK;
  if (rc) return rc;
  return smmc::host_simulate_to_host(
      e, sim, host_final, host_chunk_mean, host_chunk_var, progress, stats, hist,
      [](smmc_engine *eng, const smmc_sim *part, float *d_final, float *d_cm, float *d_cv, void *d_rec, const void *ctx) {
        return enqueue_stationary(eng, part, static_cast<const smmc_stationary *>(ctx), d_final, d_cm, d_cv, d_rec);
      },
      st);
}

int smmc_engine_stationary_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_stationary *st) {
  int rc = check_stationary(e, sim, st);
  if (rc) return rc;
  // the table alone must fit: which outputs the call will ask for is not known here
  rc = sim->n_paths ? smmc::host_check_lds(smmc::engine_view(e), lds_need(e, sim, false), kLdsHolds) : SMMC_OK;
  if (rc) return rc;
  // the bounds on a product come from the table's extremes, the capital and n_periods, not from the order of the
  // draws: smmc_engine_divide_kind's proof as it is, the checked window included (tested once per 8 periods)
  float lo, hi;
  return smmc::host_divide_kind(e, sim, true, &lo, &hi);
}

}  // extern "C"
