// smmc_regimes.cpp -- smmc_engine_simulate_regimes, its _to_host form and smmc_engine_regimes_divide_kind
// (include/smmc.h): Gaussian paths under a two-state Markov law, Hamilton's regime-switching model.
//
// A translation unit of its own, as smmc_blocks.cpp: it holds the checks of `rg`, the divide rule on the union of the
// two regimes' bounds, and the three entries.  The run -- kernel arguments, grid, LDS refusal, accumulator lease, timed
// launch, fold -- is smmc_blocks.cpp's, lent through smmc_host.h (host_enqueue_paths) with launch_regimes as its kernel;
// the _to_host form is host_simulate_to_host around the same enqueue.  It keeps no state per engine.  The reference draws
// every period from one law (src/simulations.cpp:14-16); it has no hidden state.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "smmc_host.h"
#include "smmc_internal.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

constexpr const char *kLdsHolds = "draw tables and histogram";

// The sim the shared host code sees: gauss_mean and gauss_std of the caller's are not read, the staged draw yields
// standard normals (scale 1; the launch below takes the shift to 0).
smmc_sim plain_sim(const smmc_sim *sim) {
  smmc_sim plain = *sim;
  plain.gauss_mean = 0.0f;
  plain.gauss_std = 1.0f;
  return plain;
}

int check_regimes(const smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg) {
  if (!e) return host_fail(SMMC_ERR_INVALID, "engine is NULL");
  if (!sim) return host_fail(SMMC_ERR_INVALID, "sim is NULL");
  if (sim->struct_size != sizeof(smmc_sim))
    return host_fail(SMMC_ERR_INVALID, "smmc_sim.struct_size is %u, this library expects %zu", sim->struct_size, sizeof(smmc_sim));
  if (sim->mode != SMMC_MODE_GAUSSIAN)
    return host_fail(SMMC_ERR_INVALID, "regimes are a law of Gaussian returns: mode must be SMMC_MODE_GAUSSIAN (got %d)", sim->mode);
  int rc = smmc::host_require_v3(sim, "regimes support");
  if (rc) return rc;
  const smmc_sim plain = plain_sim(sim);
  rc = smmc::host_check_sim(e, &plain);
  if (rc) return rc;
  if (!rg) return host_fail(SMMC_ERR_INVALID, "the smmc_regimes argument is NULL");
  if (rg->struct_size != sizeof(smmc_regimes))
    return host_fail(SMMC_ERR_INVALID, "smmc_regimes.struct_size is %u, this library expects %zu", rg->struct_size, sizeof(smmc_regimes));
  for (int r = 0; r < 2; ++r) {
    if (!std::isfinite(rg->mean[r])) return host_fail(SMMC_ERR_INVALID, "mean[%d] is not finite", r);
    if (!std::isfinite(rg->std[r])) return host_fail(SMMC_ERR_INVALID, "std[%d] is not finite", r);
    if (rg->std[r] < 0.0f) return host_fail(SMMC_ERR_INVALID, "std[%d] is %g: a deviation is >= 0", r, static_cast<double>(rg->std[r]));
    if (rg->leave_q16[r] > SMMC_REGIME_Q16_ONE)
      return host_fail(SMMC_ERR_INVALID, "leave_q16[%d] is %u: the probability leave_q16 / 65536 is at most 1", r, rg->leave_q16[r]);
  }
  if (rg->start1_q16 > SMMC_REGIME_Q16_ONE)
    return host_fail(SMMC_ERR_INVALID, "start1_q16 is %u: the probability start1_q16 / 65536 is at most 1", rg->start1_q16);
  if (rg->reserved[0] != 0 || rg->reserved[1] != 0)
    return host_fail(SMMC_ERR_INVALID, "smmc_regimes.reserved is {%u, %u}, it must be 0", rg->reserved[0], rg->reserved[1]);
  return SMMC_OK;
}

// The rule of include/smmc.h (smmc_engine_regimes_divide_kind): smmc_engine_divide_kind's on the union of the two
// regimes' bounds, each regime's as one Gaussian asset's (smmc_portfolio.cpp, asset_bounds: the deviation rounded up).
int regimes_divide(const smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg, float *chk_lo, float *chk_hi) {
  *chk_lo = 0.0f;
  *chk_hi = 0.0f;
  double lo_a = INFINITY, hi_a = 0.0;
  for (int r = 0; r < 2; ++r) {
    smmc_sim one = *sim;
    one.gauss_mean = rg->mean[r];
    one.gauss_std = std::nextafter(rg->std[r], std::numeric_limits<float>::infinity());  // rounded up
    double lo, hi;
    if (!smmc::host_multiplier_bounds(e, &one, &lo, &hi)) return SMMC_DIV_EXACT;
    lo_a = std::min(lo_a, lo);
    hi_a = std::max(hi_a, hi);
  }
  return smmc::host_divide_kind_of_bounds(sim, lo_a, hi_a, true, chk_lo, chk_hi);
}

size_t lds_need(const smmc_sim *sim, bool record) { return smmc::regimes_lds_bytes(record ? sim->n_bins : 0u); }

struct Launch {  // what launch_regimes takes beside the kernel arguments of the plain sim
  smmc::RegimeArgs r;
  int div;
  float chk_lo, chk_hi;
};

// host_enqueue_paths with regimes_kernel.  Device must be current.
int enqueue_regimes(smmc_engine *e, const smmc_sim *s, const smmc_regimes *rg, float *d_final, float *d_chunk_mean, float *d_chunk_var,
                    void *d_stats) {
  Launch l;
  for (int r = 0; r < 2; ++r) {
    l.r.scale[r] = rg->std[r];
    l.r.shift100[r] = 100.0f + rg->mean[r];
    l.r.leave_q16[r] = rg->leave_q16[r];
  }
  l.r.start1_q16 = rg->start1_q16;
  l.div = regimes_divide(e, s, rg, &l.chk_lo, &l.chk_hi);
  const smmc_sim plain = plain_sim(s);
  const smmc::PathLaunch w = {"launch_regimes",
                              // the divide and the window the enqueue derives are the plain sim's: this law's own replace them
                              [](const smmc::KernelArgs &a, int, uint32_t grid, hipStream_t stream, const void *ctx) {
                                const Launch *l = static_cast<const Launch *>(ctx);
                                smmc::KernelArgs b = a;
                                b.gauss_shift100 = 0.0f;  // the staged draw yields standard normals: scale 1, shift 0
                                b.chk_lo = l->chk_lo;
                                b.chk_hi = l->chk_hi;
                                return smmc::launch_regimes(b, l->r, l->div, grid, stream);
                              },
                              &l, lds_need(s, d_stats != nullptr), kLdsHolds};
  return smmc::host_enqueue_paths(e, &plain, w, d_final, d_chunk_mean, d_chunk_var, d_stats);
}

}  // namespace

extern "C" {

int smmc_engine_simulate_regimes(smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg, float *d_final, float *d_chunk_mean,
                                 float *d_chunk_var, void *d_stats) {
  const int rc = check_regimes(e, sim, rg);
  if (rc) return rc;
  if (smmc::host_misaligned({d_final, d_chunk_mean, d_chunk_var}, 4))
    return host_fail(SMMC_ERR_INVALID, "d_final, d_chunk_mean and d_chunk_var must be 4-byte aligned");
  if (smmc::host_misaligned({d_stats}, 8)) return host_fail(SMMC_ERR_INVALID, "d_stats must be 8-byte aligned");
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  return enqueue_regimes(e, sim, rg, d_final, d_chunk_mean, d_chunk_var, d_stats);
}

int smmc_engine_simulate_regimes_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg, float *host_final,
                                         float *host_chunk_mean, float *host_chunk_var, volatile int64_t *progress, smmc_stats *stats,
                                         uint64_t *hist) {
  int rc = check_regimes(e, sim, rg);
  if (rc) return rc;
  // refuse before the pipeline allocates anything
  rc = sim->n_paths ? smmc::host_check_lds(smmc::engine_view(e), lds_need(sim, stats || hist), kLdsHolds) : SMMC_OK;
  if (rc) return rc;
  const smmc_sim plain = plain_sim(sim);
  return smmc::host_simulate_to_host(
      e, &plain, host_final, host_chunk_mean, host_chunk_var, progress, stats, hist,
      [](smmc_engine *eng, const smmc_sim *part, float *d_final, float *d_cm, float *d_cv, void *d_rec, const void *ctx) {
        return enqueue_regimes(eng, part, static_cast<const smmc_regimes *>(ctx), d_final, d_cm, d_cv, d_rec);
      },
      rg);
}

int smmc_engine_regimes_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg) {
  int rc = check_regimes(e, sim, rg);
  if (rc) return rc;
  // the draw tables alone must fit: which outputs the call will ask for is not known here
  rc = sim->n_paths ? smmc::host_check_lds(smmc::engine_view(e), lds_need(sim, false), kLdsHolds) : SMMC_OK;
  if (rc) return rc;
  float lo, hi;
  return regimes_divide(e, sim, rg, &lo, &hi);
}

}  // extern "C"
