// smmc_excursions.cpp -- smmc_engine_simulate_excursions and its _to_host form (include/smmc.h): drawdown, running
// extremes, time under water and the first passage of two levels, reduced along every path.
//
// A translation unit of its own, as smmc_cashflow.cpp: smmc_capi.cpp owns struct smmc_engine and never calls into
// this file; what is needed of an engine comes through smmc_host.h.  It keeps no state per engine: the two
// records use the halves of the engine's partial array, the four counter arrays the engine's zeroed accumulator.
// The launch is a wave walk, and its run is the shared one (smmc_host.h, host_wave_walk_run) with two records and two
// count arrays.  What is this unit's own: the argument checks, the launch shape and LDS need, how the accumulator is
// divided, the kernel arguments, and the keepdata divide rule asked before the device is touched.
// The reference draws the MINIMUM and TARGET levels across its trajectory plot
// (examples/visualize_returns_cpu_v2.cpp:397-411) and counts final values below the minimum (:125-138); what
// happened along a path it can only read off the stored trajectories.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "smmc_host.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as cashflow_kernel: a workgroup flushes 2 (n_periods + 1) + 2 n_bins counters.
constexpr uint32_t kExcursionGroupsPerCU = 32;
// The engine's accumulator (kHistSpread x SMMC_MAX_BINS counters, zero between launches) as this launch divides it:
// the histogram of the final values, the histogram of the drawdowns, the first_below and the first_reach counts.
constexpr size_t kAccDrawdownHist = SMMC_MAX_BINS;
constexpr size_t kAccBelowAt = 2u * SMMC_MAX_BINS;
constexpr size_t kAccReachAt = kAccBelowAt + SMMC_MAX_EXCURSION_PERIODS + 1u;
static_assert(kAccReachAt + SMMC_MAX_EXCURSION_PERIODS + 1u <= static_cast<size_t>(smmc::kHistSpread) * SMMC_MAX_BINS,
              "the engine's accumulator holds two histograms and two first-passage count arrays");

int check_excursions(const smmc_engine *e, const smmc_sim *sim, const smmc_excursions *x, const smmc_excursion_outputs *out) {
  int rc = smmc::host_check_sim(e, sim);
  if (rc) return rc;
  if (!x) return host_fail(SMMC_ERR_INVALID, "the smmc_excursions argument is NULL");
  if (x->struct_size != sizeof(smmc_excursions))
    return host_fail(SMMC_ERR_INVALID, "smmc_excursions.struct_size is %u, this library expects %zu", x->struct_size,
                     sizeof(smmc_excursions));
  if (!out) return host_fail(SMMC_ERR_INVALID, "the smmc_excursion_outputs argument is NULL");
  if (out->struct_size != sizeof(smmc_excursion_outputs))
    return host_fail(SMMC_ERR_INVALID, "smmc_excursion_outputs.struct_size is %u, this library expects %zu", out->struct_size,
                     sizeof(smmc_excursion_outputs));
  rc = smmc::host_require_v3(sim, "excursions support");
  if (rc) return rc;
  if (sim->n_periods == 0) return host_fail(SMMC_ERR_INVALID, "n_periods is 0: an excursion needs at least one period");
  if (sim->n_periods > SMMC_MAX_EXCURSION_PERIODS)
    return host_fail(SMMC_ERR_INVALID, "n_periods %u exceeds SMMC_MAX_EXCURSION_PERIODS %d", sim->n_periods,
                     SMMC_MAX_EXCURSION_PERIODS);
  if (std::isnan(x->lower)) return host_fail(SMMC_ERR_INVALID, "lower is NaN (-inf means never below)");
  if (std::isnan(x->target)) return host_fail(SMMC_ERR_INVALID, "target is NaN (+inf means never reached)");
  if (std::isnan(x->drawdown_threshold)) return host_fail(SMMC_ERR_INVALID, "drawdown_threshold is NaN");
  return SMMC_OK;
}

int check_alignment(const smmc_excursion_outputs *o) {
  if (smmc::host_misaligned({o->final, o->peak, o->low, o->drawdown, o->drawdown_period, o->underwater, o->first_below, o->first_reach}, 4))
    return host_fail(SMMC_ERR_INVALID, "the per-path output pointers must be 4-byte aligned");
  if (smmc::host_misaligned({o->stats, o->drawdown_stats, o->first_below_at, o->first_reach_at}, 8))
    return host_fail(SMMC_ERR_INVALID, "the record and count-array pointers must be 8-byte aligned");
  return SMMC_OK;
}

// The launch shape of a request, and the refusals that follow from it; both entries ask before any device work.
struct Geometry {
  uint32_t grid, half;  // workgroups; where the second record's partials start in the engine's partial array
  uint32_t n_bins;      // of the launch: 0 when no record is asked for
};
int plan(const smmc_engine *e, const smmc::EngineView &view, const smmc_sim *sim, const smmc_excursion_outputs *out, Geometry *g) {
  // two records leave two partials per workgroup: the halves of the engine's partial array
  g->half = view.max_grid / 2u;
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kExcursionGroupsPerCU, g->half,
                                           &g->grid);
  if (sim->n_paths && !g->grid) return host_fail(SMMC_ERR_INVALID, "the engine's launch grid is too small for two records");
  if (rc) return rc;
  g->n_bins = (out->stats || out->drawdown_stats) ? sim->n_bins : 0u;
  const smmc::KernelArgs a = smmc::host_make_args(e, sim);
  const size_t lds = smmc::excursions_lds_bytes(a.mode, a.table_len, a.n_periods, g->n_bins);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "table, first-passage counters and histograms need %zu bytes of LDS, device allows %zu", lds,
                     view.max_lds);
  return SMMC_OK;
}

}  // namespace

extern "C" {

int smmc_engine_simulate_excursions(smmc_engine *e, const smmc_sim *sim, const smmc_excursions *x,
                                    const smmc_excursion_outputs *out) {
  int rc = check_excursions(e, sim, x, out);
  if (rc) return rc;
  rc = check_alignment(out);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  Geometry g;
  rc = plan(e, view, sim, out, &g);
  if (rc) return rc;
  const uint32_t grid = g.grid, half = g.half;
  smmc::KernelArgs a = smmc::host_make_args(e, sim);
  a.n_bins = g.n_bins;
  // a value has to be right when it is looked at: the keepdata rule (never SMMC_DIV_CHECKED)
  const int div = smmc_engine_divide_kind(e, sim, 1);
  if (div < 0) return div;
  smmc::ExcursionArgs xa;
  std::memset(&xa, 0, sizeof xa);
  xa.lower = x->lower;
  xa.target = x->target;
  xa.drawdown_threshold = x->drawdown_threshold;
  xa.dd_hist_inv = static_cast<double>(a.n_bins);  // n_bins / (1 - 0)
  xa.d_peak = out->peak;
  xa.d_low = out->low;
  xa.d_drawdown = out->drawdown;
  xa.d_drawdown_period = out->drawdown_period;
  xa.d_underwater = out->underwater;
  xa.d_first_below = out->first_below;
  xa.d_first_reach = out->first_reach;
  a.d_final = out->final;
  const uint32_t n_counts = sim->n_periods + 1u;
  const smmc::WaveWalk walk = {"launch_excursions", grid, sim->n_bins,
                               {{out->stats, 0, 0, &a.partials, &a.d_hist},
                                {out->drawdown_stats, half, kAccDrawdownHist, &xa.dd_partials, &xa.d_dd_hist}},
                               {{out->first_below_at, kAccBelowAt, n_counts, &xa.d_below_at},
                                {out->first_reach_at, kAccReachAt, n_counts, &xa.d_reach_at}}};
  return smmc::host_wave_walk_run(e, walk, smmc::FoldRecord(), [&](hipStream_t stream) {
    return smmc::launch_excursions(a, xa, div != SMMC_DIV_FAST, grid, stream);
  });
}

int smmc_engine_simulate_excursions_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_excursions *x,
                                            const smmc_excursion_outputs *out) {
  int rc = check_excursions(e, sim, x, out);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  Geometry g;
  rc = plan(e, view, sim, out, &g);
  if (rc) return rc;
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  typedef smmc_excursion_outputs O;
  const size_t stats_bytes = static_cast<size_t>(smmc_stats_bytes(sim->n_bins));
  const size_t at_bytes = sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u);
  const size_t per_path = sizeof(float) * sim->n_paths;
  const smmc::OutputField fields[12] = {
      {offsetof(O, stats), stats_bytes},        {offsetof(O, drawdown_stats), stats_bytes}, {offsetof(O, first_below_at), at_bytes},
      {offsetof(O, first_reach_at), at_bytes},  {offsetof(O, final), per_path},             {offsetof(O, peak), per_path},
      {offsetof(O, low), per_path},             {offsetof(O, drawdown), per_path},          {offsetof(O, drawdown_period), per_path},
      {offsetof(O, underwater), per_path},      {offsetof(O, first_below), per_path},       {offsetof(O, first_reach), per_path}};
  return smmc::host_outputs_struct_to_host(e, "simulate_excursions_to_host", *out, fields,
                                           [&](const O *d) { return smmc_engine_simulate_excursions(e, sim, x, d); });
}

}  // extern "C"
