// smmc_sweep.cpp -- smmc_engine_simulate_cashflow_sweep and its siblings (include/smmc.h): up to SMMC_MAX_SWEEP
// constant cash-flow schedules stepped on the same paths in one launch.
//
// A translation unit of its own, like smmc_cashflow.cpp: smmc_capi.cpp and smmc_cashflow.cpp never call into this
// file.  A scenario's argument checks and its divide are smmc_engine_cashflow_divide_kind's -- the rule is stated
// once, in smmc_cashflow.cpp -- and the launch is a wave walk whose run is the shared one (smmc_host.h,
// host_wave_walk_run, with the per-scenario fold).  What is this unit's own: the checks across scenarios, the counter
// cap, the padding to the kernel's widths, the LDS need and the kernel arguments.  The scenarios travel as kernel
// arguments: nothing is staged, the unit keeps no state per engine.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>

#include "smmc_host.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as cashflow_kernel; a workgroup leaves one partial per scenario in the engine's max_grid
// partials, so the grid is capped at max_grid / sweep_width as well.
constexpr uint32_t kSweepGroupsPerCU = 32;
// The checks that need no output pointer; *kind: SMMC_DIV_FAST iff every scenario's own rule says so.
int check_sweep(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *scenarios, uint32_t n_scenarios, int *kind) {
  int rc = smmc::host_check_sim(e, sim);
  if (rc) return rc;
  if (!scenarios) return host_fail(SMMC_ERR_INVALID, "scenarios is NULL");
  if (n_scenarios == 0) return host_fail(SMMC_ERR_INVALID, "n_scenarios is 0");
  if (n_scenarios > SMMC_MAX_SWEEP)
    return host_fail(SMMC_ERR_INVALID, "n_scenarios %u exceeds SMMC_MAX_SWEEP %d", n_scenarios, SMMC_MAX_SWEEP);
  *kind = SMMC_DIV_FAST;
  for (uint32_t s = 0; s < n_scenarios; ++s) {
    const smmc_cashflow &cf = scenarios[s];
    if (cf.struct_size == sizeof(smmc_cashflow) && (cf.amounts || cf.fractions))
      return host_fail(SMMC_ERR_INVALID, "scenarios[%u] has per-period arrays: a sweep takes constant schedules (amount, fraction, floor)", s);
    const int one = smmc_engine_cashflow_divide_kind(e, sim, &cf);  // its checks, then its rule
    if (one < 0) return one;
    if (one != SMMC_DIV_FAST) *kind = SMMC_DIV_EXACT;
  }
  return SMMC_OK;
}

int check_counters(const smmc_sim *sim, uint32_t n_scenarios, bool want_stats) {
  const uint64_t per = static_cast<uint64_t>(sim->n_periods) + 1u + (want_stats ? sim->n_bins : 0u);
  if (n_scenarios * per > SMMC_MAX_SWEEP_COUNTERS)
    return host_fail(SMMC_ERR_INVALID, "n_scenarios * (n_periods + 1 + n_bins) = %u * %llu exceeds SMMC_MAX_SWEEP_COUNTERS %d",
                     n_scenarios, static_cast<unsigned long long>(per), SMMC_MAX_SWEEP_COUNTERS);
  return SMMC_OK;
}

}  // namespace

extern "C" {

int smmc_engine_cashflow_sweep_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *scenarios, uint32_t n_scenarios) {
  int kind = SMMC_DIV_EXACT;
  const int rc = check_sweep(e, sim, scenarios, n_scenarios, &kind);
  return rc ? rc : kind;
}

int smmc_engine_simulate_cashflow_sweep(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *scenarios, uint32_t n_scenarios,
                                        float *d_final, float *d_paid, uint32_t *d_ruin_period, void *d_stats,
                                        uint64_t *d_depleted_at) {
  int kind = SMMC_DIV_EXACT;
  int rc = check_sweep(e, sim, scenarios, n_scenarios, &kind);
  if (rc) return rc;
  rc = check_counters(sim, n_scenarios, d_stats != nullptr);
  if (rc) return rc;
  rc = smmc::cashflow_check_pointers(d_final, d_paid, d_ruin_period, d_stats, d_depleted_at);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  const uint32_t width = smmc::sweep_width(n_scenarios);
  if (view.max_grid < width) return host_fail(SMMC_ERR_INVALID, "the engine's grid of %u workgroups is too small for a sweep", view.max_grid);
  uint32_t grid = 0;
  rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kSweepGroupsPerCU, view.max_grid / width, &grid);
  if (rc) return rc;
  smmc::KernelArgs a = smmc::host_make_args(e, sim);
  if (!d_stats) a.n_bins = 0;
  const size_t lds = smmc::cashflow_sweep_lds_bytes(a.mode, a.table_len, a.n_periods, a.n_bins, n_scenarios);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "table, the scenarios' depletion counters and histograms need %zu bytes of LDS, device allows %zu",
                     lds, view.max_lds);
  smmc::SweepArgs c;
  std::memset(&c, 0, sizeof c);
  c.n = n_scenarios;
  for (uint32_t s = 0; s < SMMC_MAX_SWEEP; ++s) {  // beyond the request: copies of its last scenario
    const smmc_cashflow &cf = scenarios[std::min(s, n_scenarios - 1u)];
    c.amount[s] = cf.amount;
    c.fraction[s] = cf.fraction;
    c.floor[s] = cf.floor;
  }
  c.d_paid = d_paid;
  c.d_ruin_period = d_ruin_period;
  a.d_final = d_final;
  const bool exact_div = kind != SMMC_DIV_FAST;
  // a.partials: [scenario][grid]
  const smmc::WaveWalk walk = {"launch_cashflow_sweep", grid, sim->n_bins, {{d_stats, 0, 0, &a.partials, &a.d_hist}},
                               {{d_depleted_at, smmc::kSweepDepletedAt, n_scenarios * (sim->n_periods + 1u), &c.d_depleted}}};
  return smmc::host_wave_walk_run(e, walk, smmc::FoldScenarios{n_scenarios},
                                  [&](hipStream_t stream) { return smmc::launch_cashflow_sweep(a, c, exact_div, grid, stream); });
}

int smmc_engine_simulate_cashflow_sweep_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *scenarios,
                                                uint32_t n_scenarios, float *host_final, float *host_paid,
                                                uint32_t *host_ruin_period, void *host_stats, uint64_t *host_depleted_at) {
  int kind = SMMC_DIV_EXACT;
  int rc = check_sweep(e, sim, scenarios, n_scenarios, &kind);
  if (rc) return rc;
  rc = check_counters(sim, n_scenarios, host_stats != nullptr);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  const size_t per_path = sizeof(float) * sim->n_paths * n_scenarios;
  const smmc::HostPiece pieces[5] = {{host_stats, static_cast<size_t>(smmc_stats_bytes(sim->n_bins)) * n_scenarios},
                                     {host_depleted_at, sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u) * n_scenarios},
                                     {host_final, per_path}, {host_paid, per_path}, {host_ruin_period, per_path}};
  return smmc::host_outputs_to_host(e, "simulate_cashflow_sweep_to_host", pieces, 5, [&](void *const *dev) {
    return smmc_engine_simulate_cashflow_sweep(e, sim, scenarios, n_scenarios, static_cast<float *>(dev[2]), static_cast<float *>(dev[3]),
                                               static_cast<uint32_t *>(dev[4]), dev[0], static_cast<uint64_t *>(dev[1]));
  });
}

}  // extern "C"
