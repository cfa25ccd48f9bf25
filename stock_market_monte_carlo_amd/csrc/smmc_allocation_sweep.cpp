// smmc_allocation_sweep.cpp -- smmc_engine_simulate_allocation_sweep, its _to_host form and
// smmc_engine_allocation_sweep_divide_kind (include/smmc.h): up to SMMC_MAX_SWEEP portfolio strategies -- weights,
// rebalancing, a constant cash flow and a floor each -- stepped on the same jointly drawn paths in one launch.
//
// A translation unit of its own, like smmc_sweep.cpp and smmc_portfolio_cashflow.cpp: no other unit calls into this
// file.  A scenario's argument checks are lent by smmc_portfolio.cpp and smmc_cashflow.cpp (smmc_host.h, "lend"),
// its divide is smmc_engine_portfolio_cashflow_divide_kind's, asked scenario by scenario -- the rule and its proof stay
// in smmc_portfolio_cashflow.cpp.  What is this unit's own: the checks across scenarios (one joint law, constant
// schedules), the padding to the kernel's widths, the counter cap, the LDS need and the kernel arguments.  The launch is
// a wave walk and its run the shared one (smmc_host.h, host_wave_walk_run, with the per-scenario fold); the scenarios
// travel as kernel arguments: nothing is staged, the unit keeps no state per engine.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "smmc_host.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as cashflow_sweep_kernel; a workgroup leaves one partial per scenario in the engine's max_grid
// partials, so the grid is capped at max_grid / width as well.
constexpr uint32_t kGroupsPerCU = 32;

// The checks that need no output structure; *kind: SMMC_DIV_FAST iff every scenario's own rule says so.
int check_scenarios(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs, const smmc_cashflow *cfs, uint32_t n_scenarios,
                    int *kind) {
  int rc = SMMC_OK;  // (e and sim are portfolio_check's to judge: a portfolio needs no single-series table)
  if (!pfs) return host_fail(SMMC_ERR_INVALID, "pfs is NULL");
  if (!cfs) return host_fail(SMMC_ERR_INVALID, "cfs is NULL");
  if (n_scenarios == 0) return host_fail(SMMC_ERR_INVALID, "n_scenarios is 0");
  if (n_scenarios > SMMC_MAX_SWEEP)
    return host_fail(SMMC_ERR_INVALID, "n_scenarios %u exceeds SMMC_MAX_SWEEP %d", n_scenarios, SMMC_MAX_SWEEP);
  *kind = SMMC_DIV_FAST;
  for (uint32_t s = 0; s < n_scenarios; ++s) {
    const smmc_portfolio &pf = pfs[s];
    const smmc_cashflow &cf = cfs[s];
    rc = smmc::portfolio_check(e, sim, &pf);
    if (!rc) rc = smmc::cashflow_check_schedule(sim, &cf);
    if (rc) return rc;
    if (cf.amounts || cf.fractions)
      return host_fail(SMMC_ERR_INVALID, "cfs[%u] has per-period arrays: a sweep takes constant schedules (amount, fraction, floor)", s);
    if (pf.n_assets != pfs[0].n_assets)
      return host_fail(SMMC_ERR_INVALID, "pfs[%u].n_assets is %u, pfs[0].n_assets is %u: the scenarios of a sweep share one joint law", s,
                       pf.n_assets, pfs[0].n_assets);
    if (std::memcmp(pf.means, pfs[0].means, sizeof pf.means) != 0)
      return host_fail(SMMC_ERR_INVALID, "pfs[%u].means differs from pfs[0].means: the scenarios of a sweep share one joint law", s);
    if (std::memcmp(pf.factor, pfs[0].factor, sizeof pf.factor) != 0)
      return host_fail(SMMC_ERR_INVALID, "pfs[%u].factor differs from pfs[0].factor: the scenarios of a sweep share one joint law", s);
    const int one = smmc_engine_portfolio_cashflow_divide_kind(e, sim, &pf, &cf);  // the rule of smmc_portfolio_cashflow.cpp
    if (one < 0) return one;
    if (one != SMMC_DIV_FAST) *kind = SMMC_DIV_EXACT;
  }
  return SMMC_OK;
}

// The launch's arguments, grid and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::AllocationSweepArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs, const smmc_cashflow *cfs, uint32_t n_scenarios,
         bool want_stats, Plan *out) {
  const uint64_t per = static_cast<uint64_t>(sim->n_periods) + 1u + (want_stats ? sim->n_bins : 0u);
  if (n_scenarios * per > SMMC_MAX_SWEEP_COUNTERS)
    return host_fail(SMMC_ERR_INVALID, "n_scenarios * (n_periods + 1 + n_bins) = %u * %llu exceeds SMMC_MAX_SWEEP_COUNTERS %d",
                     n_scenarios, static_cast<unsigned long long>(per), SMMC_MAX_SWEEP_COUNTERS);
  const smmc::EngineView view = smmc::engine_view(e);
  const uint32_t width = smmc::allocation_sweep_width(n_scenarios);
  if (view.max_grid < width) return host_fail(SMMC_ERR_INVALID, "the engine's grid of %u workgroups is too small for a sweep", view.max_grid);
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kGroupsPerCU, view.max_grid / width,
                                           &out->grid);
  if (rc) return rc;
  smmc::AllocationSweepArgs &x = out->x;
  std::memset(&x, 0, sizeof x);
  smmc::portfolio_launch_args(e, sim, &pfs[0], &out->a, &x.p);  // the shared law; weights and R follow per scenario
  if (!want_stats) out->a.n_bins = 0;
  x.n = n_scenarios;
  for (uint32_t s = 0; s < SMMC_MAX_SWEEP; ++s) {  // beyond the request: copies of its last scenario
    const uint32_t from = std::min(s, n_scenarios - 1u);
    std::memcpy(x.weights[s], pfs[from].weights, sizeof x.weights[s]);
    x.rebalance_every[s] = pfs[from].rebalance_every;
    x.amount[s] = cfs[from].amount;
    x.fraction[s] = cfs[from].fraction;
    x.floor[s] = cfs[from].floor;
  }
  const size_t lds = smmc::allocation_sweep_lds_bytes(out->a.mode, out->a.table_len, pfs[0].n_assets, sim->n_periods, out->a.n_bins, n_scenarios);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "asset table, the scenarios' depletion counters, histograms and partials need %zu bytes of LDS, device allows %zu",
                     lds, view.max_lds);
  return SMMC_OK;
}

}  // namespace

extern "C" {

int smmc_engine_allocation_sweep_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs, const smmc_cashflow *cfs,
                                             uint32_t n_scenarios) {
  int kind = SMMC_DIV_EXACT;
  const int rc = check_scenarios(e, sim, pfs, cfs, n_scenarios, &kind);
  return rc ? rc : kind;
}

int smmc_engine_simulate_allocation_sweep(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs, const smmc_cashflow *cfs,
                                          uint32_t n_scenarios, const smmc_allocation_sweep_outputs *out) {
  int kind = SMMC_DIV_EXACT;
  int rc = check_scenarios(e, sim, pfs, cfs, n_scenarios, &kind);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_allocation_sweep_outputs");
  if (rc) return rc;
  rc = smmc::host_check_depletion_alignment(out);
  if (rc) return rc;
  Plan pl;
  rc = plan(e, sim, pfs, cfs, n_scenarios, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  smmc::AllocationSweepArgs &x = pl.x;
  pl.a.d_final = out->d_final;
  x.p.d_holdings = out->d_holdings;
  x.d_paid = out->d_paid;
  x.d_ruin_period = out->d_ruin_period;
  const bool exact_div = kind != SMMC_DIV_FAST;
  // pl.a.partials: [scenario][grid]
  const smmc::WaveWalk walk = {"launch_allocation_sweep", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kSweepDepletedAt, n_scenarios * (sim->n_periods + 1u), &x.d_depleted}}};
  return smmc::host_wave_walk_run(e, walk, smmc::FoldScenarios{n_scenarios}, [&](hipStream_t stream) {
    return smmc::launch_allocation_sweep(pl.a, x, exact_div, pl.grid, stream);
  });
}

int smmc_engine_simulate_allocation_sweep_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs, const smmc_cashflow *cfs,
                                                  uint32_t n_scenarios, const smmc_allocation_sweep_outputs *out) {
  int kind = SMMC_DIV_EXACT;
  int rc = check_scenarios(e, sim, pfs, cfs, n_scenarios, &kind);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_allocation_sweep_outputs");
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pfs, cfs, n_scenarios, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  typedef smmc_allocation_sweep_outputs O;
  const size_t per_path = sizeof(float) * sim->n_paths * n_scenarios;
  const smmc::OutputField fields[6] = {{offsetof(O, d_stats), static_cast<size_t>(smmc_stats_bytes(sim->n_bins)) * n_scenarios},
                                       {offsetof(O, d_depleted_at), sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u) * n_scenarios},
                                       {offsetof(O, d_final), per_path},
                                       {offsetof(O, d_holdings), per_path * pfs[0].n_assets},
                                       {offsetof(O, d_paid), per_path},
                                       {offsetof(O, d_ruin_period), per_path}};
  return smmc::host_outputs_struct_to_host(e, "simulate_allocation_sweep_to_host", *out, fields, [&](const O *d) {
    return smmc_engine_simulate_allocation_sweep(e, sim, pfs, cfs, n_scenarios, d);
  });
}

}  // extern "C"
