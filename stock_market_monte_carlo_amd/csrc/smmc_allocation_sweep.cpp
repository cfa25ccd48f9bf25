// smmc_allocation_sweep.cpp -- smmc_engine_simulate_allocation_sweep, its _to_host form and
// smmc_engine_allocation_sweep_divide_kind (include/smmc.h): up to SMMC_MAX_SWEEP portfolio strategies -- weights,
// rebalancing, a constant cash flow and a floor each -- stepped on the same jointly drawn paths in one launch.
//
// A translation unit of its own, like smmc_sweep.cpp and smmc_portfolio_cashflow.cpp: no other unit calls into this
// file.  A scenario's argument checks are lent by smmc_portfolio.cpp and smmc_cashflow.cpp (smmc_internal.h, "lend"),
// its divide is smmc_engine_portfolio_cashflow_divide_kind's, asked scenario by scenario -- the rule and its proof stay
// in smmc_portfolio_cashflow.cpp.  What is this unit's own: the checks across scenarios (one joint law, constant
// schedules), the padding to the kernel's widths, the counter cap, the LDS need and the launch.  The launch is a wave
// walk on the shared host side (host_wave_walk_grid, engine_acc_lease, host_timed_launch, host_outputs_to_host); the
// scenarios travel as kernel arguments: nothing is staged, the unit keeps no state per engine.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>

#include "smmc_host.h"
#include "smmc_internal.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as cashflow_sweep_kernel; a workgroup leaves one partial per scenario in the engine's max_grid
// partials, so the grid is capped at max_grid / width as well.
constexpr uint32_t kGroupsPerCU = 32;
// The engine's accumulator: [scenario][bucket] from 0, [scenario][period] from kDepletedAt.
constexpr size_t kDepletedAt = SMMC_MAX_SWEEP_COUNTERS;
static_assert(2u * SMMC_MAX_SWEEP_COUNTERS <= static_cast<size_t>(smmc::kHistSpread) * SMMC_MAX_BINS,
              "the engine's accumulator holds a sweep's buckets and depletion counters");

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

int check_outputs(const smmc_allocation_sweep_outputs *out) {
  if (!out) return host_fail(SMMC_ERR_INVALID, "the smmc_allocation_sweep_outputs argument is NULL");
  if (out->struct_size != sizeof(smmc_allocation_sweep_outputs))
    return host_fail(SMMC_ERR_INVALID, "smmc_allocation_sweep_outputs.struct_size is %u, this library expects %zu", out->struct_size,
                     sizeof(smmc_allocation_sweep_outputs));
  if (out->reserved != 0)
    return host_fail(SMMC_ERR_INVALID, "smmc_allocation_sweep_outputs.reserved is %u, it must be 0", out->reserved);
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
  rc = check_outputs(out);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(out->d_final) | reinterpret_cast<uintptr_t>(out->d_holdings) | reinterpret_cast<uintptr_t>(out->d_paid) |
       reinterpret_cast<uintptr_t>(out->d_ruin_period)) & 3u)
    return host_fail(SMMC_ERR_INVALID, "d_final, d_holdings, d_paid and d_ruin_period must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(out->d_stats) | reinterpret_cast<uintptr_t>(out->d_depleted_at)) & 7u)
    return host_fail(SMMC_ERR_INVALID, "d_stats and d_depleted_at must be 8-byte aligned");
  Plan pl;
  rc = plan(e, sim, pfs, cfs, n_scenarios, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);

  smmc::KernelArgs &a = pl.a;
  smmc::AllocationSweepArgs &x = pl.x;
  a.d_final = out->d_final;
  x.p.d_holdings = out->d_holdings;
  x.d_paid = out->d_paid;
  x.d_ruin_period = out->d_ruin_period;
  smmc::ZeroLease lease;
  if ((out->d_stats && sim->n_bins) || out->d_depleted_at) {  // zero now, and zero again after the finalize launches below
    rc = smmc::engine_acc_lease(e, &lease);
    if (rc) return rc;
  }
  unsigned long long *const acc = lease.acc();
  if (out->d_stats) {
    a.partials = view.d_partials;  // [scenario][grid]
    a.d_hist = sim->n_bins ? acc : nullptr;
  }
  if (out->d_depleted_at) x.d_depleted = acc + kDepletedAt;
  if (pl.grid) {
    const bool exact_div = kind != SMMC_DIV_FAST;
    rc = smmc::host_timed_launch(e, "launch_allocation_sweep",
                                 [&] { return smmc::launch_allocation_sweep(a, x, exact_div, pl.grid, view.stream); });
    if (rc) return rc;
  }
  if (out->d_stats)
    SMMC_HIP(smmc::launch_finalize_sweep(view.d_partials, pl.grid, n_scenarios, out->d_stats, sim->n_bins, sim->n_bins ? acc : nullptr,
                                         view.stream));
  if (out->d_depleted_at)
    SMMC_HIP(smmc::launch_finalize_depleted(acc + kDepletedAt, n_scenarios * (sim->n_periods + 1u),
                                            reinterpret_cast<unsigned long long *>(out->d_depleted_at), view.stream));
  lease.finalize_queued();
  return SMMC_OK;
}

int smmc_engine_simulate_allocation_sweep_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs, const smmc_cashflow *cfs,
                                                  uint32_t n_scenarios, const smmc_allocation_sweep_outputs *out) {
  int kind = SMMC_DIV_EXACT;
  int rc = check_scenarios(e, sim, pfs, cfs, n_scenarios, &kind);
  if (rc) return rc;
  rc = check_outputs(out);
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pfs, cfs, n_scenarios, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  const size_t per_path = sizeof(float) * sim->n_paths * n_scenarios;
  const smmc::HostPiece pieces[6] = {{out->d_stats, static_cast<size_t>(smmc_stats_bytes(sim->n_bins)) * n_scenarios},
                                     {out->d_depleted_at, sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u) * n_scenarios},
                                     {out->d_final, per_path},
                                     {out->d_holdings, per_path * pfs[0].n_assets},
                                     {out->d_paid, per_path},
                                     {out->d_ruin_period, per_path}};
  return smmc::host_outputs_to_host(e, "simulate_allocation_sweep_to_host", pieces, 6, [&](void *const *dev) {
    smmc_allocation_sweep_outputs d = *out;
    d.d_stats = dev[0];
    d.d_depleted_at = static_cast<uint64_t *>(dev[1]);
    d.d_final = static_cast<float *>(dev[2]);
    d.d_holdings = static_cast<float *>(dev[3]);
    d.d_paid = static_cast<float *>(dev[4]);
    d.d_ruin_period = static_cast<uint32_t *>(dev[5]);
    return smmc_engine_simulate_allocation_sweep(e, sim, pfs, cfs, n_scenarios, &d);
  });
}

}  // extern "C"
