// smmc_portfolio_cashflow_stationary.cpp -- smmc_engine_simulate_portfolio_cashflow_stationary, its _to_host form and
// smmc_engine_portfolio_cashflow_stationary_divide_kind (include/smmc.h): smmc_engine_simulate_portfolio_cashflow's plan
// on rows chosen by the stationary bootstrap, runs of consecutive rows of geometric length.
//
// A translation unit of its own, as smmc_portfolio_cashflow_blocks.cpp: smmc_capi.cpp owns struct smmc_engine and never
// calls into this file.  The portfolio's checks, asset table and launch arguments are smmc_portfolio.cpp's, the schedule's
// checks and staging smmc_cashflow.cpp's, the checks of `st` smmc_stationary.cpp's (smmc_host.h, stationary_check), the divide rule
// the parent entry's own (asked through smmc_engine_portfolio_cashflow_divide_kind: its bounds never depend on the order of
// the rows -- DESIGN.md, "Block-bootstrap plans"): this unit states none of them again and keeps no state of its own.
// What is its own: the LDS need, the kernel arguments, and which record and count array the launch leaves.  The launch is
// a wave walk and its run the shared one (smmc_host.h, host_wave_walk_run), as are the output structure's checks.
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstring>

#include "smmc_host.h"

namespace {

using smmc::cashflow_varying;
using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as the parent: a workgroup flushes n_periods + 1 + n_bins counters.
constexpr uint32_t kGroupsPerCU = 32;

// Everything the parent refuses, then what the stationary bootstrap refuses (Gaussian mode among it).
int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const smmc_stationary *st) {
  int rc = smmc::portfolio_check(e, sim, pf);
  if (rc) return rc;
  rc = smmc::cashflow_check_schedule(sim, cf);
  return rc ? rc : smmc::stationary_check(sim, st);
}

// The launch's arguments and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::PortfolioCashflowStationaryArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const smmc_stationary *st,
         bool want_stats, Plan *out) {
  const smmc::EngineView view = smmc::engine_view(e);
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kGroupsPerCU, view.max_grid, &out->grid);
  if (rc) return rc;
  smmc::portfolio_launch_args(e, sim, pf, &out->a, &out->x.p);
  if (!want_stats) out->a.n_bins = 0;
  smmc::CashflowArgs &c = out->x.c;
  std::memset(&c, 0, sizeof c);
  c.amount = cf->amount;
  c.fraction = cf->fraction;
  c.floor = cf->floor;
  out->x.renew_q16 = st->renew_q16;
  return smmc::host_check_lds(view, smmc::portfolio_cashflow_geometric_lds_bytes(out->a.table_len, pf->n_assets, sim->n_periods, out->a.n_bins),
                              "asset table, depletion counters and histogram");
}

}  // namespace

extern "C" {

int smmc_engine_portfolio_cashflow_stationary_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                                          const smmc_stationary *st) {
  const int rc = check_request(e, sim, pf, cf, st);
  if (rc) return rc;
  return smmc_engine_portfolio_cashflow_divide_kind(e, sim, pf, cf);
}

int smmc_engine_simulate_portfolio_cashflow_stationary(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                                       const smmc_stationary *st, const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, cf, st);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_cashflow_outputs");
  if (rc) return rc;
  rc = smmc::host_check_depletion_alignment(out);
  if (rc) return rc;
  Plan pl;
  rc = plan(e, sim, pf, cf, st, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  smmc::CashflowArgs &c = pl.x.c;
  pl.a.d_final = out->d_final;
  pl.x.p.d_holdings = out->d_holdings;
  c.d_paid = out->d_paid;
  c.d_ruin_period = out->d_ruin_period;
  // the parent's rule answers for this call: the same products, in another order of the rows
  const bool exact_div = pl.grid && smmc_engine_portfolio_cashflow_divide_kind(e, sim, pf, cf) != SMMC_DIV_FAST;
  const smmc::WaveWalk walk = {"launch_portfolio_cashflow_geometric", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kDepletedAt, sim->n_periods + 1u, &c.d_depleted}}};
  return smmc::host_wave_walk_run(
      e, walk, smmc::FoldRecord(), [&](hipStream_t stream) { return smmc::launch_portfolio_cashflow_geometric(pl.a, pl.x, exact_div, pl.grid, stream); },
      [&] { return cashflow_varying(cf) && pl.grid ? smmc::cashflow_stage_schedule(e, sim, cf, &c) : SMMC_OK; });
}

int smmc_engine_simulate_portfolio_cashflow_stationary_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                               const smmc_cashflow *cf, const smmc_stationary *st,
                                                               const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, cf, st);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_cashflow_outputs");
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pf, cf, st, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  typedef smmc_portfolio_cashflow_outputs O;
  const size_t per_path = sizeof(float) * sim->n_paths;
  const smmc::OutputField fields[6] = {{offsetof(O, d_stats), static_cast<size_t>(smmc_stats_bytes(sim->n_bins))},
                                       {offsetof(O, d_depleted_at), sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u)},
                                       {offsetof(O, d_final), per_path},
                                       {offsetof(O, d_holdings), per_path * pf->n_assets},
                                       {offsetof(O, d_paid), per_path},
                                       {offsetof(O, d_ruin_period), per_path}};
  return smmc::host_outputs_struct_to_host(e, "simulate_portfolio_cashflow_stationary_to_host", *out, fields, [&](const O *d) {
    return smmc_engine_simulate_portfolio_cashflow_stationary(e, sim, pf, cf, st, d);
  });
}

}  // extern "C"
