// smmc_portfolio_cashflow.cpp -- smmc_engine_simulate_portfolio_cashflow, its _to_host form and
// smmc_engine_portfolio_cashflow_divide_kind (include/smmc.h): a withdrawal or contribution schedule on a jointly
// drawn, rebalanced K-asset portfolio, with depletion statistics.
//
// A translation unit of its own, as its two parents: smmc_capi.cpp owns struct smmc_engine and never calls into this
// file.  The portfolio's argument checks, asset table and launch arguments are smmc_portfolio.cpp's, the schedule's
// checks and staging smmc_cashflow.cpp's (smmc_host.h, "lend"): this unit states neither again and keeps no state
// of its own.  What is its own: the LDS need, the divide rule ("Portfolio cash flows", has the proof), the
// kernel arguments, and which record and count array the launch leaves.  The launch is a wave walk and its run the
// shared one (smmc_host.h, host_wave_walk_run), as are the output structure's checks.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "smmc_host.h"

namespace {

using smmc::cashflow_varying;
using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as cashflow_kernel: a workgroup flushes n_periods + 1 + n_bins counters.
constexpr uint32_t kGroupsPerCU = 32;

int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf) {
  const int rc = smmc::portfolio_check(e, sim, pf);
  return rc ? rc : smmc::cashflow_check_schedule(sim, cf);
}

// The rule of include/smmc.h (smmc_engine_portfolio_cashflow_divide_kind); DESIGN.md, "Portfolio cash flows", has the
// proof.  FAST only for the two schedule shapes it covers; everything else is the IEEE divide.
// Its two halves: the bounds of this call's own law, and the rule on given bounds (smmc_host.h lends the second).
int divide_of_bounds(const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const double *lo, double hi_max) {
  if (sim->flags & SMMC_FLAG_EXACT_DIV) return SMMC_DIV_EXACT;
  const double cap = sim->initial_capital;
  if (!(cap > 0.0) || !std::isfinite(cap)) return SMMC_DIV_EXACT;
  const uint32_t K = pf->n_assets, P = sim->n_periods;
  double lo_min = INFINITY, w_min = INFINITY, h_min = INFINITY;
  bool held = false;
  for (uint32_t k = 0; k < K; ++k) {
    lo_min = std::min(lo_min, lo[k]);
    if (!(pf->weights[k] > 0.0f)) continue;
    const float h0 = sim->initial_capital * pf->weights[k];  // the kernel's own first holding
    if (!(h0 > 0.0f)) return SMMC_DIV_EXACT;  // a weighted asset that starts at 0 would start from a flow's share
    held = true;
    w_min = std::min(w_min, static_cast<double>(pf->weights[k]));
    h_min = std::min(h_min, static_cast<double>(h0));
  }
  if (!held) return SMMC_DIV_EXACT;
  const double p = P;
  const double grow = std::max(0.0, std::log2(hi_max / 100.0)), shrink = std::max(0.0, -std::log2(lo_min / 100.0));
  // the roundings of one period (two per compounding, K - 1 of the sum, three of the flow and its shares) and the
  // weights' sum, within 1e-6 of 1, move a logarithm by less than 2^-18 per period; one bit more on each side
  const double slack = 1.0 + p * 0x1p-18;

  // the flows: all of them paid in (every amount <= 0, every fraction 0), or one constant amount and fraction 0
  bool no_fraction = true, all_in = true;
  double paid_in = 0.0;
  for (uint32_t t = 0; t < (cashflow_varying(cf) ? P : 1u); ++t) {
    const double am = cf->amounts ? cf->amounts[t] : cf->amount, fr = cf->fractions ? cf->fractions[t] : cf->fraction;
    no_fraction = no_fraction && fr == 0.0;
    all_in = all_in && am <= 0.0;
    paid_in += std::fabs(am) * (cashflow_varying(cf) ? 1.0 : p);
  }
  if (!no_fraction) return SMMC_DIV_EXACT;
  // above, both shapes: the sum of the holdings' magnitudes grows by the best asset's factor and by |amount| per period
  if (!(std::log2(cap + paid_in) + p * grow + std::log2(hi_max) + slack < 127.0)) return SMMC_DIV_EXACT;

  if (all_in) {
    // below: holdings only gain from a flow, so the portfolio rule's bound stands -- a positive holding started as the
    // smallest positive initial holding or as the smallest positive weight's share of a value that is at least cap
    // shrunk by the worst asset in every period so far, and shrinks no faster since
    const double start = std::min(std::log2(h_min), std::log2(w_min) + std::log2(cap));
    if (start - p * shrink + std::min(0.0, std::log2(lo_min)) - slack > -89.0) return SMMC_DIV_FAST;
  }
  if (!cashflow_varying(cf) && cf->amount != 0.0f) {
    // below: a holding that enters a product is the initial one, a rebalanced share of a value above the floor, or a
    // binary32 difference with the flow's share s_k = fl(amount * w_k), which is 0 or at least 2^-25 |s_k|
    const bool rebalances = pf->rebalance_every != 0 && pf->rebalance_every < P;
    if (rebalances && !(cf->floor > 0.0f)) return SMMC_DIV_EXACT;
    for (uint32_t k = 0; k < K; ++k) {
      if (!(pf->weights[k] > 0.0f)) continue;  // such a holding is 0 throughout
      const float share = cf->amount * pf->weights[k];
      double least = std::min(static_cast<double>(sim->initial_capital * pf->weights[k]), std::fabs(static_cast<double>(share)) * 0x1p-25);
      if (rebalances) least = std::min(least, static_cast<double>(cf->floor) * pf->weights[k]);
      if (!(least > 0.0) || !(std::log2(least) + std::min(0.0, std::log2(lo[k])) - 1.0 > -89.0)) return SMMC_DIV_EXACT;
    }
    return SMMC_DIV_FAST;
  }
  return SMMC_DIV_EXACT;
}
int divide_rule(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf) {
  double lo[SMMC_MAX_ASSETS], hi_max = 0.0;
  for (uint32_t k = 0; k < pf->n_assets; ++k) {
    double hi;
    if (!smmc::portfolio_asset_bounds(e, sim, pf, k, &lo[k], &hi)) return SMMC_DIV_EXACT;
    hi_max = std::max(hi_max, hi);
  }
  return divide_of_bounds(sim, pf, cf, lo, hi_max);
}

// The launch's arguments and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::PortfolioCashflowArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, bool want_stats, Plan *out) {
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
  const size_t lds = smmc::portfolio_cashflow_lds_bytes(out->a.mode, out->a.table_len, pf->n_assets, sim->n_periods, out->a.n_bins);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "asset table, depletion counters and histogram need %zu bytes of LDS, device allows %zu", lds,
                     view.max_lds);
  return SMMC_OK;
}

}  // namespace

namespace smmc {  // what smmc_portfolio_cashflow_regimes.cpp takes of this unit (smmc_host.h)
int portfolio_cashflow_divide_of_bounds(const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const double *lo, double hi_max) {
  return divide_of_bounds(sim, pf, cf, lo, hi_max);
}
}  // namespace smmc

extern "C" {

int smmc_engine_portfolio_cashflow_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf) {
  const int rc = check_request(e, sim, pf, cf);
  if (rc) return rc;
  return divide_rule(e, sim, pf, cf);
}

int smmc_engine_simulate_portfolio_cashflow(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                            const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, cf);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_cashflow_outputs");
  if (rc) return rc;
  rc = smmc::host_check_depletion_alignment(out);
  if (rc) return rc;
  Plan pl;
  rc = plan(e, sim, pf, cf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  smmc::CashflowArgs &c = pl.x.c;
  pl.a.d_final = out->d_final;
  pl.x.p.d_holdings = out->d_holdings;
  c.d_paid = out->d_paid;
  c.d_ruin_period = out->d_ruin_period;
  const bool exact_div = pl.grid && divide_rule(e, sim, pf, cf) != SMMC_DIV_FAST;
  const smmc::WaveWalk walk = {"launch_portfolio_cashflow", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kDepletedAt, sim->n_periods + 1u, &c.d_depleted}}};
  return smmc::host_wave_walk_run(
      e, walk, smmc::FoldRecord(), [&](hipStream_t stream) { return smmc::launch_portfolio_cashflow(pl.a, pl.x, exact_div, pl.grid, stream); },
      [&] { return cashflow_varying(cf) && pl.grid ? smmc::cashflow_stage_schedule(e, sim, cf, &c) : SMMC_OK; });
}

int smmc_engine_simulate_portfolio_cashflow_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                    const smmc_cashflow *cf, const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, cf);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_cashflow_outputs");
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pf, cf, out->d_stats != nullptr, &pl);
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
  return smmc::host_outputs_struct_to_host(e, "simulate_portfolio_cashflow_to_host", *out, fields,
                                           [&](const O *d) { return smmc_engine_simulate_portfolio_cashflow(e, sim, pf, cf, d); });
}

}  // extern "C"
