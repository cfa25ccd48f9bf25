// smmc_portfolio_cashflow.cpp -- smmc_engine_simulate_portfolio_cashflow, its _to_host form and
// smmc_engine_portfolio_cashflow_divide_kind (include/smmc.h): a withdrawal or contribution schedule on a jointly
// drawn, rebalanced K-asset portfolio, with depletion statistics.
//
// A translation unit of its own, as its two parents: smmc_capi.cpp owns struct smmc_engine and never calls into this
// file.  The portfolio's argument checks, asset table and launch arguments are smmc_portfolio.cpp's, the schedule's
// checks and staging smmc_cashflow.cpp's (smmc_internal.h, "lend"): this unit states neither again and keeps no state
// of its own.  What is its own: the output structure's checks, the LDS need, the divide rule ("Portfolio
// cash flows", has the proof) and the launch.  The launch is a wave walk and its host side the shared one:
// host_wave_walk_grid, engine_acc_lease, host_timed_launch, host_outputs_to_host and SMMC_HIP.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "smmc_host.h"
#include "smmc_internal.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as cashflow_kernel: a workgroup flushes n_periods + 1 + n_bins counters.
constexpr uint32_t kGroupsPerCU = 32;
// The depletion counters take the engine's accumulator from copy 1 on (copy 0 holds the final-value histogram).
constexpr size_t kDepletedAt = SMMC_MAX_BINS;
static_assert(kDepletedAt + SMMC_MAX_CASHFLOW_PERIODS + 1 <= static_cast<size_t>(smmc::kHistSpread) * SMMC_MAX_BINS,
              "the engine's accumulator holds the histogram and the depletion counters");

bool varying(const smmc_cashflow *cf) { return cf->amounts || cf->fractions; }

int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf) {
  const int rc = smmc::portfolio_check(e, sim, pf);
  return rc ? rc : smmc::cashflow_check_schedule(sim, cf);
}

int check_outputs(const smmc_portfolio_cashflow_outputs *out) {
  if (!out) return host_fail(SMMC_ERR_INVALID, "the smmc_portfolio_cashflow_outputs argument is NULL");
  if (out->struct_size != sizeof(smmc_portfolio_cashflow_outputs))
    return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_cashflow_outputs.struct_size is %u, this library expects %zu", out->struct_size,
                     sizeof(smmc_portfolio_cashflow_outputs));
  if (out->reserved != 0)
    return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_cashflow_outputs.reserved is %u, it must be 0", out->reserved);
  return SMMC_OK;
}

// The rule of include/smmc.h (smmc_engine_portfolio_cashflow_divide_kind); DESIGN.md, "Portfolio cash flows", has the
// proof.  FAST only for the two schedule shapes it covers; everything else is the IEEE divide.
int divide_rule(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf) {
  if (sim->flags & SMMC_FLAG_EXACT_DIV) return SMMC_DIV_EXACT;
  const double cap = sim->initial_capital;
  if (!(cap > 0.0) || !std::isfinite(cap)) return SMMC_DIV_EXACT;
  const uint32_t K = pf->n_assets, P = sim->n_periods;
  double lo[SMMC_MAX_ASSETS], lo_min = INFINITY, hi_max = 0.0, w_min = INFINITY, h_min = INFINITY;
  bool held = false;
  for (uint32_t k = 0; k < K; ++k) {
    double hi;
    if (!smmc::portfolio_asset_bounds(e, sim, pf, k, &lo[k], &hi)) return SMMC_DIV_EXACT;
    lo_min = std::min(lo_min, lo[k]);
    hi_max = std::max(hi_max, hi);
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
  for (uint32_t t = 0; t < (varying(cf) ? P : 1u); ++t) {
    const double am = cf->amounts ? cf->amounts[t] : cf->amount, fr = cf->fractions ? cf->fractions[t] : cf->fraction;
    no_fraction = no_fraction && fr == 0.0;
    all_in = all_in && am <= 0.0;
    paid_in += std::fabs(am) * (varying(cf) ? 1.0 : p);
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
  if (!varying(cf) && cf->amount != 0.0f) {
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
  rc = check_outputs(out);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(out->d_final) | reinterpret_cast<uintptr_t>(out->d_holdings) | reinterpret_cast<uintptr_t>(out->d_paid) |
       reinterpret_cast<uintptr_t>(out->d_ruin_period)) & 3u)
    return host_fail(SMMC_ERR_INVALID, "d_final, d_holdings, d_paid and d_ruin_period must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(out->d_stats) | reinterpret_cast<uintptr_t>(out->d_depleted_at)) & 7u)
    return host_fail(SMMC_ERR_INVALID, "d_stats and d_depleted_at must be 8-byte aligned");
  Plan pl;
  rc = plan(e, sim, pf, cf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);

  smmc::KernelArgs &a = pl.a;
  smmc::CashflowArgs &c = pl.x.c;
  a.d_final = out->d_final;
  pl.x.p.d_holdings = out->d_holdings;
  c.d_paid = out->d_paid;
  c.d_ruin_period = out->d_ruin_period;
  if (varying(cf) && pl.grid) {
    rc = smmc::cashflow_stage_schedule(e, sim, cf, &c);
    if (rc) return rc;
  }
  smmc::ZeroLease lease;
  if ((out->d_stats && sim->n_bins) || out->d_depleted_at) {  // zero now, and zero again after the finalize launches below
    rc = smmc::engine_acc_lease(e, &lease);
    if (rc) return rc;
  }
  unsigned long long *const acc = lease.acc();
  if (out->d_stats) {
    a.partials = view.d_partials;
    a.d_hist = sim->n_bins ? acc : nullptr;
  }
  if (out->d_depleted_at) c.d_depleted = acc + kDepletedAt;
  if (pl.grid) {
    const bool exact_div = divide_rule(e, sim, pf, cf) != SMMC_DIV_FAST;
    rc = smmc::host_timed_launch(e, "launch_portfolio_cashflow",
                                 [&] { return smmc::launch_portfolio_cashflow(a, pl.x, exact_div, pl.grid, view.stream); });
    if (rc) return rc;
  }
  if (out->d_stats)
    SMMC_HIP(smmc::launch_finalize(view.d_partials, pl.grid, static_cast<smmc_stats *>(out->d_stats), sim->n_bins, view.stream,
                                   sim->n_bins ? acc : nullptr, sim->n_bins ? 1u : 0u));
  if (out->d_depleted_at)
    SMMC_HIP(smmc::launch_finalize_depleted(acc + kDepletedAt, sim->n_periods + 1u,
                                            reinterpret_cast<unsigned long long *>(out->d_depleted_at), view.stream));
  lease.finalize_queued();
  return SMMC_OK;
}

int smmc_engine_simulate_portfolio_cashflow_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                    const smmc_cashflow *cf, const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, cf);
  if (rc) return rc;
  rc = check_outputs(out);
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pf, cf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  const size_t per_path = sizeof(float) * sim->n_paths;
  const smmc::HostPiece pieces[6] = {{out->d_stats, static_cast<size_t>(smmc_stats_bytes(sim->n_bins))},
                                     {out->d_depleted_at, sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u)},
                                     {out->d_final, per_path},
                                     {out->d_holdings, per_path * pf->n_assets},
                                     {out->d_paid, per_path},
                                     {out->d_ruin_period, per_path}};
  return smmc::host_outputs_to_host(e, "simulate_portfolio_cashflow_to_host", pieces, 6, [&](void *const *dev) {
    smmc_portfolio_cashflow_outputs d = *out;
    d.d_stats = dev[0];
    d.d_depleted_at = static_cast<uint64_t *>(dev[1]);
    d.d_final = static_cast<float *>(dev[2]);
    d.d_holdings = static_cast<float *>(dev[3]);
    d.d_paid = static_cast<float *>(dev[4]);
    d.d_ruin_period = static_cast<uint32_t *>(dev[5]);
    return smmc_engine_simulate_portfolio_cashflow(e, sim, pf, cf, &d);
  });
}

}  // extern "C"
