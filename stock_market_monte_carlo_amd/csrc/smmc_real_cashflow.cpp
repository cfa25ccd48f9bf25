// smmc_real_cashflow.cpp -- smmc_engine_simulate_real_cashflow, its _to_host form and
// smmc_engine_real_cashflow_divide_kind (include/smmc.h): a schedule in money of period 0 on a jointly drawn, rebalanced
// K-asset portfolio, indexed by a price index that series K of the joint law compounds per path.
//
// A translation unit of its own, as smmc_portfolio_cashflow.cpp: smmc_capi.cpp owns struct smmc_engine and never calls
// into this file, and no other unit refers to it.  The joint law is K + 1 series wide, so the portfolio's argument
// checks, asset table, multiplier bounds and launch arguments are smmc_portfolio.cpp's put to a copy of the request
// with n_assets = K + 1 (`law` below: the lent helpers take the width from the structure and need no parameter for
// it); the schedule's checks and staging are smmc_cashflow.cpp's (smmc_host.h, "lend").  What is this unit's own:
// the two checks the wider law cannot make (K = SMMC_MAX_ASSETS, weights[K] != 0), the wording of its alignment
// refusal, the divide rule ("Real cash flows", has the proof), the LDS need and the kernel arguments.  The
// launch is a wave walk and its run the shared one (smmc_host.h, host_wave_walk_run), as are the output structure's checks.
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

// Workgroups per CU, as portfolio_cashflow_kernel: a workgroup flushes n_periods + 1 + n_bins counters.
constexpr uint32_t kGroupsPerCU = 32;

// Every check on (e, sim, pf, cf); on success *law is pf at the joint law's width, n_assets = K + 1.
int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, smmc_portfolio *law) {
  if (!e) return host_fail(SMMC_ERR_INVALID, "engine is NULL");
  if (!pf || pf->struct_size != sizeof(smmc_portfolio) || pf->n_assets == 0 || pf->n_assets > SMMC_MAX_ASSETS) {
    const int rc = smmc::portfolio_check(e, sim, pf);  // the parent's refusal, in its own words
    return rc ? rc : host_fail(SMMC_ERR_INVALID, "the smmc_portfolio argument is not usable");
  }
  const uint32_t K = pf->n_assets;
  if (K == SMMC_MAX_ASSETS)
    return host_fail(SMMC_ERR_INVALID, "n_assets is %u: a real cash flow holds 1 .. SMMC_MAX_ASSETS - 1 (%d) assets, the law's last series is inflation",
                     K, SMMC_MAX_ASSETS - 1);
  *law = *pf;
  law->n_assets = K + 1u;
  int rc = smmc::portfolio_check(e, sim, law);  // width K + 1: the table's columns, means, factor, the entries beyond
  if (rc) return rc;
  if (pf->weights[K] != 0.0f)
    return host_fail(SMMC_ERR_INVALID, "weights[%u] is %g: series %u is inflation and is not held, its weight must be 0", K,
                     static_cast<double>(pf->weights[K]), K);
  return smmc::cashflow_check_schedule(sim, cf);
}

// The rule of include/smmc.h (smmc_engine_real_cashflow_divide_kind); DESIGN.md, "Real cash flows", has the proof.
// FAST only with the index inside its window AND contributions only; everything else is the IEEE divide.
int divide_rule(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *law, const smmc_cashflow *cf) {
  if (sim->flags & SMMC_FLAG_EXACT_DIV) return SMMC_DIV_EXACT;
  const double cap = sim->initial_capital;
  if (!(cap > 0.0) || !std::isfinite(cap)) return SMMC_DIV_EXACT;
  const uint32_t K = law->n_assets - 1u, P = sim->n_periods;
  const double p = P;
  // the roundings of one period move a logarithm by less than 2^-18 (the parent's count; the index chain makes two, the
  // nominal amount one more); one bit more on each side
  const double slack = 1.0 + p * 0x1p-18;

  // the index: I_t lies in [lo_I^t, hi_I^t], the product it enters is 100 times the next index before rounding
  double lo_i, hi_i;
  if (!smmc::portfolio_asset_bounds(e, sim, law, K, &lo_i, &hi_i)) return SMMC_DIV_EXACT;
  const double log_lo = std::log2(lo_i / 100.0), log_hi = std::log2(hi_i / 100.0);
  if (!(p * log_lo >= -88.0) || !(p * log_hi < 126.0)) return SMMC_DIV_EXACT;  // the window of include/smmc.h
  if (!(p * std::max(0.0, log_hi) + std::log2(hi_i) + slack < 127.0)) return SMMC_DIV_EXACT;                  // I * a_K above
  if (!(p * std::min(0.0, log_lo) + std::min(0.0, std::log2(lo_i)) - slack > -89.0)) return SMMC_DIV_EXACT;  // and below

  // the holdings: the parent's bounds over the K invested assets
  double lo_min = INFINITY, hi_max = 0.0, w_min = INFINITY, h_min = INFINITY;
  bool held = false;
  for (uint32_t k = 0; k < K; ++k) {
    double lo, hi;
    if (!smmc::portfolio_asset_bounds(e, sim, law, k, &lo, &hi)) return SMMC_DIV_EXACT;
    lo_min = std::min(lo_min, lo);
    hi_max = std::max(hi_max, hi);
    if (!(law->weights[k] > 0.0f)) continue;
    const float h0 = sim->initial_capital * law->weights[k];  // the kernel's own first holding
    if (!(h0 > 0.0f)) return SMMC_DIV_EXACT;  // a weighted asset that starts at 0 would start from a flow's share
    held = true;
    w_min = std::min(w_min, static_cast<double>(law->weights[k]));
    h_min = std::min(h_min, static_cast<double>(h0));
  }
  if (!held) return SMMC_DIV_EXACT;
  const double grow = std::max(0.0, std::log2(hi_max / 100.0)), shrink = std::max(0.0, -std::log2(lo_min / 100.0));

  // the flows: contributions only -- every real amount <= 0, so every nominal one fl(amount * I) <= 0 -- and no fraction
  double paid_in = 0.0;
  for (uint32_t t = 0; t < (cashflow_varying(cf) ? P : 1u); ++t) {
    const double am = cf->amounts ? cf->amounts[t] : cf->amount, fr = cf->fractions ? cf->fractions[t] : cf->fraction;
    if (fr != 0.0 || !(am <= 0.0)) return SMMC_DIV_EXACT;
    paid_in += std::fabs(am) * (cashflow_varying(cf) ? 1.0 : p);
  }
  paid_in *= std::pow(std::max(1.0, hi_i / 100.0), p);  // no nominal amount exceeds |amount| max(1, hi_I)^P
  // above: the sum of the holdings grows by the best asset's factor and by the nominal amount per period
  if (!(std::log2(cap + paid_in) + p * grow + std::log2(hi_max) + slack < 127.0)) return SMMC_DIV_EXACT;
  // below: holdings only gain from a flow, so the portfolio rule's bound stands (smmc_portfolio_cashflow.cpp)
  const double start = std::min(std::log2(h_min), std::log2(w_min) + std::log2(cap));
  if (!(start - p * shrink + std::min(0.0, std::log2(lo_min)) - slack > -89.0)) return SMMC_DIV_EXACT;
  return SMMC_DIV_FAST;
}

// The launch's arguments and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::RealCashflowArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *law, const smmc_cashflow *cf, bool want_stats, Plan *out) {
  const smmc::EngineView view = smmc::engine_view(e);
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kGroupsPerCU, view.max_grid, &out->grid);
  if (rc) return rc;
  smmc::portfolio_launch_args(e, sim, law, &out->a, &out->x.p);  // rows, s_k and L at the law's width
  if (!want_stats) out->a.n_bins = 0;
  smmc::CashflowArgs &c = out->x.c;
  std::memset(&c, 0, sizeof c);
  c.amount = cf->amount;
  c.fraction = cf->fraction;
  c.floor = cf->floor;
  out->x.d_final_real = nullptr;
  out->x.d_index = nullptr;
  const size_t lds = smmc::portfolio_cashflow_lds_bytes(out->a.mode, out->a.table_len, law->n_assets, sim->n_periods, out->a.n_bins);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "asset table, depletion counters and histogram need %zu bytes of LDS, device allows %zu", lds,
                     view.max_lds);
  return SMMC_OK;
}

}  // namespace

extern "C" {

int smmc_engine_real_cashflow_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf) {
  smmc_portfolio law;
  const int rc = check_request(e, sim, pf, cf, &law);
  if (rc) return rc;
  return divide_rule(e, sim, &law, cf);
}

int smmc_engine_simulate_real_cashflow(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                       const smmc_real_cashflow_outputs *out) {
  smmc_portfolio law;
  int rc = check_request(e, sim, pf, cf, &law);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_real_cashflow_outputs");
  if (rc) return rc;
  rc = smmc::host_check_depletion_alignment(out, smmc::host_misaligned({out->d_final_real, out->d_index}, 4),
                                            "d_final, d_final_real, d_index, d_holdings, d_paid and d_ruin_period must be 4-byte aligned");
  if (rc) return rc;
  Plan pl;
  rc = plan(e, sim, &law, cf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  smmc::CashflowArgs &c = pl.x.c;
  pl.a.d_final = out->d_final;
  pl.x.d_final_real = out->d_final_real;
  pl.x.d_index = out->d_index;
  pl.x.p.d_holdings = out->d_holdings;
  c.d_paid = out->d_paid;
  c.d_ruin_period = out->d_ruin_period;
  const bool exact_div = pl.grid && divide_rule(e, sim, &law, cf) != SMMC_DIV_FAST;
  const smmc::WaveWalk walk = {"launch_real_cashflow", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kDepletedAt, sim->n_periods + 1u, &c.d_depleted}}};
  return smmc::host_wave_walk_run(
      e, walk, smmc::FoldRecord(), [&](hipStream_t stream) { return smmc::launch_real_cashflow(pl.a, pl.x, exact_div, pl.grid, stream); },
      [&] { return cashflow_varying(cf) && pl.grid ? smmc::cashflow_stage_schedule(e, sim, cf, &c) : SMMC_OK; });
}

int smmc_engine_simulate_real_cashflow_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                               const smmc_real_cashflow_outputs *out) {
  smmc_portfolio law;
  int rc = check_request(e, sim, pf, cf, &law);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_real_cashflow_outputs");
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, &law, cf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  typedef smmc_real_cashflow_outputs O;
  const size_t per_path = sizeof(float) * sim->n_paths;
  const smmc::OutputField fields[8] = {{offsetof(O, d_stats), static_cast<size_t>(smmc_stats_bytes(sim->n_bins))},
                                       {offsetof(O, d_depleted_at), sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u)},
                                       {offsetof(O, d_final), per_path},
                                       {offsetof(O, d_final_real), per_path},
                                       {offsetof(O, d_index), per_path},
                                       {offsetof(O, d_holdings), per_path * pf->n_assets},
                                       {offsetof(O, d_paid), per_path},
                                       {offsetof(O, d_ruin_period), per_path}};
  return smmc::host_outputs_struct_to_host(e, "simulate_real_cashflow_to_host", *out, fields,
                                           [&](const O *d) { return smmc_engine_simulate_real_cashflow(e, sim, pf, cf, d); });
}

}  // extern "C"
