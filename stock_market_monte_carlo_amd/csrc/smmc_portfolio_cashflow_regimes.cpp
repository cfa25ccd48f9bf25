// smmc_portfolio_cashflow_regimes.cpp -- smmc_engine_simulate_portfolio_cashflow_regimes, its _to_host form and
// smmc_engine_portfolio_cashflow_regimes_divide_kind (include/smmc.h): smmc_engine_simulate_portfolio_cashflow's plan in
// Gaussian mode under smmc_engine_simulate_regimes' hidden state, each regime with a joint law of its own.
//
// A translation unit of its own, as smmc_portfolio_cashflow_stationary.cpp: smmc_capi.cpp owns struct smmc_engine and never
// calls into this file.  The portfolio's checks, bounds and launch arguments are smmc_portfolio.cpp's, the schedule's
// checks and staging smmc_cashflow.cpp's, the divide rule on given bounds smmc_portfolio_cashflow.cpp's
// (portfolio_cashflow_divide_of_bounds), the checks of the probabilities smmc_host.h's (markov_check_q16): this unit
// states none of them again and keeps no state of its own.  What is its own: the checks of `rg`, the union of the two
// regimes' bounds, the LDS need, the kernel arguments, and which record and count array the launch leaves.  The launch is
// a wave walk and its run the shared one (smmc_host.h, host_wave_walk_run), as are the output structure's checks.
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

constexpr uint32_t kK = SMMC_MAX_ASSETS;
// Workgroups per CU, as the parent: the same grid rule, so the record's two binary64 sums are the parent's too.
constexpr uint32_t kGroupsPerCU = 32;

// The sim the shared host code sees: gauss_mean and gauss_std of the caller's are not read, the staged draw yields
// standard normals.
smmc_sim plain_sim(const smmc_sim *sim) {
  smmc_sim plain = *sim;
  plain.gauss_mean = 0.0f;
  plain.gauss_std = 1.0f;
  return plain;
}

// pf with regime r's law in its Gaussian fields: what the portfolio's bounds are asked about.
smmc_portfolio law_of(const smmc_portfolio *pf, const smmc_portfolio_regimes *rg, int r) {
  smmc_portfolio law = *pf;
  std::memcpy(law.means, rg->means[r], sizeof law.means);
  std::memcpy(law.factor, rg->factor[r], sizeof law.factor);
  return law;
}

// The mode and the stream first, then everything the parent refuses of (sim, pf, cf), then pf's Gaussian fields, then rg.
int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_portfolio_regimes *rg,
                  const smmc_cashflow *cf) {
  if (!e) return host_fail(SMMC_ERR_INVALID, "engine is NULL");
  if (!sim) return host_fail(SMMC_ERR_INVALID, "sim is NULL");
  if (sim->struct_size != sizeof(smmc_sim))
    return host_fail(SMMC_ERR_INVALID, "smmc_sim.struct_size is %u, this library expects %zu", sim->struct_size, sizeof(smmc_sim));
  if (sim->mode != SMMC_MODE_GAUSSIAN)
    return host_fail(SMMC_ERR_INVALID, "a regime-switching plan is a law of Gaussian returns: mode must be SMMC_MODE_GAUSSIAN (got %d)", sim->mode);
  int rc = smmc::host_require_v3(sim, "regime-switching plans support");
  if (rc) return rc;
  const smmc_sim plain = plain_sim(sim);
  rc = smmc::portfolio_check(e, &plain, pf);
  if (rc) return rc;
  rc = smmc::cashflow_check_schedule(&plain, cf);
  if (rc) return rc;
  for (uint32_t k = 0; k < kK; ++k)
    if (pf->means[k] != 0.0f) return host_fail(SMMC_ERR_INVALID, "smmc_portfolio.means[%u] is set: the laws stand in smmc_portfolio_regimes, it must be 0", k);
  for (uint32_t i = 0; i < kK * kK; ++i)
    if (pf->factor[i] != 0.0f)
      return host_fail(SMMC_ERR_INVALID, "smmc_portfolio.factor[%u] is set: the laws stand in smmc_portfolio_regimes, it must be 0", i);
  if (!rg) return host_fail(SMMC_ERR_INVALID, "the smmc_portfolio_regimes argument is NULL");
  if (rg->struct_size != sizeof(smmc_portfolio_regimes))
    return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_regimes.struct_size is %u, this library expects %zu", rg->struct_size,
                     sizeof(smmc_portfolio_regimes));
  rc = smmc::markov_check_q16(rg->leave_q16, rg->start1_q16);
  if (rc) return rc;
  const uint32_t K = pf->n_assets;
  for (int r = 0; r < 2; ++r)
    for (uint32_t k = 0; k < kK; ++k) {
      const float m = rg->means[r][k];
      if (!std::isfinite(m)) return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_regimes.means[%d][%u] is not finite", r, k);
      if (k >= K && m != 0.0f)
        return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_regimes.means[%d][%u] is set beyond n_assets = %u: it must be 0", r, k, K);
      for (uint32_t j = 0; j < kK; ++j) {
        const float l = rg->factor[r][k * kK + j];
        if (!std::isfinite(l)) return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_regimes.factor[%d][%u][%u] is not finite", r, k, j);
        if ((j > k || k >= K) && l != 0.0f)
          return host_fail(SMMC_ERR_INVALID,
                           "smmc_portfolio_regimes.factor[%d][%u][%u] is %g: entries above the diagonal and beyond n_assets = %u must be 0", r, k,
                           j, static_cast<double>(l), K);
        if (j == k && l < 0.0f)
          return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_regimes.factor[%d][%u][%u] is %g: the diagonal must be >= 0", r, k, j,
                           static_cast<double>(l));
      }
    }
  if (rg->reserved[0] != 0 || rg->reserved[1] != 0)
    return host_fail(SMMC_ERR_INVALID, "smmc_portfolio_regimes.reserved is {%u, %u}, it must be 0", rg->reserved[0], rg->reserved[1]);
  return SMMC_OK;
}

// The rule of include/smmc.h (smmc_engine_portfolio_cashflow_regimes_divide_kind): the parent's on the union of the two
// regimes' per-asset bounds ("Regime-switching plans", has the argument).
int divide_rule(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_portfolio_regimes *rg, const smmc_cashflow *cf) {
  const smmc_sim plain = plain_sim(sim);
  double lo[kK], hi_max = 0.0;
  for (uint32_t k = 0; k < pf->n_assets; ++k) {
    lo[k] = INFINITY;
    for (int r = 0; r < 2; ++r) {
      const smmc_portfolio law = law_of(pf, rg, r);
      double lo_r, hi_r;
      if (!smmc::portfolio_asset_bounds(e, &plain, &law, k, &lo_r, &hi_r)) return SMMC_DIV_EXACT;  // also of a regime never entered
      lo[k] = std::min(lo[k], lo_r);
      hi_max = std::max(hi_max, hi_r);
    }
  }
  return smmc::portfolio_cashflow_divide_of_bounds(&plain, pf, cf, lo, hi_max);
}

// The LDS need, stated once: with the record's n_bins buckets, or with none where no record is asked for.
int check_lds(const smmc_engine *e, const smmc_sim *sim, uint32_t n_bins) {
  return smmc::host_check_lds(smmc::engine_view(e), smmc::portfolio_cashflow_markov_lds_bytes(sim->n_periods, n_bins),
                              "draw tables, depletion counters and histogram");
}

// The launch's arguments, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::PortfolioCashflowMarkovArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_portfolio_regimes *rg, const smmc_cashflow *cf,
         bool want_stats, Plan *out) {
  const smmc::EngineView view = smmc::engine_view(e);
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kGroupsPerCU, view.max_grid, &out->grid);
  if (rc) return rc;
  const smmc_sim plain = plain_sim(sim);
  smmc::PortfolioCashflowMarkovArgs &x = out->x;
  std::memset(&x, 0, sizeof x);
  smmc::portfolio_launch_args(e, &plain, pf, &out->a, &x.p);
  if (!want_stats) out->a.n_bins = 0;
  x.c.amount = cf->amount;
  x.c.fraction = cf->fraction;
  x.c.floor = cf->floor;
  for (int r = 0; r < 2; ++r) {
    for (uint32_t k = 0; k < kK; ++k) x.shift100[r][k] = 100.0f + rg->means[r][k];
    std::memcpy(x.factor[r], rg->factor[r], sizeof x.factor[r]);
    x.leave_q16[r] = rg->leave_q16[r];
  }
  x.start1_q16 = rg->start1_q16;
  return check_lds(e, sim, out->a.n_bins);
}

}  // namespace

extern "C" {

int smmc_engine_portfolio_cashflow_regimes_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                       const smmc_portfolio_regimes *rg, const smmc_cashflow *cf) {
  int rc = check_request(e, sim, pf, rg, cf);
  if (rc) return rc;
  rc = check_lds(e, sim, 0u);  // the tables and the depletion counters must fit: which record the call will ask for is not known here
  if (rc) return rc;
  return divide_rule(e, sim, pf, rg, cf);
}

int smmc_engine_simulate_portfolio_cashflow_regimes(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                    const smmc_portfolio_regimes *rg, const smmc_cashflow *cf,
                                                    const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, rg, cf);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_cashflow_outputs");
  if (rc) return rc;
  rc = smmc::host_check_depletion_alignment(out);
  if (rc) return rc;
  Plan pl;
  rc = plan(e, sim, pf, rg, cf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  smmc::CashflowArgs &c = pl.x.c;
  pl.a.d_final = out->d_final;
  pl.x.p.d_holdings = out->d_holdings;
  c.d_paid = out->d_paid;
  c.d_ruin_period = out->d_ruin_period;
  const bool exact_div = pl.grid && divide_rule(e, sim, pf, rg, cf) != SMMC_DIV_FAST;
  const smmc::WaveWalk walk = {"launch_portfolio_cashflow_markov", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kDepletedAt, sim->n_periods + 1u, &c.d_depleted}}};
  return smmc::host_wave_walk_run(
      e, walk, smmc::FoldRecord(), [&](hipStream_t stream) { return smmc::launch_portfolio_cashflow_markov(pl.a, pl.x, exact_div, pl.grid, stream); },
      [&] { return cashflow_varying(cf) && pl.grid ? smmc::cashflow_stage_schedule(e, sim, cf, &c) : SMMC_OK; });
}

int smmc_engine_simulate_portfolio_cashflow_regimes_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                            const smmc_portfolio_regimes *rg, const smmc_cashflow *cf,
                                                            const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, rg, cf);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_cashflow_outputs");
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pf, rg, cf, out->d_stats != nullptr, &pl);
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
  return smmc::host_outputs_struct_to_host(e, "simulate_portfolio_cashflow_regimes_to_host", *out, fields, [&](const O *d) {
    return smmc_engine_simulate_portfolio_cashflow_regimes(e, sim, pf, rg, cf, d);
  });
}

}  // extern "C"
