// smmc_guardrails.cpp -- smmc_engine_simulate_guardrails and its _to_host form (include/smmc.h): a constant starting
// withdrawal on a jointly drawn, rebalanced K-asset portfolio that a review rule adjusts per path, with depletion
// statistics and the counts of cuts and raises.
//
// A translation unit of its own, as smmc_portfolio_cashflow.cpp: smmc_capi.cpp owns struct smmc_engine and never calls
// into this file, and no other unit refers to it.  The portfolio's argument checks, asset table and launch arguments
// are smmc_portfolio.cpp's (smmc_host.h, "lend").  What is this unit's own: the checks of smmc_guardrails, the LDS need,
// the kernel arguments, and which record and count arrays the launch leaves.  There is no divide rule: the amount varies
// per path and the kernel always takes the IEEE divide ("Guardrails").  The launch is a wave walk and its run
// the shared one (smmc_host.h, host_wave_walk_run), as are the output structure's checks.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstddef>
#include <cstring>

#include "smmc_host.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as portfolio_cashflow_kernel: a workgroup flushes 3 (n_periods + 1) + n_bins counters.
constexpr uint32_t kGroupsPerCU = 32;
// The engine's accumulator as this launch divides it: the final-value histogram in copy 0, the depletion counters
// where every depletion entry has them, the counts of cuts and of raises behind those.
constexpr size_t kCountsLen = SMMC_MAX_CASHFLOW_PERIODS + 1u;
constexpr size_t kCutsAt = smmc::kDepletedAt + kCountsLen;
constexpr size_t kRaisesAt = kCutsAt + kCountsLen;
static_assert(kRaisesAt + kCountsLen <= static_cast<size_t>(smmc::kHistSpread) * SMMC_MAX_BINS,
              "the engine's accumulator holds the histogram and the three count arrays side by side");

int check_rule(const smmc_sim *sim, const smmc_guardrails *gr) {
  if (!gr) return host_fail(SMMC_ERR_INVALID, "the smmc_guardrails argument is NULL");
  if (gr->struct_size != sizeof(smmc_guardrails))
    return host_fail(SMMC_ERR_INVALID, "smmc_guardrails.struct_size is %u, this library expects %zu", gr->struct_size, sizeof(smmc_guardrails));
  if (sim->n_periods == 0) return host_fail(SMMC_ERR_INVALID, "n_periods is 0: a cash flow needs at least one period");
  if (sim->n_periods > SMMC_MAX_CASHFLOW_PERIODS)
    return host_fail(SMMC_ERR_INVALID, "n_periods %u exceeds SMMC_MAX_CASHFLOW_PERIODS %d", sim->n_periods, SMMC_MAX_CASHFLOW_PERIODS);
  // every comparison is written so that a NaN fails it
  if (!(gr->amount > 0.0f) || !std::isfinite(gr->amount))
    return host_fail(SMMC_ERR_INVALID, "amount must be finite and > 0 (got %g)", static_cast<double>(gr->amount));
  if (!(gr->index > 0.0f) || !std::isfinite(gr->index))
    return host_fail(SMMC_ERR_INVALID, "index must be finite and > 0 (got %g)", static_cast<double>(gr->index));
  if (!(gr->lower >= 0.0f) || !(gr->lower <= gr->upper))
    return host_fail(SMMC_ERR_INVALID, "the bands must satisfy 0 <= lower <= upper (got lower %g, upper %g)", static_cast<double>(gr->lower),
                     static_cast<double>(gr->upper));
  if (!(gr->cut > 0.0f) || !(gr->cut <= 1.0f)) return host_fail(SMMC_ERR_INVALID, "cut must satisfy 0 < cut <= 1 (got %g)", static_cast<double>(gr->cut));
  if (!(gr->raise >= 1.0f) || !std::isfinite(gr->raise))
    return host_fail(SMMC_ERR_INVALID, "raise must be finite and >= 1 (got %g)", static_cast<double>(gr->raise));
  if (!(gr->amount_min >= 0.0f) || !(gr->amount_min <= gr->amount) || !(gr->amount <= gr->amount_max))
    return host_fail(SMMC_ERR_INVALID, "the clamps must satisfy 0 <= amount_min <= amount <= amount_max (got %g, %g, %g)",
                     static_cast<double>(gr->amount_min), static_cast<double>(gr->amount), static_cast<double>(gr->amount_max));
  if (!std::isfinite(gr->floor) || gr->floor < 0.0f)
    return host_fail(SMMC_ERR_INVALID, "floor must be finite and >= 0 (got %g)", static_cast<double>(gr->floor));
  return SMMC_OK;
}

int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_guardrails *gr) {
  const int rc = smmc::portfolio_check(e, sim, pf);
  return rc ? rc : check_rule(sim, gr);
}

// The launch's arguments and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::GuardrailsArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_guardrails *gr, bool want_stats, Plan *out) {
  const smmc::EngineView view = smmc::engine_view(e);
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kGroupsPerCU, view.max_grid, &out->grid);
  if (rc) return rc;
  smmc::GuardrailsArgs &x = out->x;
  std::memset(&x, 0, sizeof x);
  smmc::portfolio_launch_args(e, sim, pf, &out->a, &x.p);
  if (!want_stats) out->a.n_bins = 0;
  x.review_every = gr->review_every;
  x.amount = gr->amount;
  x.index = gr->index;
  x.upper = gr->upper;
  x.lower = gr->lower;
  x.cut = gr->cut;
  x.raise = gr->raise;
  x.amount_min = gr->amount_min;
  x.amount_max = gr->amount_max;
  x.floor = gr->floor;
  const size_t lds = smmc::guardrails_lds_bytes(out->a.mode, out->a.table_len, pf->n_assets, sim->n_periods, out->a.n_bins);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "asset table, depletion, cut and raise counters and histogram need %zu bytes of LDS, device allows %zu",
                     lds, view.max_lds);
  return SMMC_OK;
}

}  // namespace

extern "C" {

int smmc_engine_simulate_guardrails(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_guardrails *gr,
                                    const smmc_guardrails_outputs *out) {
  int rc = check_request(e, sim, pf, gr);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_guardrails_outputs");
  if (rc) return rc;
  rc = smmc::host_check_depletion_alignment(
      out, smmc::host_misaligned({out->d_amount_last, out->d_amount_lowest, out->d_cuts, out->d_raises}, 4),
      "d_final, d_holdings, d_paid, d_ruin_period, d_amount_last, d_amount_lowest, d_cuts and d_raises must be 4-byte aligned");
  if (rc) return rc;
  if (smmc::host_misaligned({out->d_cuts_at, out->d_raises_at}, 8))
    return host_fail(SMMC_ERR_INVALID, "d_cuts_at and d_raises_at must be 8-byte aligned");
  Plan pl;
  rc = plan(e, sim, pf, gr, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  smmc::GuardrailsArgs &x = pl.x;
  pl.a.d_final = out->d_final;
  x.p.d_holdings = out->d_holdings;
  x.d_paid = out->d_paid;
  x.d_ruin_period = out->d_ruin_period;
  x.d_amount_last = out->d_amount_last;
  x.d_amount_lowest = out->d_amount_lowest;
  x.d_cuts = out->d_cuts;
  x.d_raises = out->d_raises;
  const uint32_t n_at = sim->n_periods + 1u;
  const smmc::WaveWalk walk = {"launch_guardrails", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kDepletedAt, n_at, &x.d_depleted},
                                {out->d_cuts_at, kCutsAt, n_at, &x.d_cuts_at},
                                {out->d_raises_at, kRaisesAt, n_at, &x.d_raises_at}}};
  return smmc::host_wave_walk_run(e, walk, smmc::FoldRecord(),
                                  [&](hipStream_t stream) { return smmc::launch_guardrails(pl.a, pl.x, pl.grid, stream); });
}

int smmc_engine_simulate_guardrails_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_guardrails *gr,
                                            const smmc_guardrails_outputs *out) {
  int rc = check_request(e, sim, pf, gr);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_guardrails_outputs");
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pf, gr, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  typedef smmc_guardrails_outputs O;
  const size_t per_path = sizeof(float) * sim->n_paths;
  const size_t counts = sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u);
  const smmc::OutputField fields[12] = {{offsetof(O, d_stats), static_cast<size_t>(smmc_stats_bytes(sim->n_bins))},
                                        {offsetof(O, d_depleted_at), counts},
                                        {offsetof(O, d_cuts_at), counts},
                                        {offsetof(O, d_raises_at), counts},
                                        {offsetof(O, d_final), per_path},
                                        {offsetof(O, d_holdings), per_path * pf->n_assets},
                                        {offsetof(O, d_paid), per_path},
                                        {offsetof(O, d_ruin_period), per_path},
                                        {offsetof(O, d_amount_last), per_path},
                                        {offsetof(O, d_amount_lowest), per_path},
                                        {offsetof(O, d_cuts), per_path},
                                        {offsetof(O, d_raises), per_path}};
  return smmc::host_outputs_struct_to_host(e, "simulate_guardrails_to_host", *out, fields,
                                           [&](const O *d) { return smmc_engine_simulate_guardrails(e, sim, pf, gr, d); });
}

}  // extern "C"
