// smmc_portfolio_cashflow_checkpoints.cpp -- smmc_engine_simulate_portfolio_cashflow_checkpoints and its _to_host form
// (include/smmc.h): the paths of smmc_engine_simulate_portfolio_cashflow with the record of their values after each of
// n_checkpoints chosen periods -- the fan chart of a plan.
//
// A translation unit of its own, as its parents: smmc_capi.cpp owns struct smmc_engine and never calls into this file.
// The portfolio's checks, asset table and launch arguments are smmc_portfolio.cpp's, the schedule's checks and staging
// smmc_cashflow.cpp's, the checkpoint arguments' checks smmc_capi.cpp's (smmc_host.h, "lend"), the divide rule the
// parent entry's own (asked through smmc_engine_portfolio_cashflow_divide_kind): this unit states none of them again.
// What is its own: the LDS need, the kernel arguments, which records and count array the launch leaves, and the
// partials of the checkpoint records, [checkpoint][workgroup], kept per engine in this unit's extension slot and grown
// on demand.  The launch is a wave walk and its run the shared one (smmc_host.h, host_wave_walk_run).
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstring>
#include <new>

#include "smmc_host.h"

namespace {

using smmc::cashflow_varying;
using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as the parent: a workgroup flushes its counters and leaves one partial per record.
constexpr uint32_t kGroupsPerCU = 32;

struct State {
  smmc::DeviceBuffer<smmc::BlockPartial> d_ck_partials;  // [checkpoint][workgroup], grown on demand
};
void release_state(void *p) { delete static_cast<State *>(p); }
const char kOwner = 0;  // its address names this unit's slot among the engine's (engine_ext)

int state_of(smmc_engine *e, State **out) {
  smmc::EngineExt *ext = smmc::engine_ext(e, &kOwner);
  if (!ext) return host_fail(SMMC_ERR_INVALID, "the engine has no extension slot left for the checkpoint partials");
  if (!ext->state) {
    State *st = new (std::nothrow) State();
    if (!st) return host_fail(SMMC_ERR_NOMEM, "out of host memory");
    ext->state = st;
    ext->release = release_state;
  }
  *out = static_cast<State *>(ext->state);
  return SMMC_OK;
}

// Every check that needs no device, the parent's first; records: the pointer whose alignment is checked.
int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const uint32_t *periods,
                  uint32_t n_checkpoints, const smmc_portfolio_cashflow_outputs *out, const void *records) {
  int rc = smmc::portfolio_check(e, sim, pf);
  if (rc) return rc;
  rc = smmc::cashflow_check_schedule(sim, cf);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_cashflow_outputs");
  if (rc) return rc;
  return smmc::host_check_checkpoint_args(sim, periods, n_checkpoints, nullptr, records);
}

// The launch's arguments and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::PortfolioCashflowCheckpointsArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const uint32_t *periods,
         uint32_t n_checkpoints, Plan *out) {
  const smmc::EngineView view = smmc::engine_view(e);
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kGroupsPerCU, view.max_grid, &out->grid);
  if (rc) return rc;
  smmc::portfolio_launch_args(e, sim, pf, &out->a, &out->x.p);  // a.n_bins stays sim's: the checkpoints' records have buckets
  smmc::CashflowArgs &c = out->x.c;                            // also where the final record is not asked for
  std::memset(&c, 0, sizeof c);
  c.amount = cf->amount;
  c.fraction = cf->fraction;
  c.floor = cf->floor;
  out->x.n = n_checkpoints;
  for (uint32_t i = 0; i < SMMC_MAX_CHECKPOINTS; ++i) out->x.periods[i] = i < n_checkpoints ? periods[i] : 0xffffffffu;
  out->x.ck_partials = nullptr;
  out->x.d_ck_hist = nullptr;
  const size_t lds =
      smmc::portfolio_cashflow_checkpoints_lds_bytes(out->a.mode, out->a.table_len, pf->n_assets, sim->n_periods, out->a.n_bins, n_checkpoints);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID,
                     "asset table, depletion counters, histogram and checkpoint histograms need %zu bytes of LDS, device allows %zu", lds,
                     view.max_lds);
  return SMMC_OK;
}

}  // namespace

extern "C" {

int smmc_engine_simulate_portfolio_cashflow_checkpoints(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                        const smmc_cashflow *cf, const uint32_t *periods, uint32_t n_checkpoints,
                                                        const smmc_portfolio_cashflow_outputs *out, void *d_records) {
  int rc = check_request(e, sim, pf, cf, periods, n_checkpoints, out, d_records);
  if (rc) return rc;
  rc = smmc::host_check_depletion_alignment(out);
  if (rc) return rc;
  Plan pl;
  rc = plan(e, sim, pf, cf, periods, n_checkpoints, &pl);
  if (rc) return rc;
  smmc::CashflowArgs &c = pl.x.c;
  pl.a.d_final = out->d_final;
  pl.x.p.d_holdings = out->d_holdings;
  c.d_paid = out->d_paid;
  c.d_ruin_period = out->d_ruin_period;
  // the parent's rule answers for this call: a value has to be right whenever it meets the floor, so also at a checkpoint
  const bool exact_div = pl.grid && smmc_engine_portfolio_cashflow_divide_kind(e, sim, pf, cf) != SMMC_DIV_FAST;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  State *st = nullptr;
  rc = state_of(e, &st);
  if (rc) return rc;
  // drained: an earlier launch may still read the old array
  SMMC_HIP(st->d_ck_partials.reserve(sizeof(smmc::BlockPartial) * pl.grid * n_checkpoints, &view.stream));
  const smmc::WaveWalk walk = {"launch_portfolio_cashflow_checkpoints",
                               pl.grid,
                               sim->n_bins,
                               {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kDepletedAt, sim->n_periods + 1u, &c.d_depleted}},
                               {d_records, n_checkpoints, st->d_ck_partials.p, smmc::kCheckpointBucketsAt, &pl.x.ck_partials, &pl.x.d_ck_hist}};
  return smmc::host_wave_walk_run(
      e, walk, smmc::FoldRecord(),
      [&](hipStream_t stream) { return smmc::launch_portfolio_cashflow_checkpoints(pl.a, pl.x, exact_div, pl.grid, stream); },
      [&] { return cashflow_varying(cf) && pl.grid ? smmc::cashflow_stage_schedule(e, sim, cf, &c) : SMMC_OK; }, smmc::FoldCheckpointSet());
}

int smmc_engine_simulate_portfolio_cashflow_checkpoints_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                                const smmc_cashflow *cf, const uint32_t *periods, uint32_t n_checkpoints,
                                                                const smmc_portfolio_cashflow_outputs *out, void *host_records) {
  // host memory needs no alignment: a non-null records pointer passes as an aligned one
  int rc = check_request(e, sim, pf, cf, periods, n_checkpoints, out, host_records ? reinterpret_cast<const void *>(8) : nullptr);
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pf, cf, periods, n_checkpoints, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  struct Pieces {  // the parent's outputs and the records, as one structure of pointers
    smmc_portfolio_cashflow_outputs out;
    void *records;
  };
  typedef smmc_portfolio_cashflow_outputs O;
  const Pieces host = {*out, host_records};
  const size_t per_path = sizeof(float) * sim->n_paths, at = offsetof(Pieces, out);
  const smmc::OutputField fields[7] = {{offsetof(Pieces, records), static_cast<size_t>(smmc_stats_bytes(sim->n_bins)) * n_checkpoints},
                                       {at + offsetof(O, d_stats), static_cast<size_t>(smmc_stats_bytes(sim->n_bins))},
                                       {at + offsetof(O, d_depleted_at), sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u)},
                                       {at + offsetof(O, d_final), per_path},
                                       {at + offsetof(O, d_holdings), per_path * pf->n_assets},
                                       {at + offsetof(O, d_paid), per_path},
                                       {at + offsetof(O, d_ruin_period), per_path}};
  return smmc::host_outputs_struct_to_host(e, "simulate_portfolio_cashflow_checkpoints_to_host", host, fields, [&](const Pieces *d) {
    return smmc_engine_simulate_portfolio_cashflow_checkpoints(e, sim, pf, cf, periods, n_checkpoints, &d->out, d->records);
  });
}

}  // extern "C"
