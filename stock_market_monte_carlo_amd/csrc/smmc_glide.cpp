// smmc_glide.cpp -- smmc_engine_simulate_glide, its _to_host form and smmc_engine_glide_divide_kind (include/smmc.h):
// the portfolio cash-flow call with target weights that change along the plan.
//
// A translation unit of its own, as smmc_guardrails.cpp: smmc_capi.cpp owns struct smmc_engine and never calls into this
// file, and no other unit refers to it.  The portfolio's argument checks, asset table and launch arguments are
// smmc_portfolio.cpp's, the schedule's checks and staging smmc_cashflow.cpp's (smmc_host.h, "lend").  What is this
// unit's own: the checks of smmc_glide, the divide rule ("Glide paths", carries the parent's proof over), the
// flattened change table and its staging -- kept per engine in this unit's extension slot, as the cash-flow schedule is
// --, the kernel arguments, and the launch.  One asset has one legal weight vector: such a request is checked here and
// is then smmc_engine_simulate_portfolio_cashflow itself.  The launch is a wave walk and its run the shared one
// (smmc_host.h, host_wave_walk_run), as are the output structure's checks.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#include "smmc_host.h"

namespace {

using smmc::cashflow_varying;
using smmc::DeviceGuard;
using smmc::GlideEntry;
using smmc::host_fail;

// Workgroups per CU, as portfolio_cashflow_kernel: a workgroup flushes n_periods + 1 + n_bins counters.
constexpr uint32_t kGroupsPerCU = 32;
// the most entries a table has: every change and the entry behind them
constexpr uint32_t kEntriesMax = SMMC_MAX_GLIDE_CHANGES + 1u;

// The staged change table of an engine, as smmc_cashflow.cpp stages a schedule: a call flattens the caller's arrays
// into one of kSlots page-locked slots and enqueues the upload from there; a slot is reused only after the upload that
// read it has finished (its event).  One device copy is enough: the upload of a call is ordered behind the kernel of
// the call before it on the engine stream.
constexpr int kSlots = 4;
struct GlideState {
  smmc::PinnedBuffer<GlideEntry> h_slots;  // page-locked, kSlots x kEntriesMax
  smmc::DeviceBuffer<GlideEntry> d_table;  // kEntriesMax
  hipEvent_t uploaded[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  bool in_flight[kSlots] = {false, false, false, false};
  int next = 0;
};

void release_state(void *p) {
  GlideState *st = static_cast<GlideState *>(p);
  if (!st) return;
  for (hipEvent_t ev : st->uploaded)
    if (ev) (void)hipEventDestroy(ev);
  delete st;  // the two buffers with it
}

const char kOwner = 0;  // its address names this unit's slot among the engine's (engine_ext)

// Device must be current.
int state_of(smmc_engine *e, GlideState **out) {
  smmc::EngineExt *ext = smmc::engine_ext(e, &kOwner);
  if (!ext) return host_fail(SMMC_ERR_INVALID, "the engine has no extension slot left for the glide path's change table");
  if (!ext->state) {
    GlideState *st = new (std::nothrow) GlideState();
    if (!st) return host_fail(SMMC_ERR_NOMEM, "out of host memory");
    ext->state = st;
    ext->release = release_state;
    const size_t bytes = sizeof(GlideEntry) * kEntriesMax;
    SMMC_HIP(st->h_slots.reserve(bytes * kSlots, nullptr));  // both allocated once
    SMMC_HIP(st->d_table.reserve(bytes, nullptr));
    for (hipEvent_t &ev : st->uploaded) SMMC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  *out = static_cast<GlideState *>(ext->state);
  if (!(*out)->h_slots.p || !(*out)->d_table.p || !(*out)->uploaded[kSlots - 1])
    return host_fail(SMMC_ERR_HIP, "the engine's glide-path staging buffers could not be allocated earlier");
  return SMMC_OK;
}

const float *row_of(const smmc_glide *gl, uint32_t c) { return gl->weights + static_cast<size_t>(c) * SMMC_MAX_ASSETS; }

int check_glide(const smmc_portfolio *pf, const smmc_glide *gl) {
  if (!gl) return host_fail(SMMC_ERR_INVALID, "the smmc_glide argument is NULL");
  if (gl->struct_size != sizeof(smmc_glide))
    return host_fail(SMMC_ERR_INVALID, "smmc_glide.struct_size is %u, this library expects %zu", gl->struct_size, sizeof(smmc_glide));
  if (gl->n_changes > SMMC_MAX_GLIDE_CHANGES)
    return host_fail(SMMC_ERR_INVALID, "n_changes %u exceeds SMMC_MAX_GLIDE_CHANGES %d", gl->n_changes, SMMC_MAX_GLIDE_CHANGES);
  if (gl->n_changes == 0) return SMMC_OK;
  if (!gl->after) return host_fail(SMMC_ERR_INVALID, "smmc_glide.after is NULL with n_changes = %u", gl->n_changes);
  if (!gl->weights) return host_fail(SMMC_ERR_INVALID, "smmc_glide.weights is NULL with n_changes = %u", gl->n_changes);
  const uint32_t K = pf->n_assets;
  for (uint32_t c = 0; c < gl->n_changes; ++c) {
    if (gl->after[c] == 0) return host_fail(SMMC_ERR_INVALID, "after[%u] is 0: a change takes effect after period 1 at the earliest", c);
    if (c && !(gl->after[c] > gl->after[c - 1]))
      return host_fail(SMMC_ERR_INVALID, "after[%u] = %u does not exceed after[%u] = %u: the periods must be strictly increasing", c, gl->after[c],
                       c - 1, gl->after[c - 1]);
    const float *row = row_of(gl, c);
    double sum = 0.0;  // the checks of smmc_portfolio::weights
    for (uint32_t k = 0; k < SMMC_MAX_ASSETS; ++k) {
      const float w = row[k];
      if (!std::isfinite(w) || w < 0.0f)
        return host_fail(SMMC_ERR_INVALID, "row %u of the glide path: weights[%u] is %g: a weight is finite and >= 0", c, k, static_cast<double>(w));
      if (k >= K && w != 0.0f)
        return host_fail(SMMC_ERR_INVALID, "row %u of the glide path: weights[%u] is %g beyond n_assets = %u: it must be 0", c, k,
                         static_cast<double>(w), K);
      sum += static_cast<double>(w);
    }
    if (!(std::fabs(sum - 1.0) <= 1e-6))
      return host_fail(SMMC_ERR_INVALID, "row %u of the glide path: the weights sum to %.9g, not to 1 within 1e-6", c, sum);
  }
  return SMMC_OK;
}

int check_request(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const smmc_glide *gl) {
  int rc = smmc::portfolio_check(e, sim, pf);
  if (rc) return rc;
  rc = smmc::cashflow_check_schedule(sim, cf);
  return rc ? rc : check_glide(pf, gl);
}

// The rule of include/smmc.h (smmc_engine_glide_divide_kind): the parent's (smmc_portfolio_cashflow.cpp, divide_rule)
// with every bound that depends on a weight taken over pf->weights and every row, and refused where a row weights
// another set of assets positively than pf->weights does.  DESIGN.md, "Glide paths", carries the proof over.
int divide_rule(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const smmc_glide *gl) {
  if (sim->flags & SMMC_FLAG_EXACT_DIV) return SMMC_DIV_EXACT;
  const double cap = sim->initial_capital;
  if (!(cap > 0.0) || !std::isfinite(cap)) return SMMC_DIV_EXACT;
  const uint32_t K = pf->n_assets, P = sim->n_periods;
  for (uint32_t c = 0; c < gl->n_changes; ++c)
    for (uint32_t k = 0; k < K; ++k)
      if ((row_of(gl, c)[k] > 0.0f) != (pf->weights[k] > 0.0f)) return SMMC_DIV_EXACT;
  // per asset, over pf->weights and every row: the smallest weight and the smallest magnitude of a flow's share
  auto over_rows = [&](uint32_t k, float amount, double *w_least, double *share_least) {
    *w_least = pf->weights[k];
    *share_least = std::fabs(static_cast<double>(amount * pf->weights[k]));
    for (uint32_t c = 0; c < gl->n_changes; ++c) {
      const float w = row_of(gl, c)[k];
      *w_least = std::min(*w_least, static_cast<double>(w));
      *share_least = std::min(*share_least, std::fabs(static_cast<double>(amount * w)));  // the kernel's own share, in binary32
    }
  };
  double lo[SMMC_MAX_ASSETS], lo_min = INFINITY, hi_max = 0.0, w_min = INFINITY, h_min = INFINITY;
  bool held = false;
  for (uint32_t k = 0; k < K; ++k) {
    double hi;
    if (!smmc::portfolio_asset_bounds(e, sim, pf, k, &lo[k], &hi)) return SMMC_DIV_EXACT;
    lo_min = std::min(lo_min, lo[k]);
    hi_max = std::max(hi_max, hi);
    if (!(pf->weights[k] > 0.0f)) continue;
    const float h0 = sim->initial_capital * pf->weights[k];  // the kernel's own first holding
    if (!(h0 > 0.0f)) return SMMC_DIV_EXACT;
    held = true;
    double w_least, share_least;
    over_rows(k, 0.0f, &w_least, &share_least);
    w_min = std::min(w_min, w_least);
    h_min = std::min(h_min, static_cast<double>(h0));
  }
  if (!held) return SMMC_DIV_EXACT;
  const double p = P;
  const double grow = std::max(0.0, std::log2(hi_max / 100.0)), shrink = std::max(0.0, -std::log2(lo_min / 100.0));
  const double slack = 1.0 + p * 0x1p-18;  // the parent's: the roundings of a period and the weights' sum within 1e-6 of 1

  bool no_fraction = true, all_in = true;
  double paid_in = 0.0;
  for (uint32_t t = 0; t < (cashflow_varying(cf) ? P : 1u); ++t) {
    const double am = cf->amounts ? cf->amounts[t] : cf->amount, fr = cf->fractions ? cf->fractions[t] : cf->fraction;
    no_fraction = no_fraction && fr == 0.0;
    all_in = all_in && am <= 0.0;
    paid_in += std::fabs(am) * (cashflow_varying(cf) ? 1.0 : p);
  }
  if (!no_fraction) return SMMC_DIV_EXACT;
  if (!(std::log2(cap + paid_in) + p * grow + std::log2(hi_max) + slack < 127.0)) return SMMC_DIV_EXACT;

  if (all_in) {
    const double start = std::min(std::log2(h_min), std::log2(w_min) + std::log2(cap));
    if (start - p * shrink + std::min(0.0, std::log2(lo_min)) - slack > -89.0) return SMMC_DIV_FAST;
  }
  if (!cashflow_varying(cf) && cf->amount != 0.0f) {
    const bool rebalances = pf->rebalance_every != 0 && pf->rebalance_every < P;
    if (rebalances && !(cf->floor > 0.0f)) return SMMC_DIV_EXACT;
    for (uint32_t k = 0; k < K; ++k) {
      if (!(pf->weights[k] > 0.0f)) continue;  // such a holding is 0 throughout: no row weights it either
      double w_least, share_least;
      over_rows(k, cf->amount, &w_least, &share_least);
      double least = std::min(static_cast<double>(sim->initial_capital * pf->weights[k]), share_least * 0x1p-25);
      if (rebalances) least = std::min(least, static_cast<double>(cf->floor) * w_least);
      if (!(least > 0.0) || !(std::log2(least) + std::min(0.0, std::log2(lo[k])) - 1.0 > -89.0)) return SMMC_DIV_EXACT;
    }
    return SMMC_DIV_FAST;
  }
  return SMMC_DIV_EXACT;
}

// The changes that fall inside the plan, flattened as glide_kernel walks them (GlideEntry, smmc_internal.h): entry c holds
// the targets from change c on and the periods to change c + 1 (0 behind the last); one more entry, all zero, follows.
// Returns the number of entries written; *first: after[0], or 0 when no change falls inside the plan.
uint32_t flatten(const smmc_sim *sim, const smmc_glide *gl, GlideEntry *table, uint32_t *first) {
  uint32_t n = 0;
  while (n < gl->n_changes && gl->after[n] <= sim->n_periods) ++n;  // strictly increasing: the rest is beyond P too
  std::memset(table, 0, sizeof(GlideEntry) * (n + 1u));
  for (uint32_t c = 0; c < n; ++c) {
    table[c].next = c + 1u < n ? gl->after[c + 1u] - gl->after[c] : 0u;
    for (uint32_t k = 0; k < SMMC_MAX_ASSETS; ++k) table[c].weights[k] = row_of(gl, c)[k];
  }
  *first = n ? gl->after[0] : 0u;
  return n + 1u;
}

// Flattens the changes into a free staging slot and enqueues the upload on the engine stream; x gets the device copy.
// Device must be current.
int stage_table(smmc_engine *e, const smmc_sim *sim, const smmc_glide *gl, smmc::GlideArgs *x) {
  const smmc::EngineView view = smmc::engine_view(e);
  GlideState *st = nullptr;
  const int rc = state_of(e, &st);
  if (rc) return rc;
  const int slot = st->next;
  if (st->in_flight[slot]) SMMC_HIP(hipEventSynchronize(st->uploaded[slot]));
  st->in_flight[slot] = false;
  GlideEntry *h = st->h_slots.p + static_cast<size_t>(slot) * kEntriesMax;
  const uint32_t n = flatten(sim, gl, h, &x->first);
  SMMC_HIP(hipMemcpyAsync(st->d_table.p, h, sizeof(GlideEntry) * n, hipMemcpyHostToDevice, view.stream));
  SMMC_HIP(hipEventRecord(st->uploaded[slot], view.stream));
  st->in_flight[slot] = true;
  st->next = (slot + 1) % kSlots;
  x->table = st->d_table.p;
  return SMMC_OK;
}

// The launch's arguments and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::GlideArgs x;
  uint32_t grid;
};
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, bool want_stats, Plan *out) {
  const smmc::EngineView view = smmc::engine_view(e);
  const int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kGroupsPerCU, view.max_grid, &out->grid);
  if (rc) return rc;
  std::memset(&out->x, 0, sizeof out->x);
  smmc::portfolio_launch_args(e, sim, pf, &out->a, &out->x.p);
  if (!want_stats) out->a.n_bins = 0;
  smmc::CashflowArgs &c = out->x.c;
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

int smmc_engine_glide_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                  const smmc_glide *glide) {
  const int rc = check_request(e, sim, pf, cf, glide);
  if (rc) return rc;
  return divide_rule(e, sim, pf, cf, glide);
}

int smmc_engine_simulate_glide(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                               const smmc_glide *glide, const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, cf, glide);
  if (rc) return rc;
  if (pf->n_assets == 1) return smmc_engine_simulate_portfolio_cashflow(e, sim, pf, cf, out);  // every legal row is w_0 = 1
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
  const bool exact_div = pl.grid && divide_rule(e, sim, pf, cf, glide) != SMMC_DIV_FAST;
  const smmc::WaveWalk walk = {"launch_glide", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}},
                               {{out->d_depleted_at, smmc::kDepletedAt, sim->n_periods + 1u, &c.d_depleted}}};
  return smmc::host_wave_walk_run(
      e, walk, smmc::FoldRecord(), [&](hipStream_t stream) { return smmc::launch_glide(pl.a, pl.x, exact_div, pl.grid, stream); },
      [&] {
        if (!pl.grid) return static_cast<int>(SMMC_OK);
        const int staged = cashflow_varying(cf) ? smmc::cashflow_stage_schedule(e, sim, cf, &c) : SMMC_OK;
        return staged ? staged : stage_table(e, sim, glide, &pl.x);
      });
}

int smmc_engine_simulate_glide_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                       const smmc_glide *glide, const smmc_portfolio_cashflow_outputs *out) {
  int rc = check_request(e, sim, pf, cf, glide);
  if (rc) return rc;
  if (pf->n_assets == 1) return smmc_engine_simulate_portfolio_cashflow_to_host(e, sim, pf, cf, out);
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
  return smmc::host_outputs_struct_to_host(e, "simulate_glide_to_host", *out, fields,
                                           [&](const O *d) { return smmc_engine_simulate_glide(e, sim, pf, cf, glide, d); });
}

}  // extern "C"
