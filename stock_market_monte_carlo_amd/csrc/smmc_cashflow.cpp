// smmc_cashflow.cpp -- smmc_engine_simulate_cashflow and its siblings (include/smmc.h): withdrawal and
// contribution schedules with depletion statistics.
//
// A translation unit of its own: smmc_capi.cpp owns struct smmc_engine and never calls into this file; what is
// needed of an engine comes through smmc_host.h (engine_view, host_make_args, ...), and what this file keeps per engine
// -- the staged schedule -- hangs in this unit's extension slot of the engine (engine_ext), released by
// smmc_engine_destroy.  The launch is a wave walk, and its run is the shared one (smmc_host.h, host_wave_walk_run: device,
// lease, wiring, launch, folds).  What is this unit's own: the schedule's checks and staging, the divide rule, the LDS
// need, the kernel arguments, and which record and count array the launch leaves.  The reference has no counterpart: its
// README lists withdrawal strategies as open.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "smmc_host.h"

namespace {

using smmc::cashflow_varying;
using smmc::DeviceGuard;
using smmc::host_fail;

// Workgroups per CU, as checkpoints_kernel (smmc_capi.cpp): a workgroup flushes n_periods + 1 + n_bins counters.
constexpr uint32_t kCashflowGroupsPerCU = 32;
// schedule entries per array as staged: n_periods rounded up to whole Philox blocks (8 draws at the most)
constexpr uint32_t kStrideMax = (SMMC_MAX_CASHFLOW_PERIODS + 7u) & ~7u;

// The staged schedule of an engine.  The caller's arrays may be reused on return, so a call copies them into one of
// kSlots page-locked slots and enqueues the upload from there; a slot is reused only after the upload that read it
// has finished (its event).  One device copy is enough: the upload of a call is ordered behind the kernel of the
// call before it on the engine stream.
constexpr int kSlots = 4;
struct CashflowState {
  smmc::PinnedBuffer<float> h_slots;     // page-locked, kSlots x 2 x kStrideMax
  smmc::DeviceBuffer<float> d_schedule;  // 2 x kStrideMax
  hipEvent_t uploaded[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  bool in_flight[kSlots] = {false, false, false, false};
  int next = 0;
};

void release_state(void *p) {
  CashflowState *st = static_cast<CashflowState *>(p);
  if (!st) return;
  for (hipEvent_t ev : st->uploaded)
    if (ev) (void)hipEventDestroy(ev);
  delete st;  // the two buffers with it
}

const char kOwner = 0;  // its address names this unit's slot among the engine's (engine_ext)

// Device must be current.
int state_of(smmc_engine *e, CashflowState **out) {
  smmc::EngineExt *ext = smmc::engine_ext(e, &kOwner);
  if (!ext) return host_fail(SMMC_ERR_INVALID, "the engine has no extension slot left for the cash-flow schedule");
  if (!ext->state) {
    CashflowState *st = new (std::nothrow) CashflowState();
    if (!st) return host_fail(SMMC_ERR_NOMEM, "out of host memory");
    ext->state = st;
    ext->release = release_state;
    const size_t bytes = sizeof(float) * 2u * kStrideMax;
    SMMC_HIP(st->h_slots.reserve(bytes * kSlots, nullptr));  // both allocated once
    SMMC_HIP(st->d_schedule.reserve(bytes, nullptr));
    for (hipEvent_t &ev : st->uploaded) SMMC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  *out = static_cast<CashflowState *>(ext->state);
  if (!(*out)->h_slots.p || !(*out)->d_schedule.p || !(*out)->uploaded[kSlots - 1])
    return host_fail(SMMC_ERR_HIP, "the engine's cash-flow staging buffers could not be allocated earlier");
  return SMMC_OK;
}

float amount_at(const smmc_cashflow *cf, uint32_t t) { return cf->amounts ? cf->amounts[t] : cf->amount; }
float fraction_at(const smmc_cashflow *cf, uint32_t t) { return cf->fractions ? cf->fractions[t] : cf->fraction; }

int check_cf_struct(const smmc_cashflow *cf) {
  if (!cf) return host_fail(SMMC_ERR_INVALID, "cf is NULL");
  if (cf->struct_size != sizeof(smmc_cashflow))
    return host_fail(SMMC_ERR_INVALID, "smmc_cashflow.struct_size is %u, this library expects %zu", cf->struct_size,
                     sizeof(smmc_cashflow));
  return SMMC_OK;
}

int check_schedule(const smmc_sim *sim, const smmc_cashflow *cf) {
  if (sim->n_periods == 0) return host_fail(SMMC_ERR_INVALID, "n_periods is 0: a cash flow needs at least one period");
  if (sim->n_periods > SMMC_MAX_CASHFLOW_PERIODS)
    return host_fail(SMMC_ERR_INVALID, "n_periods %u exceeds SMMC_MAX_CASHFLOW_PERIODS %d", sim->n_periods,
                     SMMC_MAX_CASHFLOW_PERIODS);
  if (!std::isfinite(cf->floor) || cf->floor < 0.0f)
    return host_fail(SMMC_ERR_INVALID, "floor must be finite and >= 0 (got %g)", static_cast<double>(cf->floor));
  if (!cf->amounts && !std::isfinite(cf->amount))
    return host_fail(SMMC_ERR_INVALID, "amount is not finite");
  if (!cf->fractions && !std::isfinite(cf->fraction))
    return host_fail(SMMC_ERR_INVALID, "fraction is not finite");
  for (uint32_t t = 0; t < sim->n_periods; ++t) {
    if (cf->amounts && !std::isfinite(cf->amounts[t])) return host_fail(SMMC_ERR_INVALID, "amounts[%u] is not finite", t);
    if (cf->fractions && !std::isfinite(cf->fractions[t])) return host_fail(SMMC_ERR_INVALID, "fractions[%u] is not finite", t);
  }
  return SMMC_OK;
}

int check_cashflow(const smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf) {
  int rc = smmc::host_check_sim(e, sim);
  if (rc) return rc;
  rc = check_cf_struct(cf);
  if (rc) return rc;
  rc = smmc::host_require_v3(sim, "cash flows support");
  if (rc) return rc;
  return check_schedule(sim, cf);
}

// Copies the arrays of a varying schedule into a free staging slot and enqueues their upload on the engine stream; c
// gets the device copy and its stride.  Device must be current.
int stage_schedule(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf, smmc::CashflowArgs *c) {
  const smmc::EngineView view = smmc::engine_view(e);
  CashflowState *st = nullptr;
  const int rc = state_of(e, &st);
  if (rc) return rc;
  const int slot = st->next;
  if (st->in_flight[slot]) SMMC_HIP(hipEventSynchronize(st->uploaded[slot]));
  st->in_flight[slot] = false;
  const uint32_t stride = (sim->n_periods + 7u) & ~7u;
  float *h = st->h_slots.p + static_cast<size_t>(slot) * 2u * kStrideMax;
  for (uint32_t t = 0; t < stride; ++t) {
    h[t] = t < sim->n_periods ? amount_at(cf, t) : 0.0f;
    h[stride + t] = t < sim->n_periods ? fraction_at(cf, t) : 0.0f;
  }
  SMMC_HIP(hipMemcpyAsync(st->d_schedule.p, h, sizeof(float) * 2u * stride, hipMemcpyHostToDevice, view.stream));
  SMMC_HIP(hipEventRecord(st->uploaded[slot], view.stream));
  st->in_flight[slot] = true;
  st->next = (slot + 1) % kSlots;
  c->schedule = st->d_schedule.p;
  c->stride = stride;
  return SMMC_OK;
}

// The rule of include/smmc.h (smmc_engine_simulate_cashflow, "Divide").  The two-instruction divide is exact for
// products of at least 2^-114; as smmc_capi.cpp the host keeps them above 2^-89 and below 2^127, one bit of margin
// on each side for the roundings along a path.
int cashflow_divide(const smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf) {
  if (sim->flags & SMMC_FLAG_EXACT_DIV) return SMMC_DIV_EXACT;
  const double cap = sim->initial_capital;
  if (!(cap > 0.0) || !std::isfinite(cap)) return SMMC_DIV_EXACT;
  double lo_a, hi_a;
  if (!smmc::host_multiplier_bounds(e, sim, &lo_a, &hi_a)) return SMMC_DIV_EXACT;
  const uint32_t n = sim->n_periods, n_sched = cashflow_varying(cf) ? n : 1u;
  double contributions = 0.0, max_amount = -INFINITY, min_fraction = INFINITY, max_fraction = -INFINITY;
  for (uint32_t t = 0; t < n_sched; ++t) {
    const double am = amount_at(cf, t), fr = fraction_at(cf, t);
    if (am < 0.0) contributions += -am * (cashflow_varying(cf) ? 1.0 : static_cast<double>(n));
    max_amount = std::max(max_amount, am);
    min_fraction = std::min(min_fraction, fr);
    max_fraction = std::max(max_fraction, fr);
  }
  if (!(min_fraction >= 0.0 && max_fraction <= 1.0)) return SMMC_DIV_EXACT;
  const double p = n;
  // above: w >= -|amount| for a live path (g >= 0, fraction >= 0), so a value never exceeds what the capital and
  // all contributions, paid in at once, grow to
  const double grow = std::max(0.0, std::log2(hi_a / 100.0));
  if (!(std::log2(cap + contributions) + p * grow + std::log2(hi_a) + 1.0 < 127.0)) return SMMC_DIV_EXACT;
  // below: a live value is the capital, or above the floor, or -- nothing but contributions and fractions below
  // 1 -- at least the capital shrunk by the worst period n times
  double live_log2 = cf->floor > 0.0f ? std::log2(static_cast<double>(cf->floor)) : -INFINITY;
  if (max_amount <= 0.0 && max_fraction < 1.0) {
    const double shrink = std::min(0.0, std::log2(lo_a / 100.0 * (1.0 - max_fraction)));
    live_log2 = std::max(live_log2, std::log2(cap) + p * shrink);
  }
  live_log2 = std::min(live_log2, std::log2(cap));
  if (!(live_log2 + std::min(0.0, std::log2(lo_a)) - 1.0 > -89.0)) return SMMC_DIV_EXACT;
  return SMMC_DIV_FAST;
}

}  // namespace

namespace smmc {  // what smmc_portfolio_cashflow.cpp takes of this unit (smmc_host.h)
int cashflow_check_schedule(const smmc_sim *sim, const smmc_cashflow *cf) {
  const int rc = check_cf_struct(cf);
  return rc ? rc : check_schedule(sim, cf);
}
int cashflow_stage_schedule(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf, CashflowArgs *c) {
  return stage_schedule(e, sim, cf, c);
}
}  // namespace smmc

extern "C" {

int smmc_engine_cashflow_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf) {
  const int rc = check_cashflow(e, sim, cf);
  if (rc) return rc;
  return cashflow_divide(e, sim, cf);
}

int smmc_engine_simulate_cashflow(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf, float *d_final,
                                  float *d_paid, uint32_t *d_ruin_period, void *d_stats, uint64_t *d_depleted_at) {
  int rc = check_cashflow(e, sim, cf);
  if (rc) return rc;
  rc = smmc::cashflow_check_pointers(d_final, d_paid, d_ruin_period, d_stats, d_depleted_at);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  uint32_t grid = 0;
  rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kCashflowGroupsPerCU, view.max_grid, &grid);
  if (rc) return rc;
  smmc::KernelArgs a = smmc::host_make_args(e, sim);
  if (!d_stats) a.n_bins = 0;
  const size_t lds = smmc::cashflow_lds_bytes(a.mode, a.table_len, a.n_periods, a.n_bins);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "table, depletion counters and histogram need %zu bytes of LDS, device allows %zu", lds,
                     view.max_lds);
  smmc::CashflowArgs c;
  std::memset(&c, 0, sizeof c);
  c.amount = cf->amount;
  c.fraction = cf->fraction;
  c.floor = cf->floor;
  c.d_paid = d_paid;
  c.d_ruin_period = d_ruin_period;
  a.d_final = d_final;
  const bool exact_div = grid && cashflow_divide(e, sim, cf) != SMMC_DIV_FAST;
  const smmc::WaveWalk walk = {"launch_cashflow", grid, sim->n_bins, {{d_stats, 0, 0, &a.partials, &a.d_hist}},
                               {{d_depleted_at, smmc::kDepletedAt, sim->n_periods + 1u, &c.d_depleted}}};
  return smmc::host_wave_walk_run(
      e, walk, smmc::FoldRecord(), [&](hipStream_t stream) { return smmc::launch_cashflow(a, c, exact_div, grid, stream); },
      [&] { return cashflow_varying(cf) && grid ? stage_schedule(e, sim, cf, &c) : SMMC_OK; });
}

int smmc_engine_simulate_cashflow_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf, float *host_final,
                                          float *host_paid, uint32_t *host_ruin_period, void *host_stats,
                                          uint64_t *host_depleted_at) {
  int rc = check_cashflow(e, sim, cf);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  const size_t per_path = sizeof(float) * sim->n_paths;
  const smmc::HostPiece pieces[5] = {{host_stats, static_cast<size_t>(smmc_stats_bytes(sim->n_bins))},
                                     {host_depleted_at, sizeof(uint64_t) * (static_cast<size_t>(sim->n_periods) + 1u)},
                                     {host_final, per_path}, {host_paid, per_path}, {host_ruin_period, per_path}};
  return smmc::host_outputs_to_host(e, "simulate_cashflow_to_host", pieces, 5, [&](void *const *dev) {
    return smmc_engine_simulate_cashflow(e, sim, cf, static_cast<float *>(dev[2]), static_cast<float *>(dev[3]),
                                         static_cast<uint32_t *>(dev[4]), dev[0], static_cast<uint64_t *>(dev[1]));
  });
}

}  // extern "C"
