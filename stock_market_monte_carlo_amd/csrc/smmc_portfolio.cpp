// smmc_portfolio.cpp -- smmc_engine_set_asset_table, smmc_engine_simulate_portfolio, its _to_host form and
// smmc_engine_portfolio_divide_kind (include/smmc.h): K jointly drawn assets per path, held with weights and
// rebalanced every R periods.
//
// A translation unit of its own, as smmc_cashflow.cpp and smmc_blocks.cpp: smmc_capi.cpp owns struct smmc_engine and
// never calls into this file; what is needed of an engine comes through smmc_host.h.  What this file keeps per engine
// -- the joint table and its columns' extremes -- hangs in this unit's extension slot of the engine (engine_ext),
// released by smmc_engine_destroy.  The launch is a wave walk and its run the shared one (smmc_host.h,
// host_wave_walk_run) with one record and no count array.  What is this unit's own: the asset table, the portfolio's
// checks, the divide rule, the LDS need and the kernel arguments.  The reference simulates one return series per path;
// it has no portfolio.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "smmc_host.h"

namespace {

using smmc::DeviceGuard;
using smmc::host_fail;

constexpr uint32_t kK = SMMC_MAX_ASSETS;
// Workgroups per CU, as cashflow_kernel: a workgroup flushes n_bins counters.
constexpr uint32_t kPortfolioGroupsPerCU = 32;

// The joint table of an engine: rows of portfolio_row_words(n_assets) words, a = 100.0f + r, padding 0.
struct PortfolioState {
  smmc::DeviceBuffer<float> d_table;
  uint32_t n_rows = 0, n_assets = 0;
  float min_a[kK] = {0, 0, 0, 0}, max_a[kK] = {0, 0, 0, 0};  // per column
  bool finite = false;
};
const char kOwner = 0;  // its address names this unit's slot among the engine's (engine_ext)

void release_state(void *p) { delete static_cast<PortfolioState *>(p); }  // the device is current (smmc_engine_destroy)

const PortfolioState *state_of(const smmc_engine *e) {
  // engine_ext claims a free slot for an owner it has not seen; an engine without an asset table then keeps an empty slot
  smmc::EngineExt *ext = smmc::engine_ext(const_cast<smmc_engine *>(e), &kOwner);
  return ext ? static_cast<const PortfolioState *>(ext->state) : nullptr;
}

int check_portfolio(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf) {
  if (!e) return host_fail(SMMC_ERR_INVALID, "engine is NULL");
  // host_check_sim asks table mode for the single-series table, which a portfolio does not read: its other checks
  // are put to a copy in Gaussian mode (SMMC_FLAG_STREAM_REF, whose check names the mode, is refused below)
  const bool table = sim && sim->struct_size == sizeof(smmc_sim) && sim->mode == SMMC_MODE_TABLE;
  smmc_sim probe;
  if (table) {
    probe = *sim;
    probe.mode = SMMC_MODE_GAUSSIAN;
    probe.flags &= ~static_cast<uint32_t>(SMMC_FLAG_STREAM_REF);
  }
  int rc = smmc::host_check_sim(e, table ? &probe : sim);
  if (rc) return rc;
  rc = smmc::host_require_v3(sim, "portfolios support");
  if (rc) return rc;
  if (!pf) return host_fail(SMMC_ERR_INVALID, "the smmc_portfolio argument is NULL");
  if (pf->struct_size != sizeof(smmc_portfolio))
    return host_fail(SMMC_ERR_INVALID, "smmc_portfolio.struct_size is %u, this library expects %zu", pf->struct_size,
                     sizeof(smmc_portfolio));
  const uint32_t K = pf->n_assets;
  if (K == 0 || K > kK) return host_fail(SMMC_ERR_INVALID, "n_assets is %u: 1 .. SMMC_MAX_ASSETS (%d)", K, SMMC_MAX_ASSETS);
  if (pf->reserved != 0) return host_fail(SMMC_ERR_INVALID, "smmc_portfolio.reserved is %u, it must be 0", pf->reserved);
  double sum = 0.0;
  for (uint32_t k = 0; k < kK; ++k) {
    const float w = pf->weights[k];
    if (!std::isfinite(w) || w < 0.0f)
      return host_fail(SMMC_ERR_INVALID, "weights[%u] is %g: a weight is finite and >= 0", k, static_cast<double>(w));
    if (k >= K && w != 0.0f)
      return host_fail(SMMC_ERR_INVALID, "weights[%u] is %g beyond n_assets = %u: it must be 0", k, static_cast<double>(w), K);
    sum += static_cast<double>(w);
  }
  if (!(std::fabs(sum - 1.0) <= 1e-6)) return host_fail(SMMC_ERR_INVALID, "the weights sum to %.9g, not to 1 within 1e-6", sum);
  if (sim->mode == SMMC_MODE_TABLE) {
    for (uint32_t k = 0; k < kK; ++k)
      if (pf->means[k] != 0.0f || std::isnan(pf->means[k]))
        return host_fail(SMMC_ERR_INVALID, "means[%u] is set in table mode: the Gaussian fields must be 0", k);
    for (uint32_t i = 0; i < kK * kK; ++i)
      if (pf->factor[i] != 0.0f || std::isnan(pf->factor[i]))
        return host_fail(SMMC_ERR_INVALID, "factor[%u] is set in table mode: the Gaussian fields must be 0", i);
    const PortfolioState *st = state_of(e);
    if (!st || st->n_rows == 0) return host_fail(SMMC_ERR_INVALID, "a table-mode portfolio needs smmc_engine_set_asset_table first");
    if (st->n_assets != K)
      return host_fail(SMMC_ERR_INVALID, "the asset table has %u columns, the portfolio n_assets = %u", st->n_assets, K);
  } else {
    for (uint32_t k = 0; k < kK; ++k) {
      if (!std::isfinite(pf->means[k])) return host_fail(SMMC_ERR_INVALID, "means[%u] is not finite", k);
      if (k >= K && pf->means[k] != 0.0f) return host_fail(SMMC_ERR_INVALID, "means[%u] is set beyond n_assets = %u: it must be 0", k, K);
      for (uint32_t j = 0; j < kK; ++j) {
        const float l = pf->factor[k * kK + j];
        if (!std::isfinite(l)) return host_fail(SMMC_ERR_INVALID, "factor[%u][%u] is not finite", k, j);
        if ((j > k || k >= K) && l != 0.0f)
          return host_fail(SMMC_ERR_INVALID, "factor[%u][%u] is %g: entries above the diagonal and beyond n_assets = %u must be 0", k, j,
                           static_cast<double>(l), K);
        if (j == k && l < 0.0f) return host_fail(SMMC_ERR_INVALID, "factor[%u][%u] is %g: the diagonal must be >= 0", k, j, static_cast<double>(l));
      }
    }
  }
  return SMMC_OK;
}

// Bounds on asset k's multiplier a_k; false if there are none that keep it positive.
bool asset_bounds(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, uint32_t k, double *lo_a, double *hi_a) {
  if (sim->mode == SMMC_MODE_TABLE) {
    const PortfolioState *st = state_of(e);
    if (!st || !st->finite) return false;
    *lo_a = st->min_a[k];
    *hi_a = st->max_a[k];
    return *lo_a > 0.0 && std::isfinite(*hi_a);
  }
  // s_k -+ Zmax * sum_j |L[k][j]|: the single-series rule for the mean means[k] and that sum as the deviation
  smmc_sim one = *sim;
  double spread = 0.0;
  for (uint32_t j = 0; j <= k; ++j) spread += std::fabs(static_cast<double>(pf->factor[k * kK + j]));
  one.gauss_mean = pf->means[k];
  one.gauss_std = std::nextafter(static_cast<float>(spread), std::numeric_limits<float>::infinity());  // rounded up
  return smmc::host_multiplier_bounds(e, &one, lo_a, hi_a);
}

// The rule of include/smmc.h (smmc_engine_portfolio_divide_kind); DESIGN.md, "Portfolios", has the proof.
int portfolio_divide(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf) {
  if (sim->flags & SMMC_FLAG_EXACT_DIV) return SMMC_DIV_EXACT;
  const double cap = sim->initial_capital;
  if (!(cap > 0.0) || !std::isfinite(cap)) return SMMC_DIV_EXACT;
  double lo_min = INFINITY, hi_max = 0.0, w_min = INFINITY, h_min = INFINITY;
  for (uint32_t k = 0; k < pf->n_assets; ++k) {
    double lo_a, hi_a;
    if (!asset_bounds(e, sim, pf, k, &lo_a, &hi_a)) return SMMC_DIV_EXACT;
    lo_min = std::min(lo_min, lo_a);
    hi_max = std::max(hi_max, hi_a);
    const float h0 = sim->initial_capital * pf->weights[k];  // the kernel's own first holding
    if (pf->weights[k] > 0.0f) w_min = std::min(w_min, static_cast<double>(pf->weights[k]));
    if (h0 > 0.0f) h_min = std::min(h_min, static_cast<double>(h0));
  }
  if (!std::isfinite(w_min) || !std::isfinite(h_min)) return SMMC_DIV_EXACT;  // nothing is held
  const double p = sim->n_periods;
  const double grow = std::max(0.0, std::log2(hi_max / 100.0)), shrink = std::max(0.0, -std::log2(lo_min / 100.0));
  // the roundings along a path: four per period (product, quotient, a share of the sum and of the weight product),
  // each within 2^-24 relative, move a logarithm by less than 2^-21 per period; one bit more on each side
  const double slack = 1.0 + p * 0x1p-21;
  // above: no holding exceeds the value, the value never exceeds cap grown by the best asset in every period
  if (!(std::log2(cap) + p * grow + std::log2(hi_max) + slack < 127.0)) return SMMC_DIV_EXACT;
  // below: a positive holding started as the smallest positive initial holding, or as the smallest positive weight's
  // share of a value that is at least cap shrunk by the worst asset in every period so far; it shrinks no faster since
  const double start = std::min(std::log2(h_min), std::log2(w_min) + std::log2(cap));
  if (!(start - p * shrink + std::min(0.0, std::log2(lo_min)) - slack > -89.0)) return SMMC_DIV_EXACT;
  return SMMC_DIV_FAST;
}

// The launch's arguments and LDS need, and the refusals that follow from them; asked before any device work.
struct Plan {
  smmc::KernelArgs a;
  smmc::PortfolioArgs p;
  uint32_t grid;
};
void launch_args(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, smmc::KernelArgs *args, smmc::PortfolioArgs *pa) {
  smmc::KernelArgs &a = *args;
  a = smmc::host_make_args(e, sim);
  a.table_a = nullptr;
  a.table_len = 0;
  if (sim->mode == SMMC_MODE_TABLE) {
    const PortfolioState *st = state_of(e);
    a.table_a = st->d_table.p;
    a.table_len = st->n_rows;
  }
  a.gauss_mean = 0.0f;  // the staged draw yields standard normals: scale 1, shift 0
  a.gauss_std = 1.0f;
  a.gauss_shift100 = 0.0f;
  smmc::PortfolioArgs &p = *pa;
  std::memset(&p, 0, sizeof p);
  p.n_assets = pf->n_assets;
  p.rebalance_every = pf->rebalance_every;
  for (uint32_t k = 0; k < kK; ++k) {
    p.weights[k] = pf->weights[k];
    p.shift100[k] = 100.0f + pf->means[k];
  }
  std::memcpy(p.factor, pf->factor, sizeof p.factor);
}
int plan(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, bool want_stats, Plan *out) {
  const smmc::EngineView view = smmc::engine_view(e);
  int rc = smmc::host_wave_walk_grid(view, sim->n_paths, smmc::wave_walk_group_paths(sim->mode), kPortfolioGroupsPerCU, view.max_grid,
                                     &out->grid);
  if (rc) return rc;
  launch_args(e, sim, pf, &out->a, &out->p);
  smmc::KernelArgs &a = out->a;
  if (!want_stats) a.n_bins = 0;
  const smmc::PortfolioArgs &p = out->p;
  const size_t lds = smmc::portfolio_lds_bytes(a.mode, a.table_len, p.n_assets, a.n_bins);
  if (lds + 2048 > view.max_lds)
    return host_fail(SMMC_ERR_INVALID, "asset table, histogram and partials need %zu bytes of LDS, device allows %zu", lds, view.max_lds);
  return SMMC_OK;
}

}  // namespace

namespace smmc {  // what smmc_portfolio_cashflow.cpp takes of this unit (smmc_host.h)
int portfolio_check(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf) { return check_portfolio(e, sim, pf); }
bool portfolio_asset_bounds(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, uint32_t k, double *lo_a, double *hi_a) {
  return asset_bounds(e, sim, pf, k, lo_a, hi_a);
}
void portfolio_launch_args(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, KernelArgs *a, PortfolioArgs *p) {
  launch_args(e, sim, pf, a, p);
}
}  // namespace smmc

extern "C" {

int smmc_engine_set_asset_table(smmc_engine *e, const float *returns_percent, uint32_t n_rows, uint32_t n_assets) {
  if (!e) return host_fail(SMMC_ERR_INVALID, "engine is NULL");
  if (!returns_percent || n_rows == 0) return host_fail(SMMC_ERR_INVALID, "empty asset table");
  if (n_assets == 0 || n_assets > kK) return host_fail(SMMC_ERR_INVALID, "n_assets is %u: 1 .. SMMC_MAX_ASSETS (%d)", n_assets, SMMC_MAX_ASSETS);
  if (static_cast<uint64_t>(n_rows) * n_assets > SMMC_MAX_TABLE)
    return host_fail(SMMC_ERR_INVALID, "asset table of %u x %u entries exceeds SMMC_MAX_TABLE %d", n_rows, n_assets, SMMC_MAX_TABLE);
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  smmc::EngineExt *ext = smmc::engine_ext(e, &kOwner);
  if (!ext) return host_fail(SMMC_ERR_INVALID, "the engine has no extension slot left for the asset table");
  if (!ext->state) {
    PortfolioState *fresh = new (std::nothrow) PortfolioState();
    if (!fresh) return host_fail(SMMC_ERR_NOMEM, "out of host memory");
    ext->state = fresh;
    ext->release = release_state;
  }
  PortfolioState *st = static_cast<PortfolioState *>(ext->state);
  // a = 100.0f + r as smmc_engine_set_table forms it; rows padded to 1, 2 or 4 words
  const uint32_t row = smmc::portfolio_row_words(n_assets);
  std::vector<float> a(static_cast<size_t>(n_rows) * row, 0.0f);
  float lo[kK], hi[kK];
  for (uint32_t k = 0; k < kK; ++k) lo[k] = std::numeric_limits<float>::infinity(), hi[k] = -lo[k];
  bool finite = true;
  for (uint32_t i = 0; i < n_rows; ++i)
    for (uint32_t k = 0; k < n_assets; ++k) {
      const float v = 100.0f + returns_percent[static_cast<size_t>(i) * n_assets + k];
      a[static_cast<size_t>(i) * row + k] = v;
      finite = finite && std::isfinite(v);
      lo[k] = std::min(lo[k], v);
      hi[k] = std::max(hi[k], v);
    }
  SMMC_HIP(hipStreamSynchronize(view.stream));  // the previous table may still be read by enqueued kernels
  st->n_rows = 0;
  SMMC_HIP(st->d_table.reserve(sizeof(float) * a.size(), nullptr));
  SMMC_HIP(hipMemcpyAsync(st->d_table.p, a.data(), sizeof(float) * a.size(), hipMemcpyHostToDevice, view.stream));
  SMMC_HIP(hipStreamSynchronize(view.stream));  // `a` is a local
  st->n_rows = n_rows;
  st->n_assets = n_assets;
  st->finite = finite;
  for (uint32_t k = 0; k < kK; ++k) st->min_a[k] = lo[k], st->max_a[k] = hi[k];
  return SMMC_OK;
}

int smmc_engine_portfolio_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf) {
  const int rc = check_portfolio(e, sim, pf);
  if (rc) return rc;
  return portfolio_divide(e, sim, pf);
}

int smmc_engine_simulate_portfolio(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_portfolio_outputs *out) {
  int rc = check_portfolio(e, sim, pf);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_outputs");
  if (rc) return rc;
  if (smmc::host_misaligned({out->d_final, out->d_holdings}, 4)) return host_fail(SMMC_ERR_INVALID, "d_final and d_holdings must be 4-byte aligned");
  if (smmc::host_misaligned({out->d_stats}, 8)) return host_fail(SMMC_ERR_INVALID, "d_stats must be 8-byte aligned");
  Plan pl;
  rc = plan(e, sim, pf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  pl.a.d_final = out->d_final;
  pl.p.d_holdings = out->d_holdings;
  const bool exact_div = pl.grid && portfolio_divide(e, sim, pf) != SMMC_DIV_FAST;
  // no count array: the accumulator is leased only for a histogram
  const smmc::WaveWalk walk = {"launch_portfolio", pl.grid, sim->n_bins, {{out->d_stats, 0, 0, &pl.a.partials, &pl.a.d_hist}}, {}};
  return smmc::host_wave_walk_run(e, walk, smmc::FoldRecord(),
                                  [&](hipStream_t stream) { return smmc::launch_portfolio(pl.a, pl.p, exact_div, pl.grid, stream); });
}

int smmc_engine_simulate_portfolio_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                           const smmc_portfolio_outputs *out) {
  int rc = check_portfolio(e, sim, pf);
  if (rc) return rc;
  rc = smmc::host_check_outputs(out, "smmc_portfolio_outputs");
  if (rc) return rc;
  Plan pl;  // refuse before anything is allocated
  rc = plan(e, sim, pf, out->d_stats != nullptr, &pl);
  if (rc) return rc;
  const smmc::EngineView view = smmc::engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  typedef smmc_portfolio_outputs O;
  const size_t per_path = sizeof(float) * sim->n_paths;
  const smmc::OutputField fields[3] = {{offsetof(O, d_stats), static_cast<size_t>(smmc_stats_bytes(sim->n_bins))},
                                       {offsetof(O, d_final), per_path},
                                       {offsetof(O, d_holdings), per_path * pf->n_assets}};
  return smmc::host_outputs_struct_to_host(e, "simulate_portfolio_to_host", *out, fields,
                                           [&](const O *d) { return smmc_engine_simulate_portfolio(e, sim, pf, d); });
}

}  // extern "C"
