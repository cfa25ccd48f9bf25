// portfolio_cashflow_checkpoints_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp: the launch symbols of the portfolio
// cash-flow checkpoint kernel (smmc_internal.h), which that file predates, and launch_finalize_checkpoints, which no
// other host-only program needs.  TEST INFRASTRUCTURE; it simulates nothing: a launch is COUNTED
// (fake_pfcf_checkpoints_launches), what it was given is kept (the divide form, the checkpoint partials' address, the
// periods), and it reports "no device", so a request that passes every argument check of
// csrc/smmc_portfolio_cashflow_checkpoints.cpp ends as SMMC_ERR_HIP and a refused one must leave the count where it was.
// Before it fails, a launch leaves a count in every counter of the three regions of the accumulator it was given: what
// the next user of the engine must not see.  The fold of the checkpoint records is the kernel's, on the host.
#include <limits>

#include "smmc_internal.h"

static int g_launches = 0, g_last_exact = -1, g_folds = 0;
static const void *g_last_partials = nullptr;
static uint32_t g_last_n = 0, g_last_period0 = 0, g_last_pad = 0;
extern "C" int fake_pfcf_checkpoints_launches(void) { return g_launches; }
extern "C" int fake_pfcf_checkpoints_last_exact(void) { return g_last_exact; }
extern "C" int fake_pfcf_checkpoints_folds(void) { return g_folds; }
extern "C" const void *fake_pfcf_checkpoints_last_partials(void) { return g_last_partials; }
extern "C" uint32_t fake_pfcf_checkpoints_last_n(void) { return g_last_n; }
extern "C" uint32_t fake_pfcf_checkpoints_last_first_period(void) { return g_last_period0; }
extern "C" uint32_t fake_pfcf_checkpoints_last_padding(void) { return g_last_pad; }  // periods[n], or 0xffffffff when n is 64

namespace smmc {
hipError_t launch_portfolio_cashflow_checkpoints(const KernelArgs &a, const PortfolioCashflowCheckpointsArgs &x, bool exact_div, uint32_t grid,
                                                 hipStream_t) {
  ++g_launches;
  g_last_exact = exact_div ? 1 : 0;
  g_last_partials = x.ck_partials;
  g_last_n = x.n;
  g_last_period0 = x.periods[0];
  g_last_pad = x.n < SMMC_MAX_CHECKPOINTS ? x.periods[x.n] : 0xffffffffu;
  for (uint32_t b = 0; a.d_hist && b < a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose folds are never queued would
  for (uint32_t t = 0; x.c.d_depleted && t <= a.n_periods; ++t) x.c.d_depleted[t] += 1;
  for (uint32_t b = 0; x.d_ck_hist && b < x.n * a.n_bins; ++b) x.d_ck_hist[b] += 1;
  for (size_t i = 0; x.ck_partials && i < static_cast<size_t>(x.n) * grid; ++i) x.ck_partials[i].count = 1;  // the array holds n x grid
  return hipErrorNoDevice;
}
// the kernel's layout with 8 waves in Gaussian mode, 4 in table mode (walk_waves), a BlockPartial each
size_t portfolio_cashflow_checkpoints_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins,
                                                uint32_t n_checkpoints) {
  const size_t waves = mode == SMMC_MODE_TABLE ? 4u : 8u;
  const size_t table = mode == SMMC_MODE_TABLE ? static_cast<size_t>(n_rows) * portfolio_row_words(n_assets) : 9216u;
  const size_t parts = waves * n_checkpoints * (sizeof(BlockPartial) / 4u);
  const size_t front = ((table > parts ? table : parts) + 1u) & ~static_cast<size_t>(1);
  const size_t counters = static_cast<size_t>(n_periods) + 1u + n_bins + static_cast<size_t>(n_checkpoints) * n_bins;
  return ((front + counters + 1u) & ~static_cast<size_t>(1)) * 4u + waves * sizeof(BlockPartial);
}
hipError_t launch_finalize_checkpoints(const BlockPartial *partials, uint32_t n_partials, uint32_t n_checkpoints, void *d_records,
                                       uint32_t n_bins, unsigned long long *hist_acc, hipStream_t) {
  ++g_folds;
  const size_t record_bytes = sizeof(smmc_stats) + sizeof(unsigned long long) * n_bins;
  for (uint32_t k = 0; k < n_checkpoints; ++k) {
    smmc_stats *out = reinterpret_cast<smmc_stats *>(static_cast<unsigned char *>(d_records) + k * record_bytes);
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(out + 1);
    for (uint32_t b = 0; b < n_bins; ++b) {
      hist[b] = hist_acc[static_cast<size_t>(k) * n_bins + b];
      hist_acc[static_cast<size_t>(k) * n_bins + b] = 0;
    }
    out->count = out->below = out->underflow = out->overflow = 0;
    out->sum = out->sumsq = 0.0;
    out->min = std::numeric_limits<float>::infinity();
    out->max = -out->min;
    for (uint32_t j = 0; j < n_partials; ++j) {
      const BlockPartial &p = partials[static_cast<size_t>(k) * n_partials + j];
      out->count += p.count;
      out->sum += p.sum;
    }
    out->n_bins = n_bins;
    out->reserved = 0;
  }
  return hipSuccess;
}
}  // namespace smmc
