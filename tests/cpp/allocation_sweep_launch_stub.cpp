// allocation_sweep_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and the other launch stubs: the launch symbols of
// the allocation-sweep kernel (smmc_internal.h), which those files predate.  TEST INFRASTRUCTURE; it simulates nothing: a
// launch is COUNTED (fake_allocation_sweep_launches), its divide form and its scenario arguments kept
// (fake_allocation_sweep_last_exact, fake_allocation_sweep_last_args), and it reports "no device", so a request that passes
// every argument check of csrc/smmc_allocation_sweep.cpp ends as SMMC_ERR_HIP and a refused one must leave the count where
// it was.  Before it fails, a launch leaves a count in every bucket and depletion counter of the accumulator it was given:
// what the next user of the engine must not see.
#include "smmc_internal.h"

static int g_launches = 0, g_last_exact = -1;
static smmc::AllocationSweepArgs g_last;
extern "C" int fake_allocation_sweep_launches(void) { return g_launches; }
extern "C" int fake_allocation_sweep_last_exact(void) { return g_last_exact; }
extern "C" const void *fake_allocation_sweep_last_args(void) { return &g_last; }

namespace smmc {
hipError_t launch_allocation_sweep(const KernelArgs &a, const AllocationSweepArgs &x, bool exact_div, uint32_t, hipStream_t) {
  ++g_launches;
  g_last_exact = exact_div ? 1 : 0;
  g_last = x;
  for (uint32_t b = 0; a.d_hist && b < x.n * a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose fold is never queued would
  for (uint32_t t = 0; x.d_depleted && t < x.n * (a.n_periods + 1u); ++t) x.d_depleted[t] += 1;
  return hipErrorNoDevice;
}
size_t allocation_sweep_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins,
                                  uint32_t n_scenarios) {
  const size_t table = mode == SMMC_MODE_TABLE ? static_cast<size_t>(n_rows) * portfolio_row_words(n_assets) : 9216u;
  return (table + static_cast<size_t>(n_scenarios) * (n_periods + 1u + n_bins)) * 4u +
         allocation_sweep_width(n_scenarios) * (mode == SMMC_MODE_TABLE ? 4u : 8u) * sizeof(BlockPartial);
}
}  // namespace smmc
