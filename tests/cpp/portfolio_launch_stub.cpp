// portfolio_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp: the launch symbols of the portfolio kernel
// (smmc_internal.h), which that file predates.  TEST INFRASTRUCTURE; it simulates nothing: a launch is COUNTED
// (fake_portfolio_launches) and reports "no device", so a request that passes every argument check of
// csrc/smmc_portfolio.cpp ends as SMMC_ERR_HIP and a refused one must leave the count where it was.  Before it fails, a
// launch leaves a count in every bucket of the accumulator it was given: what the next user of the engine must not see.
#include "smmc_internal.h"

static int g_launches = 0;
extern "C" int fake_portfolio_launches(void) { return g_launches; }

namespace smmc {
hipError_t launch_portfolio(const KernelArgs &a, const PortfolioArgs &, bool, uint32_t, hipStream_t) {
  ++g_launches;
  for (uint32_t b = 0; a.d_hist && b < a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose fold is never queued would
  return hipErrorNoDevice;
}
size_t portfolio_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_bins) {
  const size_t table = mode == SMMC_MODE_TABLE ? static_cast<size_t>(n_rows) * portfolio_row_words(n_assets) : 9216u;
  return (table + n_bins) * 4u;
}
}  // namespace smmc
