// portfolio_cashflow_stationary_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp: the launch symbols of the
// stationary-bootstrap plan's kernel (smmc_internal.h).  TEST INFRASTRUCTURE; it simulates nothing: a launch is COUNTED
// (fake_portfolio_cashflow_stationary_launches), its divide form and renewal probability kept, and it reports "no device",
// so a request that passes every argument check of csrc/smmc_portfolio_cashflow_stationary.cpp ends as SMMC_ERR_HIP and a
// refused one must leave the count where it was.  portfolio_cashflow_stationary_stub_extra_lds raises the LDS need, to
// reach the refusal that no valid request reaches on a device the library runs on.
#include "smmc_internal.h"

static int g_launches = 0, g_last_exact = -1;
static uint32_t g_last_renew = 0xffffffffu;
extern "C" int fake_portfolio_cashflow_stationary_launches(void) { return g_launches; }
extern "C" int fake_portfolio_cashflow_stationary_last_exact(void) { return g_last_exact; }
extern "C" uint32_t fake_portfolio_cashflow_stationary_last_renew(void) { return g_last_renew; }

namespace smmc {
size_t portfolio_cashflow_stationary_stub_extra_lds = 0;
hipError_t launch_portfolio_cashflow_geometric(const KernelArgs &a, const PortfolioCashflowStationaryArgs &x, bool exact_div, uint32_t,
                                                hipStream_t) {
  ++g_launches;
  g_last_exact = exact_div ? 1 : 0;
  g_last_renew = x.renew_q16;
  for (uint32_t b = 0; a.d_hist && b < a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose fold is never queued would
  for (uint32_t t = 0; x.c.d_depleted && t <= a.n_periods; ++t) x.c.d_depleted[t] += 1;
  return hipErrorNoDevice;
}
// the kernels' own layout (smmc_kernels.hip): the rows, the counters, the pad to 8 bytes, one 56-byte partial per wave
size_t portfolio_cashflow_geometric_lds_bytes(uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins) {
  const size_t words = static_cast<size_t>(n_rows) * portfolio_row_words(n_assets) + n_periods + 1u + n_bins;
  return ((words + 1u) & ~static_cast<size_t>(1)) * 4u + 4u * sizeof(BlockPartial) + portfolio_cashflow_stationary_stub_extra_lds;
}
}  // namespace smmc
