// portfolio_cashflow_regimes_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp: the launch symbols of the
// regime-switching plan's kernel (smmc_internal.h).  TEST INFRASTRUCTURE; it simulates nothing: a launch is COUNTED
// (fake_portfolio_cashflow_regimes_launches), its divide form and start1_q16 kept, and it reports "no device", so a
// request that passes every argument check of csrc/smmc_portfolio_cashflow_regimes.cpp ends as SMMC_ERR_HIP and a refused
// one must leave the count where it was.  portfolio_cashflow_regimes_stub_extra_lds raises the LDS need, to reach the
// refusal that no valid request reaches on a device the library runs on.
#include "smmc_internal.h"

static int g_launches = 0, g_last_exact = -1;
static uint32_t g_last_start = 0xffffffffu;
extern "C" int fake_portfolio_cashflow_regimes_launches(void) { return g_launches; }
extern "C" int fake_portfolio_cashflow_regimes_last_exact(void) { return g_last_exact; }
extern "C" uint32_t fake_portfolio_cashflow_regimes_last_start(void) { return g_last_start; }

namespace smmc {
size_t portfolio_cashflow_regimes_stub_extra_lds = 0;
hipError_t launch_portfolio_cashflow_markov(const KernelArgs &a, const PortfolioCashflowMarkovArgs &x, bool exact_div, uint32_t, hipStream_t) {
  ++g_launches;
  g_last_exact = exact_div ? 1 : 0;
  g_last_start = x.start1_q16;
  for (uint32_t b = 0; a.d_hist && b < a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose fold is never queued would
  for (uint32_t t = 0; x.c.d_depleted && t <= a.n_periods; ++t) x.c.d_depleted[t] += 1;
  return hipErrorNoDevice;
}
// as tests/cpp/regimes_launch_stub.cpp: 36 KiB stand for the v3 draw tables; then the counters and one 56-byte partial per wave
size_t portfolio_cashflow_markov_lds_bytes(uint32_t n_periods, uint32_t n_bins) {
  return 36u * 1024u + (static_cast<size_t>(n_periods) + 2u + n_bins) * 4u + 8u * sizeof(BlockPartial) + portfolio_cashflow_regimes_stub_extra_lds;
}
}  // namespace smmc
