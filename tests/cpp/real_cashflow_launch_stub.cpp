// real_cashflow_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and tests/cpp/portfolio_cashflow_launch_stub.cpp (whose
// portfolio_cashflow_lds_bytes csrc/smmc_real_cashflow.cpp asks at the law's width): the launch symbol of the real
// cash-flow kernel (smmc_internal.h).  TEST INFRASTRUCTURE; it simulates nothing: a launch is COUNTED
// (fake_real_cashflow_launches), its divide form kept (fake_real_cashflow_last_exact), and it reports "no device", so a
// request that passes every argument check of csrc/smmc_real_cashflow.cpp ends as SMMC_ERR_HIP and a refused one must
// leave the count where it was.  Before it fails, a launch leaves a count in every bucket and depletion counter of the
// accumulator it was given: what the next user of the engine must not see.
#include "smmc_internal.h"

static int g_launches = 0, g_last_exact = -1;
extern "C" int fake_real_cashflow_launches(void) { return g_launches; }
extern "C" int fake_real_cashflow_last_exact(void) { return g_last_exact; }

namespace smmc {
hipError_t launch_real_cashflow(const KernelArgs &a, const RealCashflowArgs &x, bool exact_div, uint32_t, hipStream_t) {
  ++g_launches;
  g_last_exact = exact_div ? 1 : 0;
  for (uint32_t b = 0; a.d_hist && b < a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose fold is never queued would
  for (uint32_t t = 0; x.c.d_depleted && t <= a.n_periods; ++t) x.c.d_depleted[t] += 1;
  return hipErrorNoDevice;
}
}  // namespace smmc
