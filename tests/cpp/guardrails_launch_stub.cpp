// guardrails_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp: the launch symbols of the guardrails kernel
// (smmc_internal.h).  TEST INFRASTRUCTURE; it simulates nothing: a launch is COUNTED (fake_guardrails_launches), the
// arguments it was given are KEPT (fake_guardrails_last_kernel_args, fake_guardrails_last_args: what the host unit
// staged), and it reports "no device", so a request that passes every argument check of csrc/smmc_guardrails.cpp ends
// as SMMC_ERR_HIP and a refused one must leave the count where it was.  Before it fails, a launch leaves a count in every
// bucket and counter of the accumulator it was given: what the next user of the engine must not see.
#include "smmc_internal.h"

static int g_launches = 0;
static smmc::KernelArgs g_kernel_args;
static smmc::GuardrailsArgs g_args;
extern "C" int fake_guardrails_launches(void) { return g_launches; }
extern "C" const void *fake_guardrails_last_kernel_args(void) { return &g_kernel_args; }
extern "C" const void *fake_guardrails_last_args(void) { return &g_args; }

namespace smmc {
hipError_t launch_guardrails(const KernelArgs &a, const GuardrailsArgs &x, uint32_t, hipStream_t) {
  ++g_launches;
  g_kernel_args = a;
  g_args = x;
  for (uint32_t b = 0; a.d_hist && b < a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose fold is never queued would
  for (unsigned long long *counts : {x.d_depleted, x.d_cuts_at, x.d_raises_at})
    for (uint32_t t = 0; counts && t <= a.n_periods; ++t) counts[t] += 1;
  return hipErrorNoDevice;
}
size_t guardrails_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins) {
  const size_t table = mode == SMMC_MODE_TABLE ? static_cast<size_t>(n_rows) * portfolio_row_words(n_assets) : 9216u;
  return (table + 3u * (static_cast<size_t>(n_periods) + 1u) + n_bins) * 4u;
}
}  // namespace smmc
