// sweep_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and tests/cpp/cashflow_launch_stub.cpp: the launch symbols
// of the cash-flow sweep kernel (smmc_internal.h), which those files predate.  TEST INFRASTRUCTURE; it simulates
// nothing: a launch reports "no device", so a request that passes every argument check of csrc/smmc_sweep.cpp ends as
// SMMC_ERR_HIP.  sweep_stub_launches() counts the launches that got that far.
#include "smmc_internal.h"

static int g_launches = 0;
extern "C" int sweep_stub_launches() { return g_launches; }

namespace smmc {
hipError_t launch_cashflow_sweep(const KernelArgs &, const SweepArgs &, bool, uint32_t, hipStream_t) {
  ++g_launches;
  return hipErrorNoDevice;
}
hipError_t launch_finalize_sweep(const BlockPartial *, uint32_t, uint32_t, void *, uint32_t, unsigned long long *, hipStream_t) {
  return hipErrorNoDevice;
}
size_t cashflow_sweep_lds_bytes(int32_t, uint32_t table_len, uint32_t n_periods, uint32_t n_bins, uint32_t n_scenarios) {
  return (static_cast<size_t>(table_len) + static_cast<size_t>(n_scenarios) * (n_periods + 1u + n_bins)) * 4u;
}
}  // namespace smmc
