// cashflow_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp: the launch symbols of the cash-flow kernel
// (smmc_internal.h), which that file predates.  TEST INFRASTRUCTURE; it simulates nothing: a launch reports
// "no device", so a request that passes every argument check of csrc/smmc_cashflow.cpp ends as SMMC_ERR_HIP.
#include "smmc_internal.h"

namespace smmc {
hipError_t launch_cashflow(const KernelArgs &, const CashflowArgs &, bool, uint32_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_finalize_depleted(unsigned long long *, uint32_t, unsigned long long *, hipStream_t) { return hipErrorNoDevice; }
size_t cashflow_lds_bytes(int32_t, uint32_t table_len, uint32_t n_periods, uint32_t n_bins) {
  return (static_cast<size_t>(table_len) + n_periods + 1u + n_bins) * 4u;
}
}  // namespace smmc
