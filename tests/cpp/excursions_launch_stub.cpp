// excursions_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and tests/cpp/cashflow_launch_stub.cpp: the launch
// symbols of the excursions kernel (smmc_internal.h), which those files predate.  TEST INFRASTRUCTURE; it simulates
// nothing: a launch reports "no device", so a request that passes every argument check of
// csrc/smmc_excursions.cpp ends as SMMC_ERR_HIP.
#include "smmc_internal.h"

namespace smmc {
hipError_t launch_excursions(const KernelArgs &, const ExcursionArgs &, bool, uint32_t, hipStream_t) { return hipErrorNoDevice; }
size_t excursions_lds_bytes(int32_t, uint32_t table_len, uint32_t n_periods, uint32_t n_bins) {
  return (static_cast<size_t>(table_len) + 2u * (static_cast<size_t>(n_periods) + 1u) + 2u * static_cast<size_t>(n_bins)) * 4u;
}
}  // namespace smmc
