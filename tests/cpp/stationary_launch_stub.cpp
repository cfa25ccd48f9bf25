// stationary_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and the other launch stubs: the launch symbols of the
// stationary-bootstrap kernel (smmc_internal.h), which those files predate.  TEST INFRASTRUCTURE; it simulates nothing:
// a launch reports "no device", so a request that passes every argument check of csrc/smmc_stationary.cpp ends as
// SMMC_ERR_HIP.
#include "smmc_internal.h"

namespace smmc {
// The largest table and histogram an engine accepts fit every device's LDS, so the refusal of a need beyond it is reached
// from here: tests/cpp/stationary_args.cpp raises the need by this many bytes for one case.
size_t stationary_stub_extra_lds = 0;
hipError_t launch_stationary(const KernelArgs &, uint32_t, int, uint32_t, hipStream_t) { return hipErrorNoDevice; }
size_t stationary_lds_bytes(uint32_t table_len, uint32_t n_bins) {
  return static_cast<size_t>(table_len) * 4u + static_cast<size_t>(n_bins) * 4u + 512u + stationary_stub_extra_lds;
}
}  // namespace smmc
