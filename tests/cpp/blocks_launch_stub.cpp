// blocks_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and the cash-flow and excursion launch stubs: the launch
// symbols of the block-bootstrap kernel (smmc_internal.h), which those files predate.  TEST INFRASTRUCTURE; it
// simulates nothing: a launch reports "no device", so a request that passes every argument check of
// csrc/smmc_blocks.cpp ends as SMMC_ERR_HIP.
#include "smmc_internal.h"

namespace smmc {
hipError_t launch_blocks(const KernelArgs &, uint32_t, bool, int, uint32_t, hipStream_t) { return hipErrorNoDevice; }
size_t blocks_lds_bytes(uint32_t table_len, uint32_t n_bins, bool wide) {
  return (static_cast<size_t>(table_len) + 8u) * (wide ? 16u : 4u) + static_cast<size_t>(n_bins) * 4u + 512u;
}
}  // namespace smmc
