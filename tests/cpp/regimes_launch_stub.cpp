// regimes_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and the other launch stubs: the launch symbols of the
// regime-switching kernel (smmc_internal.h), which those files predate.  TEST INFRASTRUCTURE; it simulates nothing: a
// launch reports "no device", so a request that passes every argument check of csrc/smmc_regimes.cpp ends as
// SMMC_ERR_HIP.
#include "smmc_internal.h"

namespace smmc {
// The draw tables and the largest histogram fit every device's LDS, so the refusal of a need beyond it is reached from
// here: tests/cpp/regimes_args.cpp raises the need by this many bytes for one case.
size_t regimes_stub_extra_lds = 0;
hipError_t launch_regimes(const KernelArgs &, const RegimeArgs &, int, uint32_t, hipStream_t) { return hipErrorNoDevice; }
size_t regimes_lds_bytes(uint32_t n_bins) { return 36u * 1024u + static_cast<size_t>(n_bins) * 4u + 512u + regimes_stub_extra_lds; }
}  // namespace smmc
