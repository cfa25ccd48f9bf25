// smmc_host.h -- what the library's host translation units share and no kernel translation unit sees: ONE statement
// of the host-buffer pinning rules (engine smmc_capi.cpp, group smmc_group.cpp, C++ drop-in smmc_dropin.cpp), the
// owner of device and page-locked memory, and the lease on an array that is zero between launches.  Not installed.
//
// Round 3 had three copies of these rules that had drifted apart: the group hard-coded the
// threshold and tested only a buffer's first byte for "already pinned", the drop-in treated SMMC_PIN_HOST=chunk
// as "whole".  The reference pins its result with cudaMallocHost (src/simulations.cu:591-592); here the
// caller owns the buffer, so it is page-locked in place (hipHostRegister) for the duration of a call.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <utility>

struct smmc_engine;

namespace smmc {

// SMMC_PIN_HOST: "0" (anything else than the words below) never; "1" / "whole" (default) the whole buffer up
// front; "chunk" chunk by chunk, one chunk ahead of the copies (every page has one owning chunk).
enum PinPolicy : int { kPinNever = 0, kPinWhole = 1, kPinChunk = 2 };
PinPolicy pin_policy_from_env();

// a result smaller than this is copied through the pageable path: registering costs more than it saves
constexpr uint64_t kPinMinBytes = 32ull << 20;

// Are BOTH ends of [p, p + bytes) in memory the runtime knows as page-locked already (hipHostMalloc'd or
// registered)?  A buffer pinned only at its front is not "pinned".
bool host_range_is_pinned(const void *p, uint64_t bytes);

// Owns one device allocation (Pinned = true: one page-locked host allocation) and its capacity: freed by the
// destructor, which needs the device current; movable, not copyable.
template <typename T = void, bool Pinned = false>
struct DeviceBuffer {
  T *p = nullptr;
  size_t bytes = 0;  // capacity
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DeviceBuffer() { (void)release(); }
  hipError_t release() {
    const hipError_t err = !p ? hipSuccess : Pinned ? hipHostFree(p) : hipFree(p);
    if (err == hipSuccess) p = nullptr, bytes = 0;
    return err;
  }
  // At least `want` bytes: at once when the capacity suffices (a steady-state call makes no HIP call here).  Otherwise
  // the old array goes first -- after *drain has run dry where an earlier launch may still read it; null where the
  // caller knows that none does (the engine's stream may itself be the null stream, hence a pointer) -- and a failed
  // allocation leaves the buffer empty.
  hipError_t reserve(size_t want, const hipStream_t *drain) {
    if (want <= bytes) return hipSuccess;
    hipError_t err = drain ? hipStreamSynchronize(*drain) : hipSuccess;
    if (err == hipSuccess) err = release();
    if (err != hipSuccess) return err;
    void *q = nullptr;
    err = Pinned ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
    if (err != hipSuccess) return err;
    p = static_cast<T *>(q);
    bytes = want;
    return hipSuccess;
  }
};
template <typename T>
using PinnedBuffer = DeviceBuffer<T, true>;

// A device array that is ZERO between launches: the kernel of a launch adds into it, the launch's finalize folds the
// counts away and leaves zeros, so nothing is cleared per call.  `dirty`: an enqueue failed between a kernel and its
// finalize, counts may be left -- the next lease clears the array first.
struct ZeroedArray {
  DeviceBuffer<unsigned long long> mem;
  bool dirty = false;
};
// The ONE statement of that protocol.  take(): the array exists (allocated on first use) and is zero (cleared on
// `stream` if dirty), and is marked dirty; finalize_queued(): the finalize that zeroes it again is in the queue, the
// mark comes off.  A lease dropped in between -- an error return -- leaves the mark on; a call that takes no lease
// never touches it.
struct ZeroLease {
  ZeroedArray *array = nullptr;
  hipError_t take(ZeroedArray &a, size_t bytes, hipStream_t stream) {
    if (!a.mem.p) a.dirty = true;
    hipError_t err = a.mem.reserve(bytes, nullptr);  // allocated once, never grown: nothing to drain
    if (err == hipSuccess && a.dirty) err = hipMemsetAsync(a.mem.p, 0, bytes, stream);
    if (err != hipSuccess) return err;
    a.dirty = true;
    array = &a;
    return hipSuccess;
  }
  unsigned long long *acc() const { return array ? array->mem.p : nullptr; }  // null: not taken
  void finalize_queued() {
    if (array) array->dirty = false;
    array = nullptr;
  }
};
// A lease on the engine's accumulator (kHistSpread x SMMC_MAX_BINS counters, smmc_capi.cpp) for the library's other
// host translation units; the device must be current.
int engine_acc_lease(smmc_engine *e, ZeroLease *lease);

}  // namespace smmc
