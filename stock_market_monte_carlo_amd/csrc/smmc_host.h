// smmc_host.h -- what the library's host translation units share and no kernel translation unit sees: ONE statement
// of the host-buffer pinning rules (engine smmc_capi.cpp, group smmc_group.cpp, C++ drop-in smmc_dropin.cpp), the
// owner of device and page-locked memory, the lease on an array that is zero between launches, what smmc_capi.cpp
// shares with the feature units (engine_view, host_fail, SMMC_HIP, host_timed_launch, host_outputs_to_host, ...), what
// those units lend each other, and the ONE statement of a wave-walk entry's run (host_wave_walk_run).  Not installed.
// smmc_internal.h holds what a kernel translation unit or a launch stub needs and is part of the kernels' source
// digest (tools/isa_loop_count.py); this header is not, so a host-only change here leaves profiles/pmc_traffic.json
// valid.
//
// Round 3 had three copies of these rules that had drifted apart: the group hard-coded the
// threshold and tested only a buffer's first byte for "already pinned", the drop-in treated SMMC_PIN_HOST=chunk
// as "whole".  The reference pins its result with cudaMallocHost (src/simulations.cu:591-592); here the
// caller owns the buffer, so it is page-locked in place (hipHostRegister) for the duration of a call.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <cstring>
#include <initializer_list>
#include <utility>

#include "smmc_internal.h"  // KernelArgs, CashflowArgs, PortfolioArgs, launch_finalize*

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
// How the depletion entries divide it.  One scenario: the final-value histogram in copy 0, the depletion counters
// from copy 1 on.  A sweep: [scenario][bucket] from 0, [scenario][period] from kSweepDepletedAt.
constexpr size_t kDepletedAt = SMMC_MAX_BINS;
static_assert(kDepletedAt + SMMC_MAX_CASHFLOW_PERIODS + 1 <= static_cast<size_t>(kHistSpread) * SMMC_MAX_BINS,
              "the engine's accumulator holds the histogram and the depletion counters");
// One scenario with checkpoints (smmc_portfolio_cashflow_checkpoints.cpp): a third region behind those two, the
// checkpoints' buckets [checkpoint][bucket].
constexpr size_t kCheckpointBucketsAt = kDepletedAt + SMMC_MAX_CASHFLOW_PERIODS + 1;
static_assert(SMMC_MAX_BINS <= kDepletedAt && kDepletedAt + SMMC_MAX_CASHFLOW_PERIODS + 1 <= kCheckpointBucketsAt &&
                  kCheckpointBucketsAt + SMMC_MAX_CHECKPOINT_BINS <= static_cast<size_t>(kHistSpread) * SMMC_MAX_BINS,
              "the engine's accumulator holds the final buckets, the depletion counters and the checkpoints' buckets side by side");
constexpr size_t kSweepDepletedAt = SMMC_MAX_SWEEP_COUNTERS;
static_assert(2u * SMMC_MAX_SWEEP_COUNTERS <= static_cast<size_t>(kHistSpread) * SMMC_MAX_BINS,
              "the engine's accumulator holds a sweep's buckets and depletion counters");

// ---- what smmc_capi.cpp shares with the library's other host translation units (smmc_cashflow.cpp, ...) -----
// Defined in smmc_capi.cpp, which owns struct smmc_engine; a unit that adds an entry point goes through these and
// keeps what it needs per engine in its own state (engine_ext), so that smmc_capi.cpp never calls into it.

// Makes `device` current for the scope and restores the caller's device after.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) ok = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

struct EngineView {  // what a launch needs to know of an engine
  int device;
  hipStream_t stream;
  uint32_t compute_units, max_grid;
  size_t max_lds;
  BlockPartial *d_partials;  // max_grid entries
  unsigned long long *clock_probe;  // KernelArgs::clock_probe of a launch now: null unless smmc_engine_timing is on
};
// One slot of state owned by another translation unit, keyed by `owner` (the address of an object of that unit):
// smmc_engine_destroy calls release(state) for every slot taken.
constexpr int kEngineExtSlots = 4;
struct EngineExt {
  const void *owner;  // null: free
  void *state;
  void (*release)(void *state);
};
int host_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));  // sets smmc_last_error()
// Returns SMMC_ERR_HIP with the call's text and place out of the enclosing function when a HIP call fails.
#define SMMC_HIP(call)                                                                                                   \
  do {                                                                                                                   \
    hipError_t err__ = (call);                                                                                           \
    if (err__ != hipSuccess)                                                                                             \
      return smmc::host_fail(SMMC_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
  } while (0)
// "<feature> counter stream v3 only": the refusal of SMMC_FLAG_STREAM_REF and SMMC_FLAG_STREAM_V2; `feature` ends in
// its verb ("cash flows support").
int host_require_v3(const smmc_sim *s, const char *feature);
// The grid of a wave-walk launch (wave_walk_group_paths): the chunks of group_paths, at most groups_per_cu workgroups
// per CU and at most grid_cap.  Refuses a request that would give a workgroup 2^32 paths or more (u32 counters).
int host_wave_walk_grid(const EngineView &v, uint64_t n_paths, uint32_t group_paths, uint32_t groups_per_cu, uint32_t grid_cap,
                        uint32_t *grid);
// The engine's timing pair around launch(ctx) -- begun before, closed on both paths; a failed launch is
// "<name> failed: <HIP's text>".  The template takes any callable returning hipError_t.
int host_timed_launch(smmc_engine *e, const char *name, hipError_t (*launch)(void *ctx), void *ctx);
template <typename F>
int host_timed_launch(smmc_engine *e, const char *name, F launch) {
  return host_timed_launch(e, name, [](void *f) { return (*static_cast<F *>(f))(); }, &launch);
}
// The _to_host form of an entry: one device allocation for all pieces (host == null: left out; the 8-byte aligned
// ones come first), run(dev, ctx) with the pieces' device pointers (null for one left out) enqueues on the engine
// stream; the stream is synchronised also after a failure (nothing of the call may outlive the buffer), the pieces
// are copied if all went well.  A HIP failure after a successful run is "<what>: <HIP's text>".  Device must be current.
struct HostPiece {
  void *host;
  size_t bytes;
};
constexpr int kMaxHostPieces = 12;  // the most any entry has: the twelve outputs of smmc_excursion_outputs
int host_outputs_to_host(smmc_engine *e, const char *what, const HostPiece *pieces, int n_pieces,
                         int (*run)(void *const *dev, void *ctx), void *ctx);
template <typename F>  // any callable int(void *const *dev), as host_timed_launch
int host_outputs_to_host(smmc_engine *e, const char *what, const HostPiece *pieces, int n_pieces, F run) {
  return host_outputs_to_host(e, what, pieces, n_pieces, [](void *const *dev, void *f) { return (*static_cast<F *>(f))(dev); }, &run);
}
int host_check_sim(const smmc_engine *e, const smmc_sim *s);
// What smmc_engine_simulate_checkpoints refuses about periods, n_checkpoints, the records pointer, the stream flags and
// n_checkpoints * n_bins, with its texts, for a checked sim; final_ptr (may be null): its 4-byte alignment.
int host_check_checkpoint_args(const smmc_sim *sim, const uint32_t *periods, uint32_t n_checkpoints, const void *final_ptr,
                               const void *records);
// bounds on a = 100 + r of one period; false if there are none (smmc_capi.cpp, divide_kind)
bool host_multiplier_bounds(const smmc_engine *e, const smmc_sim *s, double *lo_a, double *hi_a);
KernelArgs host_make_args(const smmc_engine *e, const smmc_sim *s);
EngineView engine_view(const smmc_engine *e);
// The slot of `owner`, claimed at the first ask; null when every slot belongs to somebody else.
EngineExt *engine_ext(smmc_engine *e, const void *owner);
// smmc_engine_divide_kind's rule with the window of SMMC_DIV_CHECKED (KernelArgs::chk_lo, chk_hi)
int host_divide_kind(const smmc_engine *e, const smmc_sim *s, bool allow_checked, float *chk_lo, float *chk_hi);
// the same rule for multipliers that lie in [lo_a, hi_a], lo_a > 0, whatever law they come from (smmc_regimes.cpp: the
// union of two regimes' bounds)
int host_divide_kind_of_bounds(const smmc_sim *s, double lo_a, double hi_a, bool allow_checked, float *chk_lo, float *chk_hi);
// smmc_engine_simulate_to_host's pipeline -- chunks, staging buffers, pinning, progress, merged record -- around
// another enqueue: `enqueue` is called with the device current, once per chunk, with that chunk's smmc_sim and
// device buffers (any may be null), and enqueues on the engine stream as smmc_engine_simulate does.
typedef int (*HostEnqueue)(smmc_engine *e, const smmc_sim *part, float *d_final, float *d_chunk_mean, float *d_chunk_var,
                           void *d_stats, const void *ctx);
int host_simulate_to_host(smmc_engine *e, const smmc_sim *sim, float *host_final, float *host_chunk_mean, float *host_chunk_var,
                          volatile int64_t *progress, smmc_stats *stats, uint64_t *hist, HostEnqueue enqueue, const void *ctx);

// ---- what smmc_portfolio.cpp and smmc_cashflow.cpp lend to smmc_portfolio_cashflow.cpp -----------------------------
// Each rule is stated once, in the unit that owns it; neither unit refers to the borrower.
// smmc_portfolio.cpp: every argument check of smmc_engine_simulate_portfolio on (e, sim, pf), the asset table included;
int portfolio_check(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf);
// bounds on asset k's multiplier a_k, false if there are none that keep it positive (the divide rule's);
bool portfolio_asset_bounds(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, uint32_t k, double *lo_a, double *hi_a);
// the KernelArgs and PortfolioArgs of a checked request (the asset table, the draw at scale 1, weights, s_k, L).
void portfolio_launch_args(const smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, KernelArgs *a, PortfolioArgs *p);
// smmc_cashflow.cpp: the checks of smmc_engine_simulate_cashflow on cf itself and on n_periods;
int cashflow_check_schedule(const smmc_sim *sim, const smmc_cashflow *cf);
inline bool cashflow_varying(const smmc_cashflow *cf) { return cf->amounts || cf->fractions; }  // per-period arrays
// the arrays of a varying schedule staged and their upload enqueued: c->schedule, c->stride.  Device must be current.
int cashflow_stage_schedule(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf, CashflowArgs *c);
// smmc_portfolio_cashflow.cpp, to smmc_portfolio_cashflow_regimes.cpp: smmc_engine_portfolio_cashflow_divide_kind's rule for
// multipliers a_k in [lo[k], hi_max], lo[k] > 0, k < pf->n_assets, whatever law they come from (there: the union of two
// regimes' bounds).  Every condition of the rule is monotone in lo[k] and in hi_max.
int portfolio_cashflow_divide_of_bounds(const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf, const double *lo, double hi_max);
// What smmc_engine_simulate_regimes refuses about the three probabilities, with its texts: stated here, inline, for
// smmc_portfolio_cashflow_regimes.cpp (tests/test_regimes_cpu.py lets no unit but smmc_regimes.cpp leave an undefined
// symbol of that word, so the borrower cannot call across units).
inline int markov_check_q16(const uint32_t (&leave_q16)[2], uint32_t start1_q16) {
  for (int r = 0; r < 2; ++r)
    if (leave_q16[r] > SMMC_REGIME_Q16_ONE)
      return host_fail(SMMC_ERR_INVALID, "leave_q16[%d] is %u: the probability leave_q16 / 65536 is at most 1", r, leave_q16[r]);
  if (start1_q16 > SMMC_REGIME_Q16_ONE)
    return host_fail(SMMC_ERR_INVALID, "start1_q16 is %u: the probability start1_q16 / 65536 is at most 1", start1_q16);
  return SMMC_OK;
}
// smmc_blocks.cpp, to smmc_portfolio_cashflow_blocks.cpp: what smmc_engine_simulate_blocks refuses about `blocks`, the mode
// and the stream of a checked sim, with its texts.
int blocks_check(const smmc_sim *sim, const smmc_blocks *b);
// smmc_stationary.cpp, to smmc_portfolio_cashflow_stationary.cpp: what smmc_engine_simulate_stationary refuses about `st`,
// the mode and the stream of a checked sim, with its texts.  Unlike blocks_check it is stated here, inline, and not
// defined in the lender: tests/test_stationary_cpu.py lets no unit but smmc_stationary.cpp leave an undefined symbol
// whose demangled text holds "stationary", and that text includes the parameter type `smmc_stationary const*`, so the
// borrower cannot call a function of this signature across units under any name.
inline int stationary_check(const smmc_sim *sim, const smmc_stationary *st) {
  if (!st) return host_fail(SMMC_ERR_INVALID, "the smmc_stationary argument is NULL");
  if (st->struct_size != sizeof(smmc_stationary))
    return host_fail(SMMC_ERR_INVALID, "smmc_stationary.struct_size is %u, this library expects %zu", st->struct_size, sizeof(smmc_stationary));
  if (sim->mode != SMMC_MODE_TABLE)
    return host_fail(SMMC_ERR_INVALID, "the stationary bootstrap resamples the returns table: mode must be SMMC_MODE_TABLE (got %d)", sim->mode);
  const int rc = host_require_v3(sim, "the stationary bootstrap supports");
  if (rc) return rc;
  if (st->renew_q16 > SMMC_RENEW_Q16_ONE)
    return host_fail(SMMC_ERR_INVALID, "renew_q16 is %u: the renewal probability renew_q16 / 65536 is at most 1", st->renew_q16);
  if (st->reserved[0] != 0 || st->reserved[1] != 0)
    return host_fail(SMMC_ERR_INVALID, "smmc_stationary.reserved is {%u, %u}, it must be 0", st->reserved[0], st->reserved[1]);
  return SMMC_OK;
}
// smmc_blocks.cpp, to smmc_stationary.cpp: its enqueue -- smmc_capi.cpp's enqueue_simulation around another path kernel:
// the kernel arguments of a checked sim, the grid, the LDS refusal, the accumulator lease, the divide, the timed launch
// and the fold -- with the kernel left to the caller.  Device must be current.  launch(a, div, grid, stream, ctx)
// enqueues the kernel and is reported under `name` when it fails; `lds` is what it asks of LDS for these outputs and
// `lds_holds` the words of the refusal ("<lds_holds> need N bytes of LDS, device allows M").  Nothing is launched and
// nothing refused for n_paths == 0.
struct PathLaunch {
  const char *name;
  hipError_t (*launch)(const KernelArgs &a, int div, uint32_t grid, hipStream_t stream, const void *ctx);
  const void *ctx;
  size_t lds;
  const char *lds_holds;
};
inline int host_check_lds(const EngineView &view, size_t lds, const char *lds_holds) {  // 2 KiB stay free for the runtime
  if (lds + 2048 > view.max_lds) return host_fail(SMMC_ERR_INVALID, "%s need %zu bytes of LDS, device allows %zu", lds_holds, lds, view.max_lds);
  return SMMC_OK;
}
int host_enqueue_paths(smmc_engine *e, const smmc_sim *s, const PathLaunch &w, float *d_final, float *d_chunk_mean, float *d_chunk_var,
                       void *d_stats);

// ---- what the entries of the feature units share: the checks of their outputs, the run, the _to_host form ----------
// An *_outputs structure of include/smmc.h that begins with struct_size and reserved; `type` is its name.
template <typename Out>
int host_check_outputs(const Out *out, const char *type) {
  if (!out) return host_fail(SMMC_ERR_INVALID, "the %s argument is NULL", type);
  if (out->struct_size != sizeof(Out))
    return host_fail(SMMC_ERR_INVALID, "%s.struct_size is %u, this library expects %zu", type, out->struct_size, sizeof(Out));
  if (out->reserved != 0) return host_fail(SMMC_ERR_INVALID, "%s.reserved is %u, it must be 0", type, out->reserved);
  return SMMC_OK;
}
// Is one of the pointers no multiple of `align` (4 or 8)?  The refusal's text stays the entry's own.
inline bool host_misaligned(std::initializer_list<const void *> ptrs, uintptr_t align) {
  uintptr_t bits = 0;
  for (const void *p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & (align - 1u)) != 0;
}
// The entries with loose output pointers (smmc_cashflow.cpp, smmc_sweep.cpp);
inline int cashflow_check_pointers(const void *fin, const void *paid, const void *ruin, const void *stats, const void *dep) {
  if (host_misaligned({fin, paid, ruin}, 4))
    return host_fail(SMMC_ERR_INVALID, "the final-value, paid and ruin-period pointers must be 4-byte aligned");
  if (host_misaligned({stats, dep}, 8))
    return host_fail(SMMC_ERR_INVALID, "the statistics and depletion-count pointers must be 8-byte aligned");
  return SMMC_OK;
}
// those with an outputs structure of a portfolio's depletion; `more`: one of the structure's further per-path pointers
// is misaligned, `words` then names them all.
template <typename Out>
int host_check_depletion_alignment(const Out *o, bool more = false,
                                   const char *words = "d_final, d_holdings, d_paid and d_ruin_period must be 4-byte aligned") {
  if (more || host_misaligned({o->d_final, o->d_holdings, o->d_paid, o->d_ruin_period}, 4)) return host_fail(SMMC_ERR_INVALID, "%s", words);
  if (host_misaligned({o->d_stats, o->d_depleted_at}, 8)) return host_fail(SMMC_ERR_INVALID, "d_stats and d_depleted_at must be 8-byte aligned");
  return SMMC_OK;
}

// The run of a wave-walk entry, stated ONCE (host_wave_walk_run).  The entry has made every check that needs no device
// and built its kernel arguments; it says what differs between entries:
struct WalkRecord {  // a statistics record of the launch; d_stats null: not asked for
  void *d_stats;                  // device: where the fold writes it
  uint32_t partials_at;           // its partials in the engine's partial array (EngineView::d_partials)
  size_t hist_at;                 // its bucket counts in the engine's accumulator
  BlockPartial **partials;        // the kernel arguments that get the two
  unsigned long long **d_hist;
};
struct WalkCounts {  // a count array of the launch (depletion, first passage); d_out null: not asked for
  uint64_t *d_out;                // device: where launch_finalize_depleted copies it
  size_t acc_at;                  // its counters in the engine's accumulator
  uint32_t n;
  unsigned long long **d_counts;  // the kernel argument that gets them
};
struct WalkRecordSet {  // n packed records that the launch leaves beside `records`, folded by a fold of their own (checkpoints);
  void *d_records;                // d_records null: none.  device: where that fold writes them
  uint32_t n;
  BlockPartial *partials_mem;     // their partials [record][workgroup], n x grid entries in an array of the ENTRY's own
  size_t hist_at;                 // their bucket counts [record][bucket] in the engine's accumulator
  BlockPartial **partials;        // the kernel arguments that get the two
  unsigned long long **d_hist;
};
struct WaveWalk {
  const char *name;  // of the launch, as host_timed_launch reports its failure
  uint32_t grid;     // workgroups; 0 (no paths): nothing is launched, the folds still write the empty outputs
  uint32_t n_bins;   // smmc_sim::n_bins of the request
  WalkRecord records[2];
  WalkCounts counts[3];  // the most any entry has: depletion, cuts and raises (smmc_guardrails.cpp)
  WalkRecordSet set = {};  // most entries leave none
};
// How a record is folded: one record (launch_finalize), or the packed records of n scenarios whose partials and
// buckets lie [scenario][...] from the record's offsets (launch_finalize_sweep).  A type each, so that a unit refers to
// the launch symbol of its own fold only.
struct FoldRecord {
  hipError_t operator()(const BlockPartial *partials, uint32_t grid, void *d_stats, uint32_t n_bins, unsigned long long *hist,
                        hipStream_t stream) const {
    return launch_finalize(partials, grid, static_cast<smmc_stats *>(d_stats), n_bins, stream, hist, n_bins ? 1u : 0u);
  }
};
struct FoldScenarios {
  uint32_t n;
  hipError_t operator()(const BlockPartial *partials, uint32_t grid, void *d_stats, uint32_t n_bins, unsigned long long *hist,
                        hipStream_t stream) const {
    return launch_finalize_sweep(partials, grid, n, d_stats, n_bins, hist, stream);
  }
};
// How WaveWalk::set is folded: not at all (an entry without one), or as checkpoints (launch_finalize_checkpoints).
struct NoRecordSet {
  hipError_t operator()(const WalkRecordSet &, uint32_t, uint32_t, unsigned long long *, hipStream_t) const { return hipSuccess; }
};
struct FoldCheckpointSet {
  hipError_t operator()(const WalkRecordSet &s, uint32_t grid, uint32_t n_bins, unsigned long long *hist, hipStream_t stream) const {
    return launch_finalize_checkpoints(s.partials_mem, grid, s.n, s.d_records, n_bins, hist, stream);
  }
};
struct NoPrepare {
  int operator()() const { return SMMC_OK; }
};
// The protocol: the engine's device current; prepare() (what an entry enqueues before its kernel: a staged schedule); the
// lease on the accumulator if a histogram or a count array will be counted -- zero now, and zero again after the folds;
// the kernel arguments wired; launch(stream) unless the grid is empty; the records folded, then the count arrays; and
// only with all folds in the queue the lease's mark comes off.  Any error return in between leaves the accumulator dirty.
template <typename Fold, typename Launch, typename Prepare = NoPrepare, typename FoldSet = NoRecordSet>
int host_wave_walk_run(smmc_engine *e, const WaveWalk &w, Fold fold, Launch launch, Prepare prepare = Prepare(), FoldSet fold_set = FoldSet()) {
  const EngineView view = engine_view(e);
  DeviceGuard guard(view.device);
  if (!guard.ok) return host_fail(SMMC_ERR_HIP, "hipSetDevice(%d) failed", view.device);
  int rc = prepare();
  if (rc) return rc;
  bool counted = w.set.d_records && w.n_bins;
  for (const WalkRecord &r : w.records) counted = counted || (r.d_stats && w.n_bins);
  for (const WalkCounts &c : w.counts) counted = counted || c.d_out;
  ZeroLease lease;
  if (counted) {
    rc = engine_acc_lease(e, &lease);
    if (rc) return rc;
  }
  unsigned long long *const acc = lease.acc();
  for (const WalkRecord &r : w.records)
    if (r.d_stats) {
      *r.partials = view.d_partials + r.partials_at;
      *r.d_hist = w.n_bins ? acc + r.hist_at : nullptr;
    }
  for (const WalkCounts &c : w.counts)
    if (c.d_out) *c.d_counts = acc + c.acc_at;
  if (w.set.d_records) {
    *w.set.partials = w.set.partials_mem;
    *w.set.d_hist = w.n_bins ? acc + w.set.hist_at : nullptr;
  }
  if (w.grid) {
    rc = host_timed_launch(e, w.name, [&] { return launch(view.stream); });
    if (rc) return rc;
  }
  for (const WalkRecord &r : w.records)
    if (r.d_stats)
      SMMC_HIP(fold(view.d_partials + r.partials_at, w.grid, r.d_stats, w.n_bins, w.n_bins ? acc + r.hist_at : nullptr, view.stream));
  if (w.set.d_records) SMMC_HIP(fold_set(w.set, w.grid, w.n_bins, w.n_bins ? acc + w.set.hist_at : nullptr, view.stream));
  for (const WalkCounts &c : w.counts)
    if (c.d_out) SMMC_HIP(launch_finalize_depleted(acc + c.acc_at, c.n, reinterpret_cast<unsigned long long *>(c.d_out), view.stream));
  lease.finalize_queued();
  return SMMC_OK;
}

// host_outputs_to_host for an entry that takes an *_outputs structure: `fields` lists its pointer members (offsetof) with
// the bytes behind each, the 8-byte aligned ones first; run(d) gets a copy of `out` with the device pointers in them.
struct OutputField {
  size_t offset, bytes;
};
template <typename Out, int N, typename F>
int host_outputs_struct_to_host(smmc_engine *e, const char *what, const Out &out, const OutputField (&fields)[N], F run) {
  static_assert(N <= kMaxHostPieces, "more pieces than host_outputs_to_host takes");
  HostPiece pieces[N];
  for (int i = 0; i < N; ++i) {
    std::memcpy(&pieces[i].host, reinterpret_cast<const char *>(&out) + fields[i].offset, sizeof(void *));
    pieces[i].bytes = fields[i].bytes;
  }
  return host_outputs_to_host(e, what, pieces, N, [&](void *const *dev) {
    Out d = out;
    for (int i = 0; i < N; ++i) std::memcpy(reinterpret_cast<char *>(&d) + fields[i].offset, &dev[i], sizeof(void *));
    return run(&d);
  });
}

}  // namespace smmc
