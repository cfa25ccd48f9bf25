/*
 * smmc.h -- C ABI of the MI355X Monte-Carlo returns engine (libsmmc_hip.so).
 *
 * This is the drop-in boundary for ONE path of matthijsvk/stock_market_monte_carlo:
 * the Monte-Carlo returns engine of src/simulations.cpp / src/simulations.cu.
 * Plain pointers and sizes only; no C++ or torch types.  Each entry point names
 * the reference interface it stands in for (paths relative to the reference
 * tree).  The C++ header include/stock_market_monte_carlo/simulations.h re-exports
 * the reference's own free-function signatures on top of these.
 *
 * Threading: an engine is bound to one device and one stream and is not
 * re-entrant; use one engine per host thread (engines are cheap).  Different
 * engines may be used concurrently.  No call exits the process: every failure
 * is a negative return code plus smmc_last_error() (thread-local text).
 *
 * Random stream ("counter stream v3"; round 1's stream v2 stays selectable
 * with SMMC_FLAG_STREAM_V2): Philox4x32-10, key =
 * the 64-bit seed, counter = (block of periods, global path id, mode).  A path's value
 * depends only on (seed, global path id, parameters), never on the launch
 * geometry, the shard it falls in or the number of GPUs.
 */
#ifndef SMMC_H
#define SMMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMMC_ABI_VERSION 4

/* return codes */
#define SMMC_OK 0
#define SMMC_ERR_INVALID (-1)   /* bad argument */
#define SMMC_ERR_HIP (-2)       /* a HIP runtime call failed */
#define SMMC_ERR_NO_DEVICE (-3) /* no usable gfx950 device */
#define SMMC_ERR_NOMEM (-4)

/* how a period's return is drawn */
#define SMMC_MODE_TABLE 0    /* i.i.d. with replacement from the returns table   */
#define SMMC_MODE_GAUSSIAN 1 /* N(gauss_mean, gauss_std), Box-Muller             */

/* smmc_sim.flags */
#define SMMC_FLAG_EXACT_DIV 1u /* force the IEEE divide kernel variant */
#define SMMC_FLAG_STREAM_V2 2u /* counter stream v2 (round 1's) instead of v3: its counter layout (both modes) and its Gaussian draw */
/* The reference CPU engine's OWN stream (src/simulations.cpp:240-252), table mode only: path id draws from
 * std::mt19937 seeded with (uint32_t)(seed + id) -- the reference seeds each path from a fresh
 * std::random_device and has no seed argument -- through libstdc++'s uniform_int_distribution<int>
 * (Lemire's map with rejection), then update_fund.  With the seeds the reference's generators got, the
 * final values (and, with the keepdata entries, the trajectories: mc_simulations_keepdata draws the same
 * way, src/simulations.cpp:175-186) are the reference's, bit for bit.  Statistics and chunk outputs are
 * formed from the final values by a second pass.  About 3x the arithmetic of the default stream at 360
 * periods and 4x at 1000 (the generator's 624 words of state per path are regenerated from seed chains, never
 * stored, for paths of up to 1816 periods; longer paths keep them in device memory). */
#define SMMC_FLAG_STREAM_REF 4u
#define SMMC_FLAG_QUIET 8u /* no SMMC_VERBOSE phase lines for this request (the drop-in's warm-up run) */
/* smmc_engine_simulate_to_host: leave host_final as it is -- no page-locking for the call whatever SMMC_PIN_HOST
 * says (the caller has pinned it, or has tried and failed: smmc_group_simulate registers the whole result once
 * for all its devices and passes this to every shard, so that neighbouring shards never register the page
 * their boundary falls in twice). */
#define SMMC_FLAG_HOST_NOPIN 16u

/* paths per chunk of the per-chunk mean/variance outputs: the reference's
 * THREADS_PER_BLOCK (src/simulations.cu:17), one (mean, variance) pair per block
 * in mc_simulations_gpu_kernel_reduceBlock (src/simulations.cu:240-246). */
#define SMMC_CHUNK 256

/* largest returns table an engine accepts (it is staged whole in LDS) */
#define SMMC_MAX_TABLE 16384
/* largest histogram */
#define SMMC_MAX_BINS 4096

typedef struct smmc_engine smmc_engine;

/* One simulation request: n_paths independent paths with global ids
 * first_path .. first_path + n_paths - 1, n_periods compounding steps each.
 * Mirrors the argument lists of mc_simulations (src/simulations.cpp:204-209) and
 * mc_simulations_gpu (src/simulations.cu:661-667) plus what the reference leaves
 * implicit (seed, draw mode) or computes on the host afterwards (statistics:
 * examples/benchmark_mc_gpu.cpp:7-41). */
typedef struct smmc_sim {
  uint32_t struct_size;   /* = sizeof(smmc_sim) */
  int32_t mode;           /* SMMC_MODE_*                                        */
  uint64_t seed;          /* Philox key                                         */
  uint64_t first_path;    /* global id of the first path (sharding offset)      */
  uint64_t n_paths;       /* max_n_simulations                                  */
  uint32_t n_periods;     /* n_periods                                          */
  float initial_capital;  /* initial_capital                                    */
  float gauss_mean;       /* percent per period (examples/monte_carlo_simulated.cpp:11) */
  float gauss_std;        /* percent per period (examples/monte_carlo_simulated.cpp:12) */
  uint32_t n_bins;        /* histogram buckets, 0 = none, <= SMMC_MAX_BINS      */
  float hist_lo, hist_hi; /* bucket range [lo, hi)                              */
  float below_threshold;  /* count of final values < this                       */
  uint32_t flags;         /* SMMC_FLAG_*                                        */
} smmc_sim;

/* Packed statistics record as the device writes it: this header followed by
 * n_bins uint64 bucket counts.  smmc_stats_bytes(n_bins) is its size.  All
 * integer fields are exact; sum/sumsq are double-precision sums of the float
 * final values in a fixed (launch-geometry dependent) order. */
typedef struct smmc_stats {
  uint64_t count;     /* paths simulated                                       */
  uint64_t below;     /* final value < below_threshold (benchmark_mc_gpu.cpp:30-41) */
  uint64_t underflow; /* final value < hist_lo                                 */
  uint64_t overflow;  /* final value >= hist_hi, or NaN                        */
  double sum;         /* sum of final values (benchmark_mc_gpu.cpp:13-17)      */
  double sumsq;       /* sum of squares                                        */
  float min, max;     /* +inf / -inf when count == 0                           */
  uint32_t n_bins;
  uint32_t reserved;
} smmc_stats;

/* ---- host scalar functions ------------------------------------------------ */

/* update_fund, src/simulations.cpp:14-16: fund * (100.0f + r) / 100 in binary32. */
float smmc_update_fund(float fund_value, float period_return);

/* __many_updates, src/simulations.cpp:18-22: totals[0] is read, totals[1..n] written. */
void smmc_many_updates(const float *returns, float *totals, uint32_t n_periods);

/* ---- library / device ------------------------------------------------------ */

int smmc_abi_version(void);
const char *smmc_last_error(void);
/* 64 hex digits: sha256 over the compiler flags and every source and header this library was built from
 * (stock_market_monte_carlo_amd/build.py: source_digest()).  The Python loader refuses a library whose digest
 * differs from the sources beside it; bench.py prints it; the reference has no counterpart (its build is
 * CMake's, CMakeLists.txt:99-103). */
const char *smmc_build_digest(void);

/* Number of visible HIP devices (0 and SMMC_OK when there is none). */
int smmc_device_count(int *count);

/* ---- engine ---------------------------------------------------------------- */

/* Pass as `stream` to make the engine create (and own) a non-blocking stream. */
#define SMMC_STREAM_NEW ((void *)(intptr_t)-1)

/* Binds an engine to `device`.  `stream` is the hipStream_t to launch on (e.g. the
 * caller's current torch stream); NULL is the device's default stream, as in every
 * HIP call; SMMC_STREAM_NEW asks for an engine-owned non-blocking stream.
 * Replaces the per-call cudaSetDevice/cudaMalloc/cudaFree plan of
 * create_plan_v2 (src/simulations.cu:568-574, 599-607, 632-637). */
int smmc_engine_create(int device, void *stream, smmc_engine **out);
void smmc_engine_destroy(smmc_engine *e);

/* Re-binds the engine to another stream of its device (e.g. the caller's CURRENT torch stream,
 * passed before every call).  Work already enqueued stays ordered before anything enqueued
 * afterwards.  An engine-owned stream is drained and destroyed.  A caller's stream must outlive the
 * work the engine enqueued on it; if it was destroyed after that work finished, the next set_stream
 * still succeeds (the event record on the dead handle fails, the engine lets the device drain and
 * adopts the new stream) -- every other call uses the stream bound last, so re-bind first.  smmc_engine_get_stream returns the
 * handle launches go to (so a caller can order its own streams against an engine-owned one). */
int smmc_engine_set_stream(smmc_engine *e, void *stream);
int smmc_engine_get_stream(smmc_engine *e, void **stream);
/* Ordering against another stream of the same device, for engines that keep their own stream:
 * wait_stream -- what the engine enqueues from now on runs after everything enqueued on `stream`
 * so far (call it before launching into buffers that were allocated or written on `stream`);
 * release_to_stream -- what is enqueued on `stream` from now on runs after everything the engine has
 * enqueued so far (call it before `stream` reads, frees or reuses the outputs).  Event-based, no
 * host synchronisation. */
int smmc_engine_wait_stream(smmc_engine *e, void *stream);
int smmc_engine_release_to_stream(smmc_engine *e, void *stream);

/* Uploads the historical-returns table (percent units, host memory).  Replaces
 * the H2D table copies at src/simulations.cu:382,451,525,617.  Waits for work already
 * enqueued on the engine stream; the host array may be reused on return. */
int smmc_engine_set_table(smmc_engine *e, const float *returns_percent, uint32_t n);

/* Enqueues one simulation on the engine stream and returns without waiting.
 * All output pointers are DEVICE pointers on the engine's device; any may be NULL:
 *   d_final       n_paths floats, final value of each path, coalesced
 *                 (totals of mc_simulations_gpu_kernel, src/simulations.cu:151)
 *   d_chunk_mean  ceil(n_paths / SMMC_CHUNK) floats, mean of each 256-path chunk
 *   d_chunk_var   same length, population variance of each chunk
 *                 (means/variances of the reduceBlock kernel, src/simulations.cu:240-246)
 *   d_stats       smmc_stats_bytes(sim->n_bins) bytes, packed statistics record, 8-byte aligned
 * Replaces mc_simulations_gpu_launcher / _reduceBlock_launcher
 * (src/simulations.cu:345-473). */
int smmc_engine_simulate(smmc_engine *e, const smmc_sim *sim, float *d_final, float *d_chunk_mean,
                         float *d_chunk_var, void *d_stats);

/* Same, but keeps every trajectory: d_traj is n_paths x (n_periods + 1) floats,
 * path-major (row i = the `values` vector of path i, values[0] = initial capital)
 * -- mc_data of mc_simulations_keepdata (src/simulations.cpp:139-186).  d_final
 * may be NULL.  Any 4-byte aligned d_traj; n_periods < 2^24 (SMMC_ERR_INVALID
 * otherwise). */
int smmc_engine_simulate_keepdata(smmc_engine *e, const smmc_sim *sim, float *d_traj, float *d_final);

/* ---- checkpoint statistics: the value distribution at chosen periods ------------------------ */

#define SMMC_MAX_CHECKPOINTS 64
/* largest n_checkpoints * n_bins of one call: the kernel keeps that many 32-bit bucket counters in LDS beside
 * the draw tables (32 KiB: 64 checkpoints x 128 buckets, or 31 x 256, or 2 x 4096) */
#define SMMC_MAX_CHECKPOINT_BINS 8192

/* Enqueues one simulation that also reduces the paths' values at n_checkpoints chosen periods.
 * periods[0 .. n_checkpoints): HOST array, strictly increasing, 1 <= periods[k] <= sim->n_periods; the value
 * of a path "at period p" is its value after p compounding steps = column p of its keepdata row.
 * d_records: DEVICE, n_checkpoints packed records back to back, smmc_stats_bytes(sim->n_bins) bytes each,
 * 8-byte aligned; record k is the record smmc_engine_values_stats would write for column periods[k] of the
 * trajectories smmc_engine_simulate_keepdata writes for the same sim (below_threshold, n_bins, hist_lo,
 * hist_hi of sim apply to every checkpoint): integer fields, min, max and bucket counts exactly, sum and sumsq
 * as double sums in a fixed order (two identical calls give the same bytes; no floating-point atomics).
 * d_final (may be NULL): as in smmc_engine_simulate, and bit-identical to it.
 * The values are in a register at every period; reducing them there costs K small records instead of the
 * 4 (n_periods + 1) bytes per path of keepdata.  Replaces the per-frame host passes over mc_data that put the
 * MINIMUM / TARGET levels next to the plotted lines (examples/visualize_returns_cpu_v2.cpp:397-411) and
 * update_count_below_min (:125-138) evaluated for an earlier period than the last.
 * Divide: a checkpoint value has to be right when it is taken, so the end-of-path rerun of SMMC_DIV_CHECKED
 * does not apply; the launch follows the keepdata rule, smmc_engine_divide_kind(e, sim, 1): the fast form when
 * the host proves the window, the IEEE divide otherwise or with SMMC_FLAG_EXACT_DIV.
 * SMMC_ERR_INVALID: n_checkpoints == 0 or > SMMC_MAX_CHECKPOINTS; a period that is 0, above n_periods or not
 * above the one before it; NULL periods or d_records; SMMC_FLAG_STREAM_REF or SMMC_FLAG_STREAM_V2 (counter
 * stream v3 only); n_checkpoints * n_bins > SMMC_MAX_CHECKPOINT_BINS; more than 2^32 paths per workgroup
 * (n_paths beyond some 10^13: shard the request, the records merge with smmc_stats_merge).
 * Asynchronous on the engine stream; periods[] may be reused on return. */
int smmc_engine_simulate_checkpoints(smmc_engine *e, const smmc_sim *sim, const uint32_t *periods,
                                     uint32_t n_checkpoints, float *d_final, void *d_records);
/* Synchronous convenience: the same into HOST memory (records: n_checkpoints * smmc_stats_bytes(n_bins) bytes). */
int smmc_engine_simulate_checkpoints_to_host(smmc_engine *e, const smmc_sim *sim, const uint32_t *periods,
                                             uint32_t n_checkpoints, float *host_final, void *host_records);

/* ---- cash flows: withdrawal and contribution schedules with depletion statistics ------------- */

#define SMMC_MAX_CASHFLOW_PERIODS 4096 /* depletion counters live in LDS: 16 KiB of u32 */

/* What is taken out of (or, negative, paid into) every path after each period's return.  For period t = 1 ..
 * n_periods, a_t = 100 + r_t as in smmc_engine_simulate, every operation binary32 and rounded on its own:
 *   g  = (v * a_t) / 100                       update_fund, src/simulations.cpp:14-16
 *   w  = amount[t-1] + g * fraction[t-1]       the product is rounded, then the sum
 *   v' = g - w
 *   live path, v' > floor:     v = v', paid += w
 *   live path, !(v' > floor):  depleted at t: v = 0, paid += max(g, 0), ruin_period = t (NaN counts as depleted;
 *                              max is fmaxf: a NaN g pays 0)
 *   depleted path:             v stays 0, paid and ruin_period stay; its draws are still consumed
 * amount is in money units, fraction a plain fraction of the value after the period's return (0.004 = 0.4 %).
 * The reference README's open "withdrawal strategies": a fixed amount every period (amount, fraction 0), some
 * percentage every period (fraction, amount 0), a varying percentage every period (the arrays; also how a caller
 * indexes amounts to inflation).  With amount = fraction = 0 and floor = 0 the final values are those of
 * smmc_engine_simulate, bit for bit, while no multiplier is <= 0. */
typedef struct smmc_cashflow {
  uint32_t struct_size;   /* = sizeof(smmc_cashflow) */
  float amount, fraction; /* used for every period when the array below is NULL */
  const float *amounts;   /* HOST, n_periods floats, or NULL */
  const float *fractions; /* HOST, n_periods floats, or NULL */
  float floor;            /* depleted when !(value > floor); >= 0 */
} smmc_cashflow;

/* Enqueues one simulation with the cash flow cf on the engine stream and returns without waiting; the host arrays
 * of cf may be reused on return (the engine stages them).  All outputs are DEVICE pointers, any may be NULL; they
 * are written, not accumulated into:
 *   d_final        n_paths final values, 0 for a depleted path
 *   d_paid         n_paths totals paid out (binary32 running sums in period order, from 0)
 *   d_ruin_period  n_paths periods of depletion, 0 = never depleted
 *   d_stats        packed record of the final values, smmc_stats_bytes(sim->n_bins) bytes, 8-byte aligned, with
 *                  the field rules of smmc_engine_simulate
 *   d_depleted_at  n_periods + 1 counts: [0] paths never depleted, [t] paths depleted at period t; their sum is
 *                  n_paths.  8-byte aligned.
 * A path's outputs depend only on (seed, global path id, parameters, schedule), never on first_path, the shard or
 * the launch geometry; shards of one request merge by smmc_stats_merge and by adding d_depleted_at.  Integer
 * fields, min, max, bucket counts and d_depleted_at are exact; sum and sumsq are double sums in a fixed order
 * (no floating-point atomics): two identical calls give the same bytes.
 * Divide: the result never depends on the variant.  The proof behind smmc_engine_divide_kind does not carry over
 * (a live value can come close to 0), so the reciprocal-multiply form is used only when BOTH hold, the IEEE
 * divide otherwise or with SMMC_FLAG_EXACT_DIV (smmc_engine_cashflow_divide_kind says which):
 *   below  every live value is above L = the larger of floor and, when every amount is <= 0 and every fraction
 *          is in [0, 1), capital * min(1, lo (1 - max fraction))^n_periods (lo, hi: the smallest and largest
 *          multiplier / 100); capital itself is the first live value; min(capital, L) times the smallest
 *          multiplier stays above 2^-88.  A depleted path's product 0 * a is exact in both forms.
 *   above  every fraction is in [0, 1], and (capital + the sum of the contributions, the amounts < 0)
 *          * max(1, hi)^n_periods times the largest multiplier stays below 2^126.
 * SMMC_ERR_INVALID with a text: NULL cf or a wrong struct_size; n_periods == 0 or > SMMC_MAX_CASHFLOW_PERIODS;
 * floor negative or not finite; a non-finite amount, fraction or schedule entry; SMMC_FLAG_STREAM_REF or
 * SMMC_FLAG_STREAM_V2 (counter stream v3 only); the table-mode and bin-count errors of smmc_engine_simulate;
 * 2^32 paths or more per workgroup (shard the request). */
int smmc_engine_simulate_cashflow(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf, float *d_final,
                                  float *d_paid, uint32_t *d_ruin_period, void *d_stats, uint64_t *d_depleted_at);
/* Synchronous convenience: the same into HOST memory. */
int smmc_engine_simulate_cashflow_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf,
                                          float *host_final, float *host_paid, uint32_t *host_ruin_period,
                                          void *host_stats, uint64_t *host_depleted_at);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT: the divide a smmc_engine_simulate_cashflow of (sim, cf) uses, by the rule above
 * (never SMMC_DIV_CHECKED), or an error of that call's argument checks. */
int smmc_engine_cashflow_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *cf);

/* ---- cash-flow sweeps: up to eight constant schedules on the same paths, one launch ---------- */

#define SMMC_MAX_SWEEP 8
#define SMMC_MAX_SWEEP_COUNTERS 8192 /* n_scenarios * (n_periods + 1 + n_bins) u32 counters in LDS: 32 KiB */

/* "Which withdrawal still survives?" is a curve over schedules.  One launch draws every period's return once and
 * steps n_scenarios (1 .. SMMC_MAX_SWEEP) schedules on it: the scenarios share their paths (common random
 * numbers), and the draw -- more than half of a single call's work -- is made once.
 * scenarios: a HOST array of n_scenarios smmc_cashflow, each a CONSTANT schedule: amount, fraction and floor are
 * used, amounts and fractions must be NULL.  It may be reused on return.
 * Outputs: DEVICE pointers, scenario-major, any may be NULL, written, not accumulated into; alignment as
 * smmc_engine_simulate_cashflow:
 *   d_final, d_paid, d_ruin_period   [n_scenarios][n_paths]
 *   d_stats                          n_scenarios packed records, smmc_stats_bytes(sim->n_bins) bytes each
 *   d_depleted_at                    [n_scenarios][n_periods + 1]
 * Arithmetic: scenario s is smmc_engine_simulate_cashflow(sim, &scenarios[s]).  final, paid, ruin_period,
 * depleted_at, the record's integer fields, min, max and bucket counts are those of that call, bit for bit; sum and
 * sumsq are double sums in a fixed order of the sweep's own (no floating-point atomics: two identical sweeps give
 * the same bytes) and agree with the single call's to 1e-12 relative.  A path depends on (seed, global path id,
 * parameters, its scenario) only: not on the other scenarios, n_scenarios, first_path or the launch geometry.
 * Shards merge by smmc_stats_merge and by adding d_depleted_at, scenario by scenario.
 * Divide: SMMC_DIV_FAST if and only if smmc_engine_cashflow_divide_kind says FAST for every scenario; otherwise,
 * or with SMMC_FLAG_EXACT_DIV, the IEEE divide for all of them (smmc_engine_cashflow_sweep_divide_kind says
 * which).  Results never depend on the variant.
 * Monotone in the amount: take two scenarios with equal floor, fraction = 0 and amounts a <= b.  On every path the
 * value under b is <= the value under a after every period, and the period of depletion under b is not later than
 * under a ("never depleted" counting as latest).  Every binary32 operation of the contract is monotone: for a
 * multiplier > 0, v -> (v * a_t) / 100 is non-decreasing, g - amount is non-decreasing in g and non-increasing
 * in the amount, and a depleted path holds 0, which no live path (> floor >= 0) is below.
 * SMMC_ERR_INVALID with a text: everything smmc_engine_simulate_cashflow refuses, for any scenario; NULL
 * scenarios; n_scenarios 0 or above SMMC_MAX_SWEEP; a scenario with amounts or fractions; n_scenarios *
 * (n_periods + 1 + n_bins) above SMMC_MAX_SWEEP_COUNTERS, n_bins counting as 0 when d_stats is NULL; 2^32 paths or
 * more per workgroup (shard the request); tables and counters beyond the device's LDS. */
int smmc_engine_simulate_cashflow_sweep(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *scenarios,
                                        uint32_t n_scenarios, float *d_final, float *d_paid,
                                        uint32_t *d_ruin_period, void *d_stats, uint64_t *d_depleted_at);
/* Synchronous convenience: the same into HOST memory. */
int smmc_engine_simulate_cashflow_sweep_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *scenarios,
                                                uint32_t n_scenarios, float *host_final, float *host_paid,
                                                uint32_t *host_ruin_period, void *host_stats,
                                                uint64_t *host_depleted_at);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT: the divide a sweep of (sim, scenarios) uses, or an error of that call's checks
 * of sim and of the scenarios (the counter cap depends on the outputs and is the simulating calls' alone). */
int smmc_engine_cashflow_sweep_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_cashflow *scenarios,
                                           uint32_t n_scenarios);

/* ---- excursions: drawdown, running extremes, first passage of levels -------------------------- */

#define SMMC_MAX_EXCURSION_PERIODS 4096 /* two arrays of n_periods + 1 u32 first-passage counters live in LDS */

/* What happened ALONG a path, reduced while its value is in a register.  For a path with values v_0 =
 * initial_capital and v_t, t = 1 .. n_periods -- bit for bit the row of smmc_engine_simulate_keepdata for the same
 * smmc_sim -- every operation binary32 and rounded on its own (nothing fuses), every comparison false for NaN:
 *   at t = 0: peak = low = dd_peak = dd_low = v_0; dd_period = run = longest = first_below = first_reach = 0
 *   for t = 1 .. n_periods, v = v_t:
 *     if (v > peak) peak = v
 *     if (v < low)  low  = v
 *     if (fl(v * dd_peak) < fl(dd_low * peak))    a deeper relative drawdown than the deepest so far (strict); uses
 *         dd_peak = peak, dd_low = v, dd_period = t      the peak already updated above
 *     run = (v < peak) ? run + 1 : 0;  longest = max(longest, run)
 *     if (first_below == 0 && v <  lower)  first_below = t     the reference's `val < min_final_amount`
 *     if (first_reach == 0 && v >= target) first_reach = t
 *   at the end: drawdown = fl(fl(dd_peak - dd_low) / dd_peak)  one IEEE divide per path
 * v / peak > dd_low / dd_peak is decided by cross-multiplication, which keeps the divide out of the period loop and
 * is part of the contract: the two products round, and overflow to inf, as binary32 products do.  For values that
 * stay finite and positive, drawdown is max over t of 1 - v_t / (running maximum) to a few binary32 roundings. */
typedef struct smmc_excursions {
  uint32_t struct_size;     /* = sizeof(smmc_excursions) */
  float lower;              /* MINIMUM level: first_below = first t with v_t <  lower  */
  float target;             /* TARGET level:  first_reach = first t with v_t >= target */
  float drawdown_threshold; /* `below` of the drawdown record counts paths with drawdown < this */
} smmc_excursions;

/* All pointers DEVICE (HOST in the _to_host form), any may be NULL; written, not accumulated into.  The per-path
 * arrays are 4-byte aligned, the records and the count arrays 8-byte aligned. */
typedef struct smmc_excursion_outputs {
  uint32_t struct_size; /* = sizeof(smmc_excursion_outputs) */
  float *final, *peak, *low, *drawdown;                               /* n_paths each */
  uint32_t *drawdown_period, *underwater, *first_below, *first_reach; /* n_paths each; underwater = `longest` */
  void *stats;          /* record of the final values: exactly smmc_engine_simulate's d_stats */
  void *drawdown_stats; /* record of `drawdown`: n_bins buckets over [0, 1), below = drawdown < drawdown_threshold,
                           underflow < 0, overflow >= 1 or NaN; smmc_stats_bytes(sim->n_bins) bytes */
  uint64_t *first_below_at, *first_reach_at; /* n_periods + 1 counts each: [0] never, [t] first at period t; the
                                                sum of each is n_paths */
} smmc_excursion_outputs;

/* Enqueues one simulation on the engine stream and returns without waiting.  A path's outputs depend only on
 * (seed, global path id, parameters), never on first_path, the shard or the launch geometry.  Integer fields, min,
 * max, bucket counts and the two count arrays are exact; sum and sumsq are double sums in a fixed order (no
 * floating-point atomics): two identical calls give the same bytes.  Shards of one request merge by
 * smmc_stats_merge and by adding the count arrays.
 * Divide by 100: a value has to be right when it is looked at, so the launch follows the keepdata rule,
 * smmc_engine_divide_kind(e, sim, 1): the fast form when proven, the IEEE divide otherwise or with
 * SMMC_FLAG_EXACT_DIV; never SMMC_DIV_CHECKED.  The result does not depend on it.
 * SMMC_ERR_INVALID with a text: NULL x or out, or a wrong struct_size; n_periods == 0 or >
 * SMMC_MAX_EXCURSION_PERIODS; a NaN lower, target or drawdown_threshold (+-inf is allowed: "never" / "always");
 * SMMC_FLAG_STREAM_REF or SMMC_FLAG_STREAM_V2 (counter stream v3 only); the table-mode and bin-count errors of
 * smmc_engine_simulate; table, counters and histograms beyond the device's LDS; 2^32 paths or more per workgroup
 * (shard the request). */
int smmc_engine_simulate_excursions(smmc_engine *e, const smmc_sim *sim, const smmc_excursions *x,
                                    const smmc_excursion_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_excursions_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_excursions *x,
                                            const smmc_excursion_outputs *out);

/* ---- block bootstrap: table paths drawn in runs of consecutive months --------------------------- */

/* SMMC_MODE_TABLE draws every period on its own, which keeps nothing of what lies between neighbouring months of
 * the table (volatility clustering, momentum, the shape of a crash and its recovery).  The circular block bootstrap
 * builds a path from runs of L = block_len consecutive table entries.  Counter stream v3, table mode only; with the
 * table a[i] = 100.0f + r[i] (one binary32 addition at smmc_engine_set_table) of T entries:
 *   block b = 0, 1, ... of path id starts at table index s_b, which is EXACTLY the index the SMMC_MODE_TABLE stream
 *     draws for that path at period b: Philox4x32-10 block b / D with the key (seed lo, seed hi) and the counter
 *     (b / D, id lo, id hi, 0) of table mode, digit b % D; D = 8 for T <= 2048 -- the four base-T digits of the
 *     64-bit fraction (out[0] : out[1]), then the four of (out[2] : out[3]) -- and D = 4 above, digit j =
 *     floor(out[j] * T / 2^32).  No new random-number construction: the starts of a path over P periods are the
 *     table-mode indices of the same path over ceil(P / L) periods.
 *   period t = 0 .. n_periods - 1 uses entry (s_{t div L} + t mod L) mod T: a block that runs past the end of the
 *     table continues at its beginning.  L may exceed T or n_periods.
 *   the step is smmc_update_fund's: total = fl(fl(total * a) / 100.0f), two binary32 roundings after the one in a.
 * A path depends only on (seed, global path id, table, L); the launch shape and the sharding are invisible, and the
 * value after p periods does not depend on n_periods (a run with n_periods = p yields column p of a longer run).
 * With block_len = 1 every output is bit-identical to smmc_engine_simulate's in table mode. */
#define SMMC_BLOCKS_CIRCULAR 0 /* the only kind; anything else is SMMC_ERR_INVALID (runs of random length have entries of
                                  their own: smmc_engine_simulate_stationary) */
typedef struct smmc_blocks {
  uint32_t struct_size; /* = sizeof(smmc_blocks) */
  uint32_t block_len;   /* L >= 1 */
  uint32_t kind;        /* SMMC_BLOCKS_CIRCULAR */
  uint32_t reserved;    /* 0 */
} smmc_blocks;

/* smmc_engine_simulate with block draws: the same outputs with the same meaning (DEVICE pointers, any may be NULL),
 * enqueued on the engine stream; n_periods == 0 and n_paths == 0 behave as there.
 * SMMC_ERR_INVALID with a text: mode != SMMC_MODE_TABLE; no table set; SMMC_FLAG_STREAM_V2 or SMMC_FLAG_STREAM_REF;
 * NULL blocks, a wrong struct_size, block_len == 0, kind != SMMC_BLOCKS_CIRCULAR, reserved != 0; table, its circular
 * extension and the histogram beyond the device's LDS; the other argument errors of smmc_engine_simulate.
 * Divide by 100: smmc_engine_blocks_divide_kind; the result does not depend on it. */
int smmc_engine_simulate_blocks(smmc_engine *e, const smmc_sim *sim, const smmc_blocks *blocks, float *d_final,
                                float *d_chunk_mean, float *d_chunk_var, void *d_stats);
/* smmc_engine_simulate_to_host with block draws: HOST pointers, the same chunked pipeline, pinning rules
 * (SMMC_PIN_HOST, SMMC_FLAG_HOST_NOPIN), progress reports and merged record. */
int smmc_engine_simulate_blocks_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_blocks *blocks, float *host_final,
                                        float *host_chunk_mean, float *host_chunk_var, volatile int64_t *progress,
                                        smmc_stats *stats, uint64_t *hist);
/* SMMC_DIV_FAST, SMMC_DIV_CHECKED or SMMC_DIV_EXACT: the divide a smmc_engine_simulate_blocks of (sim, blocks) uses,
 * or an error of that call's argument checks.  The bounds on a product come from the table's smallest and largest
 * entry, the capital and n_periods, never from the order of the draws, so the rule is smmc_engine_divide_kind(e, sim,
 * 0)'s: the kernel tests the checked window at least once every 8 periods and redoes a path that ever leaves it with
 * the IEEE divide. */
int smmc_engine_blocks_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_blocks *blocks);

/* ---- stationary bootstrap: table paths in runs of geometric length ------------------------------- */

/* The block bootstrap cuts every path at the same periods 0, L, 2L, ...: a statistic at period t then depends on
 * t mod L, the series is not stationary.  The stationary bootstrap (Politis and Romano, 1994) starts a new run at every
 * period with probability p and otherwise continues with the next month of the table: run lengths are geometric with
 * mean 1 / p and the series is stationary.  Counter stream v3, table mode only; the table a[i] = 100.0f + r[i] of T
 * entries, P = n_periods, and ONE parameter q = renew_q16 in [0, 65536]: p = q / 65536.
 *   candidate start c_t of period t = 0 .. P - 1 is EXACTLY the index the SMMC_MODE_TABLE stream draws for that path at
 *     period t: Philox4x32-10 block t / D with the key (seed lo, seed hi) and the counter (t / D, id lo, id hi, 0), digit
 *     t % D, D and the digits as the block bootstrap states them above.  No new index construction.
 *   renewal field f_t is a 16-bit field of a SECOND Philox4x32-10 block with the same key and the counter
 *     (t / 8, id lo, id hi, 2): word (t % 8) / 2 of its output, the low half for an even t % 8, the high half for an odd
 *     one.  The block index is t / 8 whatever D is.  Fourth counter word 2 belongs to these fields alone: 0 is the
 *     table's, the odd values 1, 3, ... are the Gaussian series' (portfolios below), no other stream uses an even one.
 *   index: i_0 = c_0; for t >= 1, i_t = c_t if f_t < q, else i_t = i_{t-1} + 1, wrapped to 0 at T (circular, as the block
 *     bootstrap).  The field of period 0 is not used.
 *   the step is smmc_update_fund's: total = fl(fl(total * a[i_t]) / 100.0f).
 * A path depends only on (seed, global path id, table, q); the launch shape and the sharding are invisible, and the value
 * after p periods does not depend on n_periods.  Two identities, bit for bit in every output:
 *   q = 65536 is smmc_engine_simulate in table mode;
 *   q = 0 is smmc_engine_simulate_blocks with any block_len >= n_periods.
 * The resolution of p is 2^-16. */
#define SMMC_RENEW_Q16_ONE 65536u /* renew_q16 of p = 1; the largest value accepted */
typedef struct smmc_stationary {
  uint32_t struct_size; /* = sizeof(smmc_stationary) */
  uint32_t renew_q16;   /* q: 0 .. SMMC_RENEW_Q16_ONE */
  uint32_t reserved[2]; /* 0 */
} smmc_stationary;

/* smmc_engine_simulate_blocks with these draws: the same outputs with the same meaning (DEVICE pointers, any may be
 * NULL; d_final, d_chunk_mean, d_chunk_var 4-byte and d_stats 8-byte aligned), enqueued on the engine stream;
 * n_periods == 0 and n_paths == 0 behave as there.
 * SMMC_ERR_INVALID with a text: NULL st, a wrong struct_size, renew_q16 > 65536, a reserved word != 0; mode !=
 * SMMC_MODE_TABLE; SMMC_FLAG_STREAM_V2 or SMMC_FLAG_STREAM_REF; no table set; table and histogram beyond the device's
 * LDS; the other argument errors of smmc_engine_simulate.
 * Divide by 100: smmc_engine_stationary_divide_kind; the result does not depend on it. */
int smmc_engine_simulate_stationary(smmc_engine *e, const smmc_sim *sim, const smmc_stationary *st, float *d_final,
                                    float *d_chunk_mean, float *d_chunk_var, void *d_stats);
/* smmc_engine_simulate_to_host with these draws: HOST pointers, the same chunked pipeline, pinning rules, progress
 * reports and merged record. */
int smmc_engine_simulate_stationary_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_stationary *st, float *host_final,
                                            float *host_chunk_mean, float *host_chunk_var, volatile int64_t *progress,
                                            smmc_stats *stats, uint64_t *hist);
/* SMMC_DIV_FAST, SMMC_DIV_CHECKED or SMMC_DIV_EXACT: the divide a smmc_engine_simulate_stationary of (sim, st) uses, or
 * an error of that call's argument checks.  The rule of smmc_engine_divide_kind(e, sim, 0): its bounds come from the
 * table's extremes, the capital and n_periods, never from the order of the draws; the kernel tests the checked window
 * once every 8 periods and redoes a path that ever leaves it with the IEEE divide. */
int smmc_engine_stationary_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_stationary *st);

/* ---- regime-switching Gaussian paths: a two-state Markov law for returns ------------------------- */

/* SMMC_MODE_GAUSSIAN draws every period from one normal law.  Here a path carries a hidden state s_t in {0, 1} (Hamilton's
 * two regimes: bull and bear) that persists from period to period, each regime with a mean and a deviation of its own:
 * the Gaussian counterpart of what runs of consecutive months do for the table.  SMMC_MODE_GAUSSIAN, counter stream v3
 * only.  sim->gauss_mean and sim->gauss_std are NOT read: the two regimes' numbers stand in `rg`.  For a path with its
 * 64-bit global id and the 0-based period t:
 *   z_t is EXACTLY the standard normal that smmc_engine_simulate_portfolio (below) draws in Gaussian mode for asset 0 at
 *     period t: Philox4x32-10 block (t / 4, id lo, id hi, 1) under the key (seed lo, seed hi), draw t % 4, the v3 tables
 *     at scale 1 and shift 0.  No new normal construction.
 *   f_t is a 16-bit field of a SECOND Philox4x32-10 block with the same key and the counter (t / 8, id lo, id hi, 4): word
 *     (t % 8) / 2 of its output, the low half for an even t % 8, the high half for an odd one -- the stationary bootstrap's
 *     field with fourth counter word 4 in place of 2.  Even fourth words are field streams: 0 is the table's, 2 the
 *     renewal's, 4 belongs to these fields alone.
 *   state: s_0 = 1 if f_0 < start1_q16, else 0; for t >= 1, s_t = s_{t-1} ^ (f_t < leave_q16[s_{t-1}] ? 1 : 0).
 *   multiplier: a_t = fmaf(std[s_t], z_t, fl(100.0f + mean[s_t])), ONE fused operation: the portfolio's own form for one
 *     asset.
 *   the step is smmc_update_fund's: total = fl(fl(total * a_t) / 100.0f).
 * A path depends only on (seed, global path id, rg); the launch shape and the sharding are invisible.  Identities, bit for
 * bit on the final values, the chunk means and variances and the statistics record:
 *   1. mean[0] == mean[1] and std[0] == std[1], with any probabilities, is smmc_engine_simulate_portfolio in Gaussian mode
 *      with n_assets = 1, weight 1, means = {mean[0]}, factor = {std[0]}, rebalance_every = 0;
 *   2. start1_q16 = 0 and leave_q16[0] = 0 is that call with regime 0's numbers whatever regime 1 holds; start1_q16 =
 *      65536 and leave_q16[1] = 0 is that call with regime 1's numbers;
 *   3. the first P' periods of a P-period request are the P'-period request.
 * The resolution of every probability is 2^-16; the mean sojourn in regime r is 65536 / leave_q16[r] periods and the
 * chain's stationary share of regime 1 is leave_q16[0] / (leave_q16[0] + leave_q16[1]). */
#define SMMC_REGIME_Q16_ONE 65536u /* a q16 of probability 1; the largest value accepted */
typedef struct smmc_regimes {
  uint32_t struct_size;  /* = sizeof(smmc_regimes) */
  float mean[2];         /* percent per period, regime 0 and 1 */
  float std[2];          /* percent per period, >= 0 */
  uint32_t leave_q16[2]; /* probability of leaving regime r at a period, in units of 2^-16: 0 .. 65536 */
  uint32_t start1_q16;   /* probability that period 0 is in regime 1: 0 .. 65536 */
  uint32_t reserved[2];  /* 0 */
} smmc_regimes;

/* smmc_engine_simulate with these draws: the same outputs with the same meaning (DEVICE pointers, any may be NULL;
 * d_final, d_chunk_mean, d_chunk_var 4-byte and d_stats 8-byte aligned), enqueued on the engine stream; n_periods == 0
 * and n_paths == 0 behave as there.
 * SMMC_ERR_INVALID with a text, before any device work: NULL rg, a wrong struct_size, a mode other than
 * SMMC_MODE_GAUSSIAN, SMMC_FLAG_STREAM_V2 or SMMC_FLAG_STREAM_REF, a q16 above 65536, a mean or deviation that is not
 * finite, a negative deviation, a reserved word != 0; draw tables and histogram beyond the device's LDS; the other
 * argument errors of smmc_engine_simulate.
 * Divide by 100: smmc_engine_regimes_divide_kind; the result does not depend on it. */
int smmc_engine_simulate_regimes(smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg, float *d_final,
                                 float *d_chunk_mean, float *d_chunk_var, void *d_stats);
/* smmc_engine_simulate_to_host with these draws: HOST pointers, the same chunked pipeline, pinning rules, progress
 * reports and merged record. */
int smmc_engine_simulate_regimes_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg, float *host_final,
                                         float *host_chunk_mean, float *host_chunk_var, volatile int64_t *progress,
                                         smmc_stats *stats, uint64_t *hist);
/* SMMC_DIV_FAST, SMMC_DIV_CHECKED or SMMC_DIV_EXACT: the divide a smmc_engine_simulate_regimes of (sim, rg) uses, or an
 * error of that call's argument checks.  The rule of smmc_engine_divide_kind(e, sim, 0) on the UNION of the two regimes'
 * multiplier bounds, each regime's as one Gaussian asset's (mean[r], std[r] rounded up): a path's multipliers are, period
 * by period, one regime's or the other's.  No bounds for either regime is SMMC_DIV_EXACT.  The kernel tests the checked
 * window once every 8 periods and redoes a path that ever leaves it with the IEEE divide. */
int smmc_engine_regimes_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_regimes *rg);

/* ---- portfolios: jointly drawn assets, weights, periodic rebalancing ---------------------------- */

/* K = n_assets return series per path, drawn JOINTLY, held with weights w_k and rebalanced to them every R =
 * rebalance_every periods (R = 0: never, buy and hold).  Counter stream v3 only.  Two independent runs cannot be
 * combined into this: table mode needs the same historical month for every asset, Gaussian mode a given correlation,
 * and with rebalancing the value of a path is no function of the assets' separate products.
 *
 * Holdings, every operation one binary32 rounding:
 *   at the start       h_k = fl(initial_capital * w_k)
 *   period t = 1 .. P  h_k = fl(fl(h_k * a_k(t)) / 100.0f) for every asset: smmc_update_fund from its second rounding on
 *   the value          V_t = ((h_0 + h_1) + h_2) + h_3, binary32 additions left to right over the K assets (K = 1:
 *                      V_t = h_0); V_0 is the same sum of the initial holdings
 *   rebalance          if R > 0 and t mod R == 0, the holdings of the following periods are h_k = fl(V_t * w_k)
 *   the final value    V_P, formed BEFORE any rebalance at P; so are the final holdings
 * V_p does not depend on n_periods.  With K = 1 and w_0 = 1 every R gives the plain path.
 *
 * Table mode: joint rows.  smmc_engine_set_asset_table gives the engine a table of n_rows x n_assets returns in percent,
 * row-major, stored as a = 100.0f + r (as smmc_engine_set_table stores its table; the two tables are independent and
 * a portfolio does not need the single-series one).  Period t of a path uses row i_t for EVERY asset, and i_t is
 * exactly the index SMMC_MODE_TABLE draws for that path at period t - 1 (0-based) with T = n_rows: the same key, the
 * same counter (t' / D, id lo, id hi, 0), the same digits; D = 8 for n_rows <= 2048, else 4.  With K = 1 and w_0 = 1
 * the final values are bit-identical to smmc_engine_simulate's on the same column.
 *
 * Gaussian mode: correlated normals.  Asset j's STANDARD normals z_j for the periods 4b .. 4b + 3 are counter stream
 * v3's Box-Muller draws of the Philox block (b, id lo, id hi, 1 + 2 j) with the launch's key, taken with scale 1.0f and
 * shift 0.0f: asset 0 reads the very words of the plain Gaussian stream; odd fourth words belong to Gaussian assets,
 * even ones belong to the table side (0: its indices, 2: the stationary bootstrap's renewal fields).  With s_k = fl(100.0f + means[k]) and the lower-triangular factor L (percent),
 *   a_k = fma(L[k][k], z_k, fma(L[k][k-1], z_{k-1}, ... fma(L[k][0], z_0, s_k))),
 * the terms taken from j = 0 upwards, each step ONE fused multiply-add.  sim->gauss_mean and sim->gauss_std are not
 * read.  K = 1 gives the LAW of the plain Gaussian mode with gauss_std = L[0][0] but not its bits: the plain mode
 * folds the standard deviation into the coefficients of the radius cubic, here it multiplies the finished normal.
 *
 * A path depends only on (seed, global path id, table or means and L, weights, R); the launch shape and the sharding
 * are invisible. */
#define SMMC_MAX_ASSETS 4
typedef struct smmc_portfolio {
  uint32_t struct_size;     /* = sizeof(smmc_portfolio) */
  uint32_t n_assets;        /* K, 1 .. SMMC_MAX_ASSETS */
  uint32_t rebalance_every; /* R; 0 = never (buy and hold) */
  uint32_t reserved;        /* 0 */
  float weights[SMMC_MAX_ASSETS];                  /* w_k >= 0, summing to 1 within 1e-6; entries k >= K must be 0 */
  float means[SMMC_MAX_ASSETS];                    /* Gaussian mode: percent per period; else 0 */
  float factor[SMMC_MAX_ASSETS * SMMC_MAX_ASSETS]; /* Gaussian mode: lower-triangular L, percent, L[k][j] at
                                                      [k * SMMC_MAX_ASSETS + j], diagonal >= 0; everything else 0 */
} smmc_portfolio;

typedef struct smmc_portfolio_outputs {
  uint32_t struct_size, reserved; /* = sizeof(smmc_portfolio_outputs), 0 */
  float *d_final;    /* n_paths, nullable */
  float *d_holdings; /* asset-major K x n_paths final holdings (before any rebalance at P), nullable */
  void *d_stats;     /* packed record of the final values, smmc_stats_bytes(n_bins), nullable */
} smmc_portfolio_outputs;

/* The joint table of table-mode portfolios: n_rows x n_assets returns in percent, row-major; n_assets in 1 ..
 * SMMC_MAX_ASSETS, n_rows * n_assets <= SMMC_MAX_TABLE.  Copied before the call returns; replaces an earlier one. */
int smmc_engine_set_asset_table(smmc_engine *e, const float *returns_percent, uint32_t n_rows, uint32_t n_assets);
/* One portfolio simulation, enqueued on the engine stream; out holds DEVICE pointers (4-byte aligned, d_stats 8-byte),
 * any may be NULL.  n_periods == 0 yields V_0; n_paths == 0 launches nothing and yields the empty record.
 * SMMC_ERR_INVALID with a text: NULL or wrongly sized structures; SMMC_FLAG_STREAM_V2 or SMMC_FLAG_STREAM_REF;
 * n_assets == 0 or > SMMC_MAX_ASSETS; reserved != 0; a weight that is negative, NaN or infinite, or non-zero at
 * k >= n_assets; |sum of the weights (in double) - 1| > 1e-6; table mode without an asset table or with one of another
 * column count, or with a non-zero entry in means or factor; Gaussian mode with a non-finite mean or factor entry, a
 * non-zero entry above the diagonal or beyond K, or a negative diagonal; asset table, histogram and partials beyond the
 * device's LDS; 2^32 or more paths per workgroup (shard the request); the other argument errors of
 * smmc_engine_simulate.  Divide by 100: smmc_engine_portfolio_divide_kind; the result does not depend on it. */
int smmc_engine_simulate_portfolio(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                   const smmc_portfolio_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_portfolio_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                           const smmc_portfolio_outputs *out);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT (never SMMC_DIV_CHECKED: the holdings are summed at every rebalance, so a value must
 * be right whenever it is looked at -- keepdata's rule), or an error of the call's argument checks.  FAST when every
 * product h_k * a_k provably stays inside [2^-89, 2^127) or is exactly 0: per asset a_k lies between its column's
 * extremes (table mode) or inside s_k -+ Zmax * sum_j |L[k][j]| (Gaussian mode, the draw bound of
 * smmc_engine_divide_kind); a value lies between V_0 times the worst and the best asset's multiplier / 100 to the
 * power t; a positive holding is at least the smallest positive initial holding, or the smallest positive weight times
 * the lowest possible value, shrunk by the worst multiplier since ("Portfolios").  A holding of exactly 0
 * stays 0 in both forms.  SMMC_FLAG_EXACT_DIV forces the IEEE divide. */
int smmc_engine_portfolio_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf);

/* ---- portfolio cash flows: a schedule on a rebalanced portfolio, with depletion statistics ------ */

/* "60/40, rebalanced yearly, 4 % out every year, contributions before that": the portfolio of smmc_portfolio (meaning,
 * checks and draws exactly as in smmc_engine_simulate_portfolio, the asset table of smmc_engine_set_asset_table
 * included) with the cash flow of smmc_cashflow (meaning and checks exactly as in smmc_engine_simulate_cashflow; amounts
 * and fractions may be arrays; 1 <= n_periods <= SMMC_MAX_CASHFLOW_PERIODS) taken out of its value after every period's
 * return.  Counter stream v3 only.  The two parent calls cannot be combined into this from outside: with a cash flow
 * and a rebalance a path's value is no function of two separate runs.
 *
 * Per path, every operation ONE binary32 rounding, nothing fused, every comparison false for NaN; a_k(t) are the
 * portfolio contract's multipliers, R = rebalance_every, P = n_periods:
 *   start            h_k = fl(capital * w_k);  paid = 0;  ruin = 0;  alive
 *   t = 1 .. P       h_k = fl(fl(h_k * a_k(t)) / 100.0f)            every asset, as the portfolio step
 *                    g   = ((h_0 + h_1) + h_2) + h_3                left to right over K
 *                    w   = fl(amount[t-1] + fl(g * fraction[t-1]))
 *                    vn  = fl(g - w)
 *     live, vn > floor:     paid = fl(paid + w);  v = vn
 *                           if R > 0 and t mod R == 0 and t != P:   h_k = fl(vn * w_k)          rebalance what is left
 *                           else:                                   h_k = fl(h_k - fl(w * w_k)) the flow settles at the
 *                                                                                               target weights
 *     live, !(vn > floor):  depleted at t: every h_k = 0, v = 0, paid = fl(paid + fmaxf(g, 0)), ruin = t
 *     depleted:             nothing changes (a lane mask keeps it so, not the arithmetic); its draws are still consumed
 *   final value = v after period P;  final holdings = h_k after period P (no rebalance at P)
 * What follows from it:
 *   - The final value is vn.  The sum of the final holdings may differ from it in the last bits.
 *   - A flow settles at the target weights: contributions buy the target mix, withdrawals sell it.  A holding whose
 *     share of a withdrawal exceeds it turns NEGATIVE and compounds as such until the next rebalance; the contract does
 *     not clamp it, and the value alone decides depletion.  Buy and hold with long withdrawals gets there.
 *   - Zero flows (amount = fraction = 0, floor = 0, no arrays) give smmc_engine_simulate_portfolio's final values and
 *     holdings bit for bit, while every value stays finite and above 0.
 *   - Table mode with K = 1, w_0 = 1 and any R gives smmc_engine_simulate_cashflow's final, paid, ruin_period and
 *     depleted_at bit for bit on that column.
 *   - A path depends only on (seed, global path id, table or means and factor, weights, R, schedule, floor), never on
 *     first_path, the shard or the launch geometry. */
typedef struct smmc_portfolio_cashflow_outputs {
  uint32_t struct_size, reserved; /* = sizeof(smmc_portfolio_cashflow_outputs), 0 */
  float *d_final;          /* n_paths final values, 0 for a depleted path */
  float *d_holdings;       /* final holdings, asset-major K x n_paths */
  float *d_paid;           /* n_paths totals paid out */
  uint32_t *d_ruin_period; /* n_paths periods of depletion, 0 = never */
  void *d_stats;           /* packed record of the final values, smmc_stats_bytes(n_bins), with the field rules of
                              smmc_engine_simulate */
  uint64_t *d_depleted_at; /* n_periods + 1 counts: [0] never depleted, [t] depleted at period t; their sum is n_paths */
} smmc_portfolio_cashflow_outputs;

/* Enqueues one such simulation on the engine stream and returns without waiting; the host arrays of cf may be reused on
 * return.  out holds DEVICE pointers (4-byte aligned, d_stats and d_depleted_at 8-byte), any may be NULL; they are
 * written, not accumulated into.  Integer fields, min, max, bucket counts and the depletion counts are exact; sum and
 * sumsq are double sums in a fixed order with no floating-point atomics, so two identical calls give the same bytes.
 * Shards merge by smmc_stats_merge and by adding d_depleted_at.  n_paths == 0 launches nothing and yields the empty
 * record and zero counts.
 * SMMC_ERR_INVALID with a text: everything smmc_engine_simulate_portfolio refuses for sim and pf, everything
 * smmc_engine_simulate_cashflow refuses for cf and n_periods; a NULL or wrongly sized out, or reserved != 0; asset
 * table, depletion counters and histogram beyond the device's LDS; 2^32 or more paths per workgroup (shard the
 * request). */
int smmc_engine_simulate_portfolio_cashflow(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                            const smmc_cashflow *cf, const smmc_portfolio_cashflow_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_portfolio_cashflow_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                    const smmc_cashflow *cf, const smmc_portfolio_cashflow_outputs *out);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT (never SMMC_DIV_CHECKED), or an error of the call's argument checks.  Results never
 * depend on the form.  The reciprocal-multiply form is used only where the host proves that every product h_k * a_k is
 * exactly 0 or has a magnitude inside [2^-89, 2^127) (the device self-test of the form covers both signs); otherwise,
 * or with SMMC_FLAG_EXACT_DIV, the IEEE divide.  With the per-asset multiplier bounds of
 * smmc_engine_portfolio_divide_kind, a positive capital, every positively weighted asset starting above 0, every
 * fraction 0 and (capital + the sum of |amount|) grown by the best asset in every period below 2^126, FAST holds for
 *   contributions only   every amount <= 0: holdings only gain, and the portfolio rule's lower bound stands;
 *   one constant amount  not 0, no arrays, and floor > 0 if a rebalance happens (0 < R < P): a holding that enters a
 *                        product is the initial one, at least floor * w_k after a rebalance, or a binary32 difference
 *                        with the share fl(amount * w_k), which is 0 or at least 2^-25 of that share; each of these
 *                        times the asset's smallest multiplier stays above 2^-88.
 * Anything else -- a fraction, varying withdrawals -- is EXACT ("Portfolio cash flows", has the proof). */
int smmc_engine_portfolio_cashflow_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                               const smmc_cashflow *cf);

/* ---- block-bootstrap plans: portfolio cash flows on runs of consecutive months ------------------- */

/* smmc_engine_simulate_portfolio_cashflow on paths built as smmc_engine_simulate_blocks builds them: independent rows keep
 * the correlation between assets and destroy what lies between neighbouring months -- volatility clusters, the shape of a
 * crash and of its recovery, runs of bad years --, which is what sequence-of-returns risk and the depletion statistics are
 * made of.  A path is a sequence of runs of L = blocks->block_len consecutive rows of the asset table.
 * Scope: SMMC_MODE_TABLE and counter stream v3 only; the table is the one given by smmc_engine_set_asset_table, T = n_rows.
 * Block starts: block b = 0, 1, ... of a path starts at row s_b, exactly the row smmc_engine_simulate_portfolio's table
 *     stream draws for that path at 0-based period b: the same key, counter (b / D, id lo, id hi, 0) and digits, D = 8
 *     for n_rows <= 2048 and 4 above.
 * Row of a period: period t = 1 .. P uses row (s_{(t-1) div L} + (t-1) mod L) mod n_rows, for every asset.  L may exceed
 *     n_rows or P.
 * No new random numbers: the starts of a path over P periods are the parent's rows over ceil(P / L) periods.
 * Recurrence: everything after the row is smmc_engine_simulate_portfolio_cashflow's, word for word -- the holdings, the
 *     left-to-right value, the flow, settling at the target weights, the rebalance at t mod R == 0 && t != P, depletion,
 *     the lane mask of a depleted path (whose draws are still consumed), the outputs, the exactness of the record and the
 *     counts, byte-identical repeat calls, shards merged by smmc_stats_merge and by adding d_depleted_at, n_paths == 0.
 * A path depends only on (seed, global path id, table, weights, R, schedule, floor, L).
 * Identities:
 *   1. block_len == 1 is smmc_engine_simulate_portfolio_cashflow bit for bit: final, holdings, paid, ruin_period,
 *      depleted_at, the record's integer fields, min, max and bucket counts; sum and sumsq within relative 1e-12 (another
 *      summation order is allowed).
 *   2. K = 1, w_0 = 1, zero flows and floor 0 give smmc_engine_simulate_blocks' final values bit for bit for the same
 *      column (also given to smmc_engine_set_table) and the same L, while every value stays finite and above 0, whatever
 *      divide either call takes.
 *   3. Zero flows with any K are the block bootstrap of smmc_engine_simulate_portfolio.
 *   4. block_len >= n_periods: every path is ONE run of consecutive rows from s_0, the parent's first row.
 * SMMC_ERR_INVALID with a text, before any device work: everything smmc_engine_simulate_portfolio_cashflow refuses;
 * mode != SMMC_MODE_TABLE; everything smmc_engine_simulate_blocks refuses for blocks (NULL, a wrong struct_size, block_len
 * == 0, kind != SMMC_BLOCKS_CIRCULAR, reserved != 0); the asset table with its circular extension of 7 rows, the n_periods
 * + 1 depletion counters, the n_bins buckets and the waves' partials beyond the device's LDS less 2048 bytes (the text
 * names both numbers).  out holds DEVICE pointers as in the parent.  Asynchronous on the engine stream. */
int smmc_engine_simulate_portfolio_cashflow_blocks(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                   const smmc_cashflow *cf, const smmc_blocks *blocks,
                                                   const smmc_portfolio_cashflow_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_portfolio_cashflow_blocks_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                           const smmc_cashflow *cf, const smmc_blocks *blocks,
                                                           const smmc_portfolio_cashflow_outputs *out);
/* After the call's argument checks, blocks included: what smmc_engine_portfolio_cashflow_divide_kind(e, sim, pf, cf)
 * returns.  That rule's bounds come from the columns' extremes, the capital, P, the weights and the schedule, never from
 * the order of the rows, and a block path is the parent's recurrence on another order of the same rows (DESIGN.md,
 * "Block-bootstrap plans").  Results never depend on the form. */
int smmc_engine_portfolio_cashflow_blocks_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                      const smmc_cashflow *cf, const smmc_blocks *blocks);

/* ---- stationary-bootstrap plans: portfolio cash flows on runs of geometric length ---------------- */

/* smmc_engine_simulate_portfolio_cashflow on rows chosen as smmc_engine_simulate_stationary chooses its entries: the block
 * plan above cuts every path at the same periods, so a survival probability or a depletion count at period t depends on
 * t mod L; here a path starts a new run at every period with probability p = st->renew_q16 / 65536 and the series of rows
 * is stationary.  Scope: SMMC_MODE_TABLE and counter stream v3 only; the table is the one given by
 * smmc_engine_set_asset_table, T = n_rows; K = 1 .. 4 assets, P = n_periods, q = renew_q16 in [0, 65536].
 * Row rule: period t = 0 .. P - 1 (0-based) of a path reads row i_t of the asset table, for every asset.  i_0 = c_0; for
 *     t > 0, i_t = c_t if f_t < q, else i_{t-1} + 1, wrapped to 0 at n_rows.
 *   c_t is EXACTLY the row smmc_engine_simulate_portfolio's table stream draws for that path at 0-based period t: the same
 *     key, counter (t / D, id lo, id hi, 0) and digits over n_rows, D = 8 for n_rows <= 2048 and 4 above.
 *   f_t is the renewal field of the stationary bootstrap above, unchanged: the Philox4x32-10 block with the launch's key
 *     and the counter (t / 8, id lo, id hi, 2), word (t % 8) / 2 of its output, the low half for an even t % 8, the high
 *     half for an odd one.  The field of period 0 is not used.
 * No other random numbers are drawn.
 * Recurrence: everything after the row is smmc_engine_simulate_portfolio_cashflow's, word for word (0-based period t is
 *     that call's period t + 1) -- the holdings, the left-to-right value, the flow, settling at the target weights, the
 *     rebalance, the floor, depletion, the six outputs, the exactness of the record and the counts, byte-identical repeat
 *     calls, shards merged by smmc_stats_merge and by adding d_depleted_at, n_paths == 0.
 * Depleted paths: a depleted path keeps drawing its candidates and fields and walking its index; nothing of a path depends
 *     on another path's state.  A path depends only on (seed, global path id, table, weights, R, schedule, floor, q).
 * Identities, bit for bit on every output (sum and sumsq of the record follow the launch shape, which is the same):
 *   1. q = 65536 is smmc_engine_simulate_portfolio_cashflow in table mode.
 *   2. q = 0 is smmc_engine_simulate_portfolio_cashflow_blocks with any block_len >= n_periods: one run from c_0.
 *   3. K = 1, w_0 = 1, zero amount and fraction, floor 0: d_final equals the final values of
 *      smmc_engine_simulate_stationary for the same column (also given to smmc_engine_set_table), seed, ids and q, for
 *      every path that never depletes, whatever divide either call takes.
 * SMMC_ERR_INVALID with a text, before any device work, in this order: everything smmc_engine_simulate_portfolio refuses
 * of (sim, pf); everything smmc_engine_simulate_cashflow refuses of the schedule; everything
 * smmc_engine_simulate_stationary refuses of st (NULL, a wrong struct_size, mode != SMMC_MODE_TABLE, a stream flag,
 * renew_q16 > 65536, a reserved word != 0); the outputs structure; the asset table, the n_periods + 1 depletion counters,
 * the n_bins buckets and the waves' partials beyond the device's LDS less 2048 bytes (the text names both numbers).  out
 * holds DEVICE pointers as in the parent.  Asynchronous on the engine stream. */
int smmc_engine_simulate_portfolio_cashflow_stationary(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                       const smmc_cashflow *cf, const smmc_stationary *st,
                                                       const smmc_portfolio_cashflow_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_portfolio_cashflow_stationary_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                               const smmc_cashflow *cf, const smmc_stationary *st,
                                                               const smmc_portfolio_cashflow_outputs *out);
/* After the call's argument checks, st included: what smmc_engine_portfolio_cashflow_divide_kind(e, sim, pf, cf) returns,
 * SMMC_DIV_FAST or SMMC_DIV_EXACT (this family has no checked form).  That rule's bounds never depend on the order of the
 * rows ("Block-bootstrap plans"), and a stationary path is the parent's recurrence on another order of the same
 * rows.  Results never depend on the form. */
int smmc_engine_portfolio_cashflow_stationary_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                          const smmc_cashflow *cf, const smmc_stationary *st);

/* ---- regime-switching plans: portfolio cash flows under a two-state law ---------------------------- */

/* smmc_engine_simulate_portfolio_cashflow in Gaussian mode with the hidden state of smmc_engine_simulate_regimes: every
 * regime has a joint law of its own for the K assets (bear markets persist, and correlations rise in them), and a month's
 * multipliers are those of the regime the path is in.  The composition of those two contracts; neither is restated here.
 * Scope: SMMC_MODE_GAUSSIAN and counter stream v3 only; sim->gauss_mean and sim->gauss_std are NOT read.  pf gives
 * n_assets, weights and rebalance_every; pf->means and pf->factor must be all zero, the laws stand in `rg`.  For a path
 * with its 64-bit global id and the 0-based period t:
 *   normals: z_k(t) are EXACTLY the standard normals smmc_engine_simulate_portfolio draws in Gaussian mode: Philox block
 *     (t / 4, id lo, id hi, 1 + 2 k), draw t % 4, the v3 tables at scale 1 and shift 0.  No new normal construction.
 *   state: s_t is EXACTLY the state of smmc_engine_simulate_regimes for the same (leave_q16, start1_q16): field f_t of the
 *     block (t / 8, id lo, id hi, 4), s_0 = f_0 < start1_q16, s_t = s_{t-1} ^ (f_t < leave_q16[s_{t-1}]).  No new random
 *     numbers: a plan and a one-asset regime run with the same seed and ids see the same bull and bear months.
 *   multiplier: a_k(t) is smmc_portfolio's chain of fused multiply-adds over row k of L_{s_t} = factor[s_t], from j = 0
 *     upwards, starting at fl(100.0f + means[s_t][k]).
 *   step: everything after the multipliers is smmc_engine_simulate_portfolio_cashflow's, word for word (0-based period t
 *     is that call's period t + 1) -- the holdings, the left-to-right value, the flow settling at the target weights, the
 *     rebalance at t mod R == 0 && t != P, depletion, the lane mask of a depleted path, the six outputs and the exact
 *     counts, byte-identical repeat calls, shards merged by smmc_stats_merge and by adding d_depleted_at, n_paths == 0.
 *     A depleted path's draws are still consumed, and its state still moves.
 * A path depends only on (seed, global path id, rg, weights, R, schedule, floor).  Identities, bit for bit on d_final,
 * d_holdings, d_paid, d_ruin_period and d_depleted_at, and on the record's integer fields, min, max and buckets (sum and
 * sumsq follow the launch shape, which is the parent's: the grid rule is the same):
 *   1. means[0] == means[1] and factor[0] == factor[1], with any probabilities, is
 *      smmc_engine_simulate_portfolio_cashflow in Gaussian mode with those means and that factor;
 *   2. start1_q16 = 0 and leave_q16[0] = 0 is that call with regime 0's law whatever regime 1 holds; start1_q16 = 65536
 *      and leave_q16[1] = 0 is that call with regime 1's law;
 *   3. K = 1, w_0 = 1, zero flows and floor 0 give the final values of smmc_engine_simulate_regimes with mean[r] =
 *      means[r][0] and std[r] = factor[r][0], for any R, while every value stays finite and above 0;
 *   4. for P' < P, d_ruin_period restricted to values <= P' and d_depleted_at[1 .. P'] of the P-period run equal those of
 *      the P'-period run of the same schedule prefix. */
typedef struct smmc_portfolio_regimes {
  uint32_t struct_size;                               /* = sizeof(smmc_portfolio_regimes) = 184 */
  uint32_t leave_q16[2];                              /* as smmc_regimes */
  uint32_t start1_q16;                                /* as smmc_regimes */
  float means[2][SMMC_MAX_ASSETS];                    /* regime r, asset k: percent per period; 0 at k >= K */
  float factor[2][SMMC_MAX_ASSETS * SMMC_MAX_ASSETS]; /* regime r: lower-triangular L_r, laid out as smmc_portfolio.factor */
  uint32_t reserved[2];                               /* 0 */
} smmc_portfolio_regimes;

/* out holds DEVICE pointers as in the parent; asynchronous on the engine stream.
 * SMMC_ERR_INVALID with a text, before any device work: a mode other than SMMC_MODE_GAUSSIAN; SMMC_FLAG_STREAM_V2 or
 * SMMC_FLAG_STREAM_REF; everything smmc_engine_simulate_portfolio_cashflow refuses of sim, pf, cf and out; a non-zero
 * pf->means or pf->factor entry; NULL rg or a wrong struct_size; a q16 above 65536; in either regime a mean or factor
 * entry that is not finite, a non-zero entry above the diagonal or at k >= K, a negative diagonal; a reserved word != 0;
 * draw tables, depletion counters and histogram beyond the device's LDS less 2048 bytes. */
int smmc_engine_simulate_portfolio_cashflow_regimes(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                    const smmc_portfolio_regimes *rg, const smmc_cashflow *cf,
                                                    const smmc_portfolio_cashflow_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_portfolio_cashflow_regimes_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                            const smmc_portfolio_regimes *rg, const smmc_cashflow *cf,
                                                            const smmc_portfolio_cashflow_outputs *out);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT (never SMMC_DIV_CHECKED, as the parent), or an error of the call's argument checks.
 * The rule of smmc_engine_portfolio_cashflow_divide_kind on the UNION of the two regimes' per-asset bounds: per asset, the
 * smaller of the two lower bounds and the larger of the two upper ones, each regime's as a portfolio with that regime's
 * means and factor has them.  Every multiplier of a path is one regime's or the other's, and every condition of the rule
 * is monotone in the bounds.  "FAST in each regime separately" is no proof: the rule's two sufficient conditions could
 * then hold in different regimes, and a path mixes them.  No bounds for a regime is SMMC_DIV_EXACT, also for a regime that
 * is never entered.  Results never depend on the form. */
int smmc_engine_portfolio_cashflow_regimes_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                       const smmc_portfolio_regimes *rg, const smmc_cashflow *cf);

/* ---- portfolio cash-flow checkpoints: the value distribution along a plan ----------------------- */

/* "What does my wealth look like in year 5, 10, 15 ... under this plan": smmc_engine_simulate_portfolio_cashflow with
 * the paths' values reduced also after n_checkpoints chosen periods, one launch (the fan chart of a plan).  Neither
 * keepdata (no cash flows; 4 (n_periods + 1) bytes per path) nor two separate calls can give this.
 * The path: exactly the path of smmc_engine_simulate_portfolio_cashflow for the same (sim, pf, cf) -- recurrence,
 * draws, masks and roundings are that contract's.  The value of a path at period p is v after period p's step: vn
 * while the path is live, 0 from the period of its depletion on.
 * periods[0 .. n_checkpoints): HOST array, strictly increasing, 1 <= periods[k] <= sim->n_periods, 1 <= n_checkpoints <=
 * SMMC_MAX_CHECKPOINTS; may be reused on return.
 * d_records (required, DEVICE, 8-byte aligned): n_checkpoints packed records back to back, smmc_stats_bytes(sim->n_bins)
 * bytes each; record k is what smmc_engine_values_stats would write for the paths' values at periods[k] with sim's
 * below_threshold, n_bins, hist_lo and hist_hi: integer fields, min, max and bucket counts exactly, sum and sumsq as
 * double sums in a fixed order (two identical calls give the same bytes; no floating-point atomics).  Depleted paths are
 * in every record, as the value 0.  n_bins == 0 is allowed (records without buckets).
 * out: every member keeps the meaning it has in smmc_engine_simulate_portfolio_cashflow, may be NULL, and is
 * bit-identical to what that call writes for the same request; of d_stats the integer fields, min, max and bucket counts
 * are identical and sum and sumsq agree within relative 1e-12.
 * Divide: smmc_engine_portfolio_cashflow_divide_kind(e, sim, pf, cf) answers for this call too -- a value already has to
 * be right whenever it meets the floor, so a checkpoint asks nothing more, and SMMC_DIV_CHECKED never applies.
 * Shards merge with smmc_stats_merge per record and by adding d_depleted_at.  n_paths == 0 launches nothing and yields
 * empty records, the empty final record and zero counts.
 * SMMC_ERR_INVALID with a text and without a launch: everything smmc_engine_simulate_portfolio_cashflow refuses;
 * n_checkpoints == 0 or > SMMC_MAX_CHECKPOINTS; a period that is 0, above n_periods or not above the one before it; NULL
 * periods or d_records; a d_records that is not 8-byte aligned; n_checkpoints * n_bins > SMMC_MAX_CHECKPOINT_BINS; asset
 * table (or draw tables), n_periods + 1 depletion counters, n_bins final buckets, n_checkpoints * n_bins checkpoint
 * buckets and the waves' partials beyond the device's LDS less 2048 bytes (the text names both numbers).
 * Asynchronous on the engine stream. */
int smmc_engine_simulate_portfolio_cashflow_checkpoints(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                        const smmc_cashflow *cf, const uint32_t *periods, uint32_t n_checkpoints,
                                                        const smmc_portfolio_cashflow_outputs *out, void *d_records);
/* Synchronous convenience: the same with HOST pointers in out and for the records (no alignment asked of them). */
int smmc_engine_simulate_portfolio_cashflow_checkpoints_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                                                const smmc_cashflow *cf, const uint32_t *periods,
                                                                uint32_t n_checkpoints,
                                                                const smmc_portfolio_cashflow_outputs *out, void *host_records);

/* ---- allocation sweeps: up to eight portfolio strategies on one set of draws, one launch ------- */

/* "Which mix, rebalanced how often, still carries this withdrawal?": n_scenarios (1 .. SMMC_MAX_SWEEP) strategies
 * stepped on the same jointly drawn paths, the draw made once per period (common random numbers, as in
 * smmc_engine_simulate_cashflow_sweep).  Counter stream v3 only.  pfs and cfs are HOST arrays of n_scenarios entries
 * each and may be reused on return; scenario s is (pfs[s], cfs[s]).
 *   - Every pfs[s] passes the checks of smmc_engine_simulate_portfolio on its own.  All of them share the joint law:
 *     n_assets, means and factor equal pfs[0]'s bit for bit; weights and rebalance_every are per scenario.  Table mode
 *     uses the engine's asset table (smmc_engine_set_asset_table).
 *   - Every cfs[s] is a CONSTANT schedule (amounts and fractions NULL); amount, fraction and floor are per scenario.
 * Scenario s IS smmc_engine_simulate_portfolio_cashflow(sim, &pfs[s], &cfs[s]): final, holdings, paid, ruin_period,
 * depleted_at and the record's integer fields, min, max and bucket counts are that call's bit for bit; sum and sumsq
 * are double sums in a fixed order of the sweep's own (no floating-point atomics: two identical sweeps give the same
 * bytes) and agree with the single call's to 1e-12 relative.  A path depends on (seed, global path id, law, its own
 * scenario) only: not on the other scenarios, on n_scenarios, on first_path or on the launch geometry.  Shards merge
 * by smmc_stats_merge and by adding d_depleted_at, scenario by scenario.
 *
 * Divide by 100: the reciprocal-multiply form if and only if smmc_engine_portfolio_cashflow_divide_kind says
 * SMMC_DIV_FAST for EVERY scenario; otherwise, or with SMMC_FLAG_EXACT_DIV, the IEEE divide for all of them
 * (smmc_engine_allocation_sweep_divide_kind says which).  Results never depend on the form. */
typedef struct smmc_allocation_sweep_outputs {
  uint32_t struct_size, reserved; /* = sizeof(smmc_allocation_sweep_outputs), 0 */
  float *d_final;          /* [n_scenarios][n_paths] final values, 0 for a depleted path */
  float *d_holdings;       /* [n_scenarios][K][n_paths] final holdings, asset-major inside a scenario */
  float *d_paid;           /* [n_scenarios][n_paths] totals paid out */
  uint32_t *d_ruin_period; /* [n_scenarios][n_paths] periods of depletion, 0 = never */
  void *d_stats;           /* n_scenarios packed records of smmc_stats_bytes(n_bins) bytes each */
  uint64_t *d_depleted_at; /* [n_scenarios][n_periods + 1] counts; every row sums to n_paths */
} smmc_allocation_sweep_outputs;

/* Enqueues one sweep on the engine stream and returns without waiting.  out holds DEVICE pointers (4-byte aligned,
 * d_stats and d_depleted_at 8-byte), any may be NULL; they are written, not accumulated into.  n_paths == 0 launches
 * nothing and yields empty records and zero counts.
 * SMMC_ERR_INVALID with a text, before any device work: everything smmc_engine_simulate_portfolio_cashflow refuses, for
 * any scenario; NULL pfs or cfs; n_scenarios 0 or above SMMC_MAX_SWEEP; a scenario with amounts or fractions; a
 * scenario whose n_assets, means or factor differ from pfs[0]'s (the text names the scenario and the field);
 * n_scenarios * (n_periods + 1 + n_bins) above SMMC_MAX_SWEEP_COUNTERS, n_bins counting as 0 when d_stats is NULL;
 * asset table, counters and partials beyond the device's LDS; 2^32 paths or more per workgroup (shard the request); a
 * NULL or wrongly sized out, or reserved != 0. */
int smmc_engine_simulate_allocation_sweep(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs,
                                          const smmc_cashflow *cfs, uint32_t n_scenarios,
                                          const smmc_allocation_sweep_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_allocation_sweep_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs,
                                                  const smmc_cashflow *cfs, uint32_t n_scenarios,
                                                  const smmc_allocation_sweep_outputs *out);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT: the divide a sweep of (sim, pfs, cfs) uses, or an error of that call's checks on
 * the scenarios. */
int smmc_engine_allocation_sweep_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pfs,
                                             const smmc_cashflow *cfs, uint32_t n_scenarios);

/* ---- real cash flows: the schedule in money of period 0, inflation drawn jointly with the assets ---- */

/* "4 % of the starting capital, raised with prices every year": smmc_engine_simulate_portfolio_cashflow with the
 * schedule's amounts and floor stated in money of period 0 and a price index that differs per path, because inflation
 * is one more series of the joint law: the same resampled month as the returns (table mode), correlated normals
 * (Gaussian mode).  Counter stream v3 only.
 *
 * pf is an smmc_portfolio with n_assets = K INVESTED assets, 1 <= K <= SMMC_MAX_ASSETS - 1.  The joint law has K + 1
 * series and series K is inflation in percent per period:
 *   - table mode: the engine's asset table (smmc_engine_set_asset_table) must have exactly K + 1 columns; the row of
 *     period t is the portfolio contract's row i_t;
 *   - Gaussian mode: means[K] and row K of factor describe inflation and may be non-zero; series K takes the Philox
 *     blocks with fourth word 1 + 2 K and the same chain of fused multiply-adds as any asset;
 *   - weights[K] must be 0, and every entry beyond K + 1 must be 0: the checks of smmc_engine_simulate_portfolio apply
 *     with the law's width K + 1.
 * cf is an smmc_cashflow with unchanged meaning and checks, except that amount / amounts[] and floor are in money of
 * period 0.  Fractions are fractions of the nominal value, as before.
 *
 * Per path, every operation ONE binary32 rounding, nothing fused, every comparison false for NaN; a_k(t), k = 0 .. K,
 * are the joint multipliers of the portfolio contract at width K + 1:
 *   start        h_k = fl(capital * w_k) (k < K);  I = 1.0f;  paid = 0;  ruin = 0;  alive
 *   t = 1 .. P   h_k = fl(fl(h_k * a_k(t)) / 100.0f)               k < K, as the portfolio step
 *                I   = fl(fl(I * a_K(t)) / 100.0f)                 the price index; on every path, depleted or not
 *                g   = (h_0 + h_1) + h_2                           left to right over K
 *                w   = fl(fl(amount[t-1] * I) + fl(g * fraction[t-1]))
 *                vn  = fl(g - w)
 *     live, vn > fl(floor * I):   exactly the live branch of smmc_engine_simulate_portfolio_cashflow (paid += w,
 *                                 rebalance or settle at the weights)
 *     live, otherwise:            exactly its depletion branch (h_k = 0, v = 0, paid += fmaxf(g, 0), ruin = t)
 *     depleted:                   nothing but I changes
 *   final = v;  index = I after period P;  final_real = v / I  (ONE IEEE-correct binary32 division per path, after the
 *   loop, whatever the form of the divide by 100)
 * paid is NOMINAL money.  A path depends only on (seed, global path id, law, weights, R, schedule, floor).
 *
 * Identities:
 *   1. Inflation identically 0 % -- a column of zeros; means[K] = 0 with row K of factor zero -- gives I == 1 throughout:
 *      final, holdings, paid, ruin_period, depleted_at and the record are those of
 *      smmc_engine_simulate_portfolio_cashflow on the first K series, bit for bit, and final_real == final.
 *   2. amount = 0, no amounts[] and floor = 0: the nominal outputs are the parent's on the first K series bit for bit,
 *      whatever the inflation series is (table mode: the row depends on n_rows only; Gaussian mode: asset j's normals
 *      depend on j only) -- while the index stays finite: 0 * inf is NaN.
 *   3. A constant inflation column c in table mode gives one deterministic sequence I_t; with floor = 0 the nominal
 *      outputs are the parent's with amounts[t-1] = fl(amount * I_t), bit for bit. */
typedef struct smmc_real_cashflow_outputs {
  uint32_t struct_size, reserved; /* = sizeof(smmc_real_cashflow_outputs), 0 */
  float *d_final;          /* n_paths nominal final values, 0 for a depleted path */
  float *d_final_real;     /* n_paths final values in money of period 0: final / index */
  float *d_index;          /* n_paths price indices after period P */
  float *d_holdings;       /* nominal final holdings, asset-major K x n_paths */
  float *d_paid;           /* n_paths totals paid out, nominal */
  uint32_t *d_ruin_period; /* n_paths periods of depletion, 0 = never */
  void *d_stats;           /* packed record of the REAL final values, smmc_stats_bytes(n_bins) */
  uint64_t *d_depleted_at; /* n_periods + 1 counts: [0] never depleted, [t] depleted at period t; their sum is n_paths */
} smmc_real_cashflow_outputs;

/* Enqueues one such simulation on the engine stream and returns without waiting; the host arrays of cf may be reused on
 * return.  out holds DEVICE pointers (4-byte aligned, d_stats and d_depleted_at 8-byte), any may be NULL; they are
 * written, not accumulated into.  Exactness of the record's fields, determinism (two identical calls give the same
 * bytes), shard merging (smmc_stats_merge, adding d_depleted_at) and n_paths == 0 (no launch, the empty record, zero
 * counts) are as in smmc_engine_simulate_portfolio_cashflow.
 * SMMC_ERR_INVALID with a text, and no launch: everything smmc_engine_simulate_portfolio_cashflow refuses, checked with
 * the law's width K + 1; n_assets == SMMC_MAX_ASSETS; weights[K] != 0; an asset table whose column count is not K + 1;
 * a NULL or wrongly sized out, or reserved != 0. */
int smmc_engine_simulate_real_cashflow(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                       const smmc_real_cashflow_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_real_cashflow_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                               const smmc_cashflow *cf, const smmc_real_cashflow_outputs *out);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT (never SMMC_DIV_CHECKED), or an error of the call's argument checks.  Results never
 * depend on the form.  The nominal amount varies with the index, so the parent's proof for "one constant amount" does
 * not carry over; the reciprocal-multiply form is used only when BOTH hold, with the multiplier bounds of
 * smmc_engine_portfolio_divide_kind for every series (lo_I, hi_I: those of series K, divided by 100):
 *   the index stays in the window   lo_I^P >= 2^-88 and hi_I^P < 2^126: every product I * a_K is inside [2^-89, 2^127);
 *   contributions only              every amount <= 0 and every fraction 0, a positive capital, every positively
 *                                   weighted asset starting above 0, and (capital + the sum of |amount| *
 *                                   max(1, hi_I)^P) grown by the best asset in every period below 2^126: holdings only
 *                                   gain, and the portfolio rule's lower bound stands.
 * Everything else, or SMMC_FLAG_EXACT_DIV, is the IEEE divide ("Real cash flows", has the proof). */
int smmc_engine_real_cashflow_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                          const smmc_cashflow *cf);

/* ---- guardrails: a withdrawal that a review rule adjusts per path ------------------------------------ */

/* "Take 4 %, index it every year, cut spending by 10 % if the withdrawal rate drifts above 5 %, raise it by 10 % if it
 * falls below 3 %" (Guyton-Klinger style guardrails; with cut = raise = 1 and the clamps, a floor-and-ceiling rule):
 * smmc_engine_simulate_portfolio_cashflow with a constant starting amount that a review after every E-th period
 * adjusts PER PATH.  Every other cash-flow call takes its schedule as fixed before the first draw; here the amount in
 * force is state of the path that feeds back into its value.  pf keeps smmc_portfolio's meaning: weights,
 * rebalance_every = R, the asset table or means and factor, the draws and the checks are exactly as in
 * smmc_engine_simulate_portfolio_cashflow.  Counter stream v3 only. */
typedef struct smmc_guardrails {
  uint32_t struct_size;    /* = sizeof(smmc_guardrails) */
  uint32_t review_every;   /* E: a review after every E-th period; 0 = never */
  float amount;            /* A0 > 0, taken after every period until a review changes it */
  float index;             /* > 0, finite: multiplies the amount at every review (1 = none; 1.02 = +2 % a review) */
  float upper, lower;      /* withdrawal-rate bands per period as fractions of the value; 0 <= lower <= upper; upper may be +inf */
  float cut, raise;        /* 0 < cut <= 1; 1 <= raise, finite */
  float amount_min, amount_max; /* 0 <= amount_min <= A0 <= amount_max; amount_max may be +inf */
  float floor;             /* depleted when !(value > floor); >= 0, finite */
} smmc_guardrails;

/* Per path, every operation ONE binary32 rounding, nothing fused, every comparison false for NaN; a_k(t) are the
 * portfolio contract's multipliers, P = n_periods, 1 <= P <= SMMC_MAX_CASHFLOW_PERIODS:
 *   start      h_k = fl(capital * w_k);  paid = 0;  ruin = 0;  alive;  cur = A0;  lowest = A0;  cuts = raises = 0
 *   t = 1..P   h_k = fl(fl(h_k * a_k(t)) / 100.0f)               IEEE divide, always
 *              g   = ((h_0 + h_1) + h_2) + h_3                    left to right over K
 *              w   = cur;  vn = fl(g - w)
 *     live, vn > floor:    paid = fl(paid + w);  v = vn
 *                          rebalance (R > 0, t mod R == 0, t != P):  h_k = fl(vn * w_k)
 *                          else:                                     h_k = fl(h_k - fl(w * w_k))
 *                          review (E > 0, t mod E == 0, t != P):
 *                            c = fl(cur * index)
 *                            if      c > fl(vn * upper):  c = fl(c * cut);    cuts   += 1;  counted in cuts_at[t]
 *                            else if c < fl(vn * lower):  c = fl(c * raise);  raises += 1;  counted in raises_at[t]
 *                            cur = fminf(fmaxf(c, amount_min), amount_max);  lowest = fminf(lowest, cur)
 *     live, !(vn > floor): depleted at t exactly as the parent: h_k = 0, v = 0, paid = fl(paid + fmaxf(g, 0)), ruin = t;
 *                          no review
 *     depleted:            nothing changes, cur / lowest / counts included; its draws are still consumed
 *   final value = v after period P;  final holdings = h_k after period P (no rebalance and no review at P)
 * What follows from it:
 *   - The bands compare the amount of the NEXT periods with the value AFTER this period's withdrawal.
 *   - E = 0 or E >= P (no review ever happens), or cut = raise = index = 1 with amount_min = 0 and amount_max = +inf,
 *     give smmc_engine_simulate_portfolio_cashflow with the constant amount A0 bit for bit, amount_last ==
 *     amount_lowest == A0 and all counts 0.
 *   - upper = +inf, lower = 0, amount_min = 0 and amount_max = +inf: the amount in force is A0 multiplied by index once
 *     per passed review, the same for every path; the call is the parent with that amounts[] bit for bit.
 *   - Table mode with K = 1, w_0 = 1 is the same rule on smmc_engine_simulate_cashflow's paths.
 *   - The divide by 100 is always the IEEE one: the amount varies per path, the case for which the proof of
 *     smmc_engine_portfolio_cashflow_divide_kind has no fast form.  SMMC_FLAG_EXACT_DIV is accepted and changes
 *     nothing; there is no divide_kind entry.
 *   - A path depends only on (seed, global path id, table or means and factor, weights, R, the smmc_guardrails), never
 *     on first_path, the shard or the launch geometry. */
typedef struct smmc_guardrails_outputs {
  uint32_t struct_size, reserved; /* = sizeof(smmc_guardrails_outputs), 0 */
  float *d_final;          /* n_paths final values, 0 for a depleted path */
  float *d_holdings;       /* final holdings, asset-major K x n_paths */
  float *d_paid;           /* n_paths totals paid out */
  uint32_t *d_ruin_period; /* n_paths periods of depletion, 0 = never */
  void *d_stats;           /* packed record of the final values, smmc_stats_bytes(n_bins) */
  uint64_t *d_depleted_at; /* n_periods + 1 counts: [0] never depleted, [t] depleted at period t; their sum is n_paths */
  float *d_amount_last;    /* n_paths amounts in force after the last review (a depleted path: when it was depleted) */
  float *d_amount_lowest;  /* n_paths lowest amounts ever in force */
  uint32_t *d_cuts;        /* n_paths numbers of cuts */
  uint32_t *d_raises;      /* n_paths numbers of raises */
  uint64_t *d_cuts_at;     /* n_periods + 1 counts: [t] paths cut at the review after period t; [0] is unused and stays 0 */
  uint64_t *d_raises_at;   /* n_periods + 1 counts, likewise */
} smmc_guardrails_outputs;

/* Enqueues one such simulation on the engine stream and returns without waiting.  out holds DEVICE pointers (4-byte
 * aligned; d_stats, d_depleted_at, d_cuts_at and d_raises_at 8-byte), any may be NULL; they are written, not
 * accumulated into.  Integer outputs, min, max and bucket counts are exact; sum and sumsq are double sums in a fixed
 * order, so two identical calls give the same bytes.  Shards merge by smmc_stats_merge and by adding the three count
 * arrays.  n_paths == 0 launches nothing and yields the empty record and zero counts.
 * SMMC_ERR_INVALID with a text: everything smmc_engine_simulate_portfolio refuses for sim and pf (the v2 and ref stream
 * flags among it); a NULL or wrongly sized gr; a field of gr outside the bounds its comment states, or not finite
 * where it must be; n_periods == 0 or above SMMC_MAX_CASHFLOW_PERIODS; a NULL or wrongly sized out, or reserved != 0;
 * asset table, the three counter arrays and histogram beyond the device's LDS; 2^32 or more paths per workgroup (shard
 * the request). */
int smmc_engine_simulate_guardrails(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_guardrails *gr,
                                    const smmc_guardrails_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_guardrails_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf,
                                            const smmc_guardrails *gr, const smmc_guardrails_outputs *out);

/* ---- glide paths: target weights that change along a plan -------------------------------------------- */

/* "90/10 at 30, 40/60 at 70" (a target-date glide path, a bond tent, a rising equity glide path):
 * smmc_engine_simulate_portfolio_cashflow with a list of later target-weight vectors.  sim, pf, cf and the outputs keep
 * that call's meaning, checks, draws, records, depletion counts and shard merging; pf->weights are the targets at the
 * start.  It cannot be composed from outside: with a rebalance and a flow the value after a change of weights is no
 * function of two separate runs, and chained runs would restart the per-path draw counters.  Counter stream v3 only. */
#define SMMC_MAX_GLIDE_CHANGES 512
typedef struct smmc_glide {
  uint32_t struct_size;   /* = sizeof(smmc_glide) */
  uint32_t n_changes;     /* 0 .. SMMC_MAX_GLIDE_CHANGES */
  const uint32_t *after;  /* HOST, n_changes periods, strictly increasing, each >= 1 */
  const float *weights;   /* HOST, n_changes x SMMC_MAX_ASSETS, row c = the targets from change c on; entries k >= K are 0 */
} smmc_glide;

/* A path trades at the end of every period t = 0 .. P (P = n_periods): at t = 0 the initial purchase
 * h_k = fl(capital * w_k), at t >= 1 the trade of smmc_engine_simulate_portfolio_cashflow -- the rebalance
 * h_k = fl(vn * w_k) or the settlement h_k = fl(h_k - fl(w * w_k)).  EVERY trade at the end of period t uses W(t):
 *   W(t) = row c of glide->weights for the largest c with after[c] <= t;  pf->weights while t < after[0].
 * Everything else is that call's recurrence unchanged, each operation one binary32 rounding: the order of operations,
 * vn > floor, depletion, no rebalance at P, the draws.
 * What follows from it:
 *   - A change of targets does NOT trade by itself.  The holdings move to the new targets at the next rebalance, and
 *     flows settle at the new targets from that period on: put a change on a rebalance period to reallocate right there.
 *   - A change with after[c] > P is legal and never reached, so the outputs of the first p periods do not depend on
 *     n_periods beyond that call's own dependence (no rebalance at P).  A change at P acts on the last settlement only:
 *     it moves the final holdings, not the final value.
 *   - n_changes == 0, or every row equal to pf->weights, gives smmc_engine_simulate_portfolio_cashflow's six outputs bit
 *     for bit.
 *   - Zero flows (amount = fraction = 0, floor = 0, no arrays) with rebalance_every == 0 give
 *     smmc_engine_simulate_portfolio's final values and holdings bit for bit whatever the changes are: nothing trades.
 *   - With one asset every legal row is w_0 = 1: the call checks its arguments and is
 *     smmc_engine_simulate_portfolio_cashflow.
 *   - A path depends only on (seed, global path id, table or means and factor, pf, glide, schedule, floor), never on
 *     first_path, the shard or the launch geometry.
 * Enqueues on the engine stream and returns without waiting; the host arrays of cf and glide may be reused on return.
 * out as smmc_engine_simulate_portfolio_cashflow takes it (DEVICE pointers, any may be NULL); n_paths == 0 launches
 * nothing and yields the empty record and zero counts.
 * SMMC_ERR_INVALID with a text: everything smmc_engine_simulate_portfolio_cashflow refuses; a NULL or wrongly sized
 * glide; n_changes > SMMC_MAX_GLIDE_CHANGES; NULL after or weights with n_changes > 0; after not strictly increasing or
 * holding a 0; a row that fails smmc_portfolio's weight checks (negative, not finite, non-zero at k >= K, a sum off 1 by
 * more than 1e-6 in double). */
int smmc_engine_simulate_glide(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                               const smmc_glide *glide, const smmc_portfolio_cashflow_outputs *out);
/* Synchronous convenience: the same with HOST pointers in out. */
int smmc_engine_simulate_glide_to_host(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                       const smmc_glide *glide, const smmc_portfolio_cashflow_outputs *out);
/* SMMC_DIV_FAST or SMMC_DIV_EXACT (never SMMC_DIV_CHECKED), or an error of the call's argument checks.  Results never
 * depend on the form.  FAST only if both hold: (1) every row weights the same set of assets positively as pf->weights
 * does -- an asset whose target is 0 for a stage is no longer bounded from below by its share, and the holding it keeps
 * from the stage before shrinks without a bound the host knows; (2) the rule of
 * smmc_engine_portfolio_cashflow_divide_kind with the smallest positive weight, the smallest share fl(amount * w_k) and
 * the smallest floor * w_k taken over pf->weights and EVERY row (the rows beyond P too).  Anything else, or
 * SMMC_FLAG_EXACT_DIV, is the IEEE divide ("Glide paths", carries the proof over). */
int smmc_engine_glide_divide_kind(smmc_engine *e, const smmc_sim *sim, const smmc_portfolio *pf, const smmc_cashflow *cf,
                                  const smmc_glide *glide);

/* Blocks until everything enqueued on the engine stream has finished. */
int smmc_engine_sync(smmc_engine *e);

/* Progress callback of the synchronous *_to_host entry points: called on the calling thread
 * with the number of paths whose results are in the caller's memory -- 0 at the start, after every
 * finished chunk, n_paths at the end.  The C++ drop-in layer stores it into the caller's
 * std::atomic<long> n_simulations (src/simulations.cpp:254; polled by
 * examples/visualize_returns_cpu_v2.cpp:360-376).  NULL clears it. */
typedef void (*smmc_progress_fn)(void *user, int64_t finished_paths);
int smmc_engine_set_progress(smmc_engine *e, smmc_progress_fn fn, void *user);

/* Simulates into HOST memory: outputs are produced in chunks of 2^22 paths and
 * copied back on a side stream while the next chunk computes (the async
 * cudaMemcpy pattern of mc_simulations_multi_gpu_launcher_async,
 * src/simulations.cu:615-626, without its extra host copy :643-644).
 * Host pointers (pinned or pageable), any may be NULL:
 *   host_final       n_paths floats
 *   host_chunk_mean  ceil(n_paths / SMMC_CHUNK) floats  (means of the reduceBlock API)
 *   host_chunk_var   same length                         (variances)
 *   progress         set (atomic release store) to the number of finished paths after every
 *                    chunk (the n_simulations counter of src/simulations.cpp:254); when it or a
 *                    progress callback is given, chunks shrink to about n_paths / 16 (at least
 *                    2^16 paths) so that a poller sees the run advance
 * Environment: SMMC_PIN_HOST=whole|chunk|0: a host_final of 32 MiB or more that is not pinned
 * already is page-locked (hipHostRegister, whole pages) for the duration of the call -- the whole
 * buffer up front (default: registration runs at 25-75 GB/s and lets the copies overlap the kernels),
 * or chunk by chunk one chunk ahead of the copies (every page has one owning chunk), or not at all; a
 * failed registration falls back to the pageable copy (reported under SMMC_VERBOSE).
 * SMMC_HOST_CHUNK_PATHS overrides the chunk length.  The per-path values, the chunk means / variances,
 * the counters, min / max and the histogram never depend on the chunk length (and so not on whether
 * progress is polled); sum and sumsq are double sums of the per-chunk records in chunk order and can
 * differ in their last bits between two chunkings.
 *   stats, hist      merged statistics header and n_bins bucket counts
 * Synchronous. */
int smmc_engine_simulate_to_host(smmc_engine *e, const smmc_sim *sim, float *host_final,
                                 float *host_chunk_mean, float *host_chunk_var, volatile int64_t *progress,
                                 smmc_stats *stats, uint64_t *hist);

/* Optional: allocates now what the next smmc_engine_simulate_to_host of up to n_paths final values will
 * need on the device (its two staging buffers), so that the first call of a process does not pay for it
 * -- e.g. while another host thread sizes the result buffer.  Results never depend on it. */
int smmc_engine_prepare_host(smmc_engine *e, uint64_t n_paths);

/* Page-locks / releases a caller's host buffer (hipHostRegister over its whole pages, visible to every
 * device): a buffer registered here is used as it is by smmc_engine_simulate_to_host and
 * smmc_group_simulate (no registration per call; 12-15 ms per 400 MB the first time).  A buffer that is
 * pinned already is left alone (SMMC_OK; smmc_host_unregister of it is then a no-op). */
int smmc_host_register(void *host_ptr, uint64_t bytes);
int smmc_host_unregister(void *host_ptr);

/* keepdata into HOST memory: host_traj is n_paths x (n_periods + 1) floats path-major,
 * host_final (may be NULL) n_paths floats.  Produced in device-sized slices.
 * Synchronous.  mc_simulations_keepdata, src/simulations.cpp:139-202. */
int smmc_engine_simulate_keepdata_to_host(smmc_engine *e, const smmc_sim *sim, float *host_traj,
                                          float *host_final);

/* ---- statistics of values already in HBM ---------------------------- */

#define SMMC_MAX_RANKS 8

/* One pass over n device floats -> packed statistics record (d_stats, device,
 * smmc_stats_bytes(n_bins) bytes): sum, sum of squares, count below a threshold, min,
 * max, bucket histogram.  Replaces the host passes update_mean_std and
 * update_count_below_min of the reference's callers (examples/visualize_returns_cpu_v2.cpp:
 * 113-138, examples/benchmark_mc_gpu.cpp:7-41) on data that never leaves the GPU.
 * Asynchronous on the engine stream. */
int smmc_engine_values_stats(smmc_engine *e, const float *d_values, uint64_t n, float below_threshold,
                             uint32_t n_bins, float hist_lo, float hist_hi, void *d_stats);

/* Exact order statistics: host_out[q] = the ranks[q]-th smallest (0-based) of n device
 * floats, n_ranks <= SMMC_MAX_RANKS, every rank < n.  Three histogram passes of radix
 * selection; the input is not modified or copied.  Synchronous. */
int smmc_engine_order_statistics(smmc_engine *e, const float *d_values, uint64_t n, const uint64_t *ranks,
                                 uint32_t n_ranks, float *host_out);

/* {min, Q1, Q2, Q3, max} with Q1 = n/4, Q2 = n/2, Q3 = Q1 + Q2 as ranks in sorted order:
 * update_quartiles, examples/visualize_returns_cpu_v2.cpp:83-111.  n >= 1.  Synchronous. */
int smmc_engine_quartiles(smmc_engine *e, const float *d_values, uint64_t n, float host_out[5]);

/* Mean of n HOST floats: chunked host-to-device copy + values_stats, double
 * accumulation; *mean = (float)sum / n as the CPU check of
 * examples/benchmark_reduce_mean.cpp:31-32.  reduce_mean_gpu, src/simulations.cu:269-341
 * (which sums in float by an in-place strided tree and overflows int indices beyond
 * 2^31 elements).  sum may be NULL.  Synchronous. */
int smmc_engine_reduce_mean_host(smmc_engine *e, const float *host_values, uint64_t n, float *mean, double *sum);

/* The same two operations on n HOST floats (copied to the device once, synchronous):
 * what update_quartiles / update_mean_std / update_count_below_min of the reference's
 * examples do on their std::vector.  stats and hist may be NULL, quartiles may be NULL. */
int smmc_engine_host_values_summary(smmc_engine *e, const float *host_values, uint64_t n, float below_threshold,
                                    uint32_t n_bins, float hist_lo, float hist_hi, smmc_stats *stats,
                                    uint64_t *hist, float quartiles[5]);

/* Device-time instrumentation: when enabled, every simulate call brackets its
 * main kernel with HIP events on the engine stream.  smmc_engine_kernel_ms
 * synchronises, returns the number of timed launches and their summed duration
 * in milliseconds, and clears the log. */
int smmc_engine_timing(smmc_engine *e, int enable);
int smmc_engine_kernel_ms(smmc_engine *e, double *total_ms, uint32_t *launches);
/* With timing enabled every workgroup of the path kernel also adds the shader clocks and the 100 MHz ticks of its
 * own lifetime to two counters: *ghz = the clock the chip HELD, on average over the workgroups of the launches since
 * the last call (0 when nothing was sampled; the reference-stream kernels are not sampled).  Synchronises and
 * clears.  The reference's counterpart is its printed phase timers (src/simulations.cu:351-358): it has no clock
 * read-out. */
int smmc_engine_kernel_clock(smmc_engine *e, double *ghz);

/* Device self-test of the kernels' divide shortcut over the binary32 bit patterns
 * [bits_lo, bits_hi): counts x where the reciprocal-multiply divide differs from the
 * IEEE x / 100.0f.  Synchronous. */
int smmc_engine_selftest(smmc_engine *e, uint32_t bits_lo, uint32_t bits_hi, uint64_t *div_mismatches);

/* Device self-test of the draws: what the kernels make of GIVEN random words.  Item i is the four 32-bit words at
 * words[4 i ..] (host memory), in the place of one Philox block's output; out (host memory) receives per item the
 * *draws_per_item multipliers a = 100 + return that a path would compound with: 8 in table mode with a table of up
 * to 2048 entries, else 4.  Mode, SMMC_FLAG_STREAM_V2, gauss_mean, gauss_std and the engine's table are taken from
 * `sim` exactly as smmc_engine_simulate takes them (seed, paths, periods and the statistics fields are not used),
 * and the words go through the same device functions and the same staged tables as in every simulation kernel, so
 * that a test can reach every bin of the Gaussian radius table, every sector of its angle table and every digit
 * boundary of a table draw on purpose.  form 0 draws one item at a time, form 1 two together (the order of the
 * kernels that interleave two Philox blocks); the values are the same.  SMMC_FLAG_STREAM_REF is refused (its
 * draw is not made of Philox words).  n = 0 sets *draws_per_item (nullable) and touches nothing else; n <= 2^28.
 * Copies in and out itself on the engine's stream.  Synchronous. */
int smmc_engine_selftest_draws(smmc_engine *e, const smmc_sim *sim, const uint32_t *words, uint64_t n, int form,
                               float *out, uint32_t *draws_per_item);

/* Which divide-by-100 a launch of `sim` uses (the result never depends on it): SMMC_DIV_FAST, the
 * reciprocal-multiply form, when the returns table (or mean +- 7 std), the capital and the number of
 * periods prove that no path can leave its domain; SMMC_DIV_CHECKED (final-value launches only)
 * when they do not but a per-block range check with an IEEE-divide rerun of the rare offending path
 * is possible; SMMC_DIV_EXACT, the IEEE divide, otherwise or with SMMC_FLAG_EXACT_DIV.
 * keepdata != 0 asks for smmc_engine_simulate_keepdata.  Returns the kind (>= 0) or an error. */
#define SMMC_DIV_FAST 0
#define SMMC_DIV_EXACT 1
#define SMMC_DIV_CHECKED 2
int smmc_engine_divide_kind(smmc_engine *e, const smmc_sim *sim, int keepdata);
/* Which kernel a smmc_engine_simulate launch of `sim` gets (the result never depends on it): 1, the form that holds
 * the path id's bits 63..32 in a scalar register, for counter stream v3 in Gaussian mode or with a table of at most
 * 2048 entries when first_path and first_path + n_paths - 1 share those bits (and their sum does not wrap) and
 * smmc_set_uniform_hi has not switched it off; otherwise 0.  smmc_engine_simulate_to_host decides per chunk.
 * Returns the form (>= 0) or an error. */
int smmc_engine_paths_form(smmc_engine *e, const smmc_sim *sim);
/* Process-wide switch for that form: 0 gives every later launch the generic kernel, 1 (the default) lets the rule
 * above decide.  For A/B runs and for profiles of the generic kernel; results never depend on it.  The library reads
 * no environment variable for it: the Python wrapper maps SMMC_UNIFORM_HI (0 | 1) onto this call before every
 * launch.  SMMC_ERR_INVALID for another value. */
int smmc_set_uniform_hi(int on);

/* Launch geometry the engine will use (workgroups x threads), for reports. */
int smmc_engine_geometry(smmc_engine *e, uint32_t *grid, uint32_t *block, uint32_t *compute_units);

/* ---- several devices of one process ----------------------------------------------------- */

/* A group runs ONE simulation request sharded over several devices of this process and produces ONE
 * merged result: the multi-GPU launcher of the reference (mc_simulations_multi_gpu_launcher_async,
 * src/simulations.cu:576-655, reached through mc_simulations_gpu(..., n_gpus), :661-680) with the
 * defects SURVEY section 0.7 lists removed -- shard g covers floor(N/G) paths plus one of the N mod G
 * leftovers (the reference drops them, :602-603), global path ids are the stream counter so the
 * result does not depend on G (the reference replays the same seeds on every GPU, :120,140), one host
 * thread per device so that all devices compute and copy at once.
 *
 * How the per-device statistics records become one is chosen at creation:
 *   SMMC_MERGE_HOST  every device's record (864 bytes at 100 buckets) is already in host memory when its
 *                    thread returns; they are added in device order.
 *   SMMC_MERGE_RCCL  ncclCommInitAll over the group's devices (once, kept for the group's lifetime;
 *                    librccl.so.1 is opened only then), and per call ONE grouped all-reduce
 *                    (ncclUint64, ncclSum) over [count, below, underflow, overflow] and the bucket
 *                    counts, after which EVERY device holds the merged integer record in its own HBM
 *                    (smmc_group_device_record); the two double sums and min / max are merged on
 *                    the host in device order (an all-reduce would make them arrival-order
 *                    dependent).  Needs distinct devices.
 * Both give the same bits.  DESIGN.md section 7 has the measured cost of each. */
typedef struct smmc_group smmc_group;
#define SMMC_MERGE_HOST 0
#define SMMC_MERGE_RCCL 1

/* devices[0 .. n_devices): HIP device ids; with SMMC_MERGE_HOST a device may appear more than once
 * (each occurrence gets its own engine and stream: several shards on one GPU). */
int smmc_group_create(const int *devices, int n_devices, int merge, smmc_group **out);
void smmc_group_destroy(smmc_group *g);
int smmc_group_size(const smmc_group *g);

/* smmc_engine_set_table on every device of the group.  A table identical to the one the devices hold is not
 * uploaded again.  If a device fails, the devices may hold different tables: the group then refuses table-mode
 * simulations (SMMC_ERR_INVALID) until a smmc_group_set_table has succeeded on all of them. */
int smmc_group_set_table(smmc_group *g, const float *returns_percent, uint32_t n);

/* Progress of smmc_group_simulate, summed over the devices (see smmc_engine_set_progress). */
int smmc_group_set_progress(smmc_group *g, smmc_progress_fn fn, void *user);

/* smmc_engine_simulate_to_host for the whole request: device g simulates its contiguous share of the
 * global path ids sim->first_path .. first_path + n_paths - 1 and streams it to its place in the host
 * arrays (any may be NULL; a pageable host_final of 32 MiB or more is page-locked ONCE for all devices, by the
 * engine's own rules -- SMMC_PIN_HOST, both ends tested for "pinned already" -- and the shards run with
 * SMMC_FLAG_HOST_NOPIN, also when that registration fails);
 * stats / hist receive the merged record.  The chunk arrays need every shard to start on a multiple
 * of SMMC_CHUNK paths: SMMC_ERR_INVALID otherwise.  Synchronous. */
int smmc_group_simulate(smmc_group *g, const smmc_sim *sim, float *host_final, float *host_chunk_mean,
                        float *host_chunk_var, volatile int64_t *progress, smmc_stats *stats, uint64_t *hist);

/* smmc_engine_prepare_host on every device of the group, for its share of n_paths (in parallel). */
int smmc_group_prepare_host(smmc_group *g, uint64_t n_paths);

/* The shard device `index` of the group gets of an n_paths request: its first path (relative to
 * sim->first_path) and its count. */
int smmc_group_shard(const smmc_group *g, uint64_t n_paths, int index, uint64_t *first, uint64_t *count);

/* SMMC_MERGE_RCCL, after a smmc_group_simulate that asked for statistics: the device pointer (on device
 * `index` of the group) of that device's copy of the merged packed record -- integer fields and
 * bucket counts are the merged ones, sum / sumsq / min / max that device's own. */
int smmc_group_device_record(smmc_group *g, int index, void **d_record);

/* Host wall-clock costs in milliseconds, for reports: creating the engines, creating the communicator
 * (opening librccl the first time included; 0 for SMMC_MERGE_HOST), and the merge step of the last
 * smmc_group_simulate. */
int smmc_group_timings(const smmc_group *g, double *engines_ms, double *comm_init_ms, double *last_merge_ms);

/* ---- statistics record helpers (host) --------------------------------------- */

uint64_t smmc_stats_bytes(uint32_t n_bins);
/* dst += src for two packed records with equal n_bins (host memory).  Merging
 * shards in ascending rank order gives a result independent of timing. */
int smmc_stats_merge(void *dst_packed, const void *src_packed);

/* ---- the reference's device demo ------------------------------------------------ */

/* vector_add_gpu, src/gpu.cu:17-47 (kernel impl_vector_add_gpu :8-14): out[i] = a[i] + b[i] for three HOST
 * arrays of n floats, computed on the current device (H2D of a and b, one launch, D2H of out; device
 * memory is allocated and freed inside the call, as in the reference).  north_star names the file beside
 * the engine; it is not part of the hot path.  kernel_seconds (optional): the launch alone, by HIP events
 * -- the figure the reference prints as "GPU time".  n == 0 is a no-op; SMMC_ERR_NO_DEVICE without a GPU. */
int smmc_vector_add(float *out, const float *a, const float *b, int64_t n, double *kernel_seconds);

#ifdef __cplusplus
}
#endif
#endif /* SMMC_H */
