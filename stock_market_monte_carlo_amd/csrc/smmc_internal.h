// smmc_internal.h -- what a kernel translation unit or a launch stub needs, shared with the host units: the argument
// structures, launch_*, *_lds_bytes and the constants (not installed).  Part of the kernels' source digest
// (tools/isa_loop_count.py): what only host units share belongs in smmc_host.h, which is not.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <atomic>

#include "smmc.h"

namespace smmc {

constexpr int kBlock = SMMC_CHUNK;  // threads per workgroup = paths per chunk (4 waves)

// One workgroup's partial statistics; reduced in a fixed order by the finalize kernel.
struct BlockPartial {
  double sum, sumsq;
  unsigned long long count, below, underflow, overflow;
  float min, max;
};

struct KernelArgs {
  int32_t mode;           // SMMC_MODE_*
  const float *table_a;  // device, table_len entries, already 100.0f + r  (MODE_TABLE)
  const float *bm_tables;  // device, Box-Muller radius + trig tables of the launch's stream (MODE_GAUSSIAN), 16-byte aligned
  uint32_t table_len;
  uint32_t key0, key1;   // Philox key = seed lo, hi
  uint64_t first_path;
  uint64_t n_paths;
  uint32_t n_periods;
  float initial_capital;
  float gauss_mean, gauss_std;
  float gauss_shift100;  // 100.0f + gauss_mean: the additive term of counter stream v3's multiplier draw
  int32_t stream;        // Gaussian draw: 2 = counter stream v2 (SMMC_FLAG_STREAM_V2), else v3
  float *d_final;        // nullable
  float *d_chunk_mean;   // nullable
  float *d_chunk_var;    // nullable
  BlockPartial *partials;        // nullable => no statistics
  unsigned long long *d_hist;    // nullable; n_bins counters, zero before the launch: the engine's accumulator, folded by finalize
  uint32_t n_bins;
  float hist_lo, hist_hi;
  double hist_inv;       // (double)n_bins / ((double)hi - (double)lo), computed on the host
  float below_threshold;
  float *d_traj;         // keepdata only: n_paths x (n_periods + 1), path-major
  float chk_lo, chk_hi;  // SMMC_DIV_CHECKED only: the window a path must stay in at Philox-block boundaries
  // Timing instrumentation (smmc_engine_timing): every workgroup of paths_kernel adds the shader clocks
  // (s_memtime) and the 100 MHz ticks (s_memrealtime) of its own lifetime -- their ratio is the clock the chip
  // HELD while this launch ran (smmc_engine_kernel_clock).  nullable.
  unsigned long long *clock_probe;
};

// The reference's own stream (SMMC_FLAG_STREAM_REF, smmc_ref_kernels.hip): per-path mt19937 seeded with
// seed0 + i, libstdc++'s Lemire map onto the table, update_fund -- src/simulations.cpp:240-252.
struct RefArgs {
  const float *table_a;   // device, table_len entries, 100.0f + r
  uint32_t table_len;
  uint32_t reject_below;  // Lemire: an output whose low product word is below (2^32 - T) % T is rejected
  uint32_t seed0;         // path i of the launch seeds its generator with (uint32_t)(seed0 + i)
  uint32_t n_paths;       // <= 2^31 per launch
  uint32_t n_periods;     // windowed kernel: <= ref_windowed_max_outputs()
  float initial_capital;
  float chk_lo, chk_hi;   // SMMC_DIV_CHECKED: as KernelArgs
  float *d_final;         // n_paths floats
  float *d_traj;          // nullable: n_paths rows of n_periods + 1 floats (keepdata)
  uint32_t traj_rows;     // d_traj, state-free kernels: consecutive rows per lane (8, 4, 2 or 1: TrajWriter, smmc_ref_kernels.hip)
  uint32_t *redo_count;   // windowed kernel: paths it left unfinished (appended to redo_list); generic kernel
  uint32_t *redo_list;    //   with redo_list != nullptr: the work items are redo_list[0 .. *redo_count)
  uint32_t *workspace;    // generic kernel: ref_workspace_bytes(grid)
};
uint32_t ref_windowed_max_outputs();
size_t ref_workspace_bytes(uint32_t grid);
size_t ref_windowed_lds_bytes(uint32_t table_len, bool traj);
hipError_t launch_ref_windowed(const RefArgs &a, int div, uint32_t grid, hipStream_t stream);
hipError_t launch_ref_generic(const RefArgs &a, bool exact_div, uint32_t grid, hipStream_t stream);
hipError_t launch_chunk_stats(const float *values, uint64_t n, float *d_mean, float *d_var, uint32_t grid,
                              hipStream_t stream);

// values_stats_kernel arguments (smmc_stats_kernels.hip)
struct ValuesArgs {
  const float *values;
  uint64_t n;
  float below_threshold;
  uint32_t n_bins;
  uint32_t hist_copies;  // lane-interleaved LDS histogram copies (values_hist_copies)
  float hist_lo, hist_hi;
  double hist_inv;
  BlockPartial *partials;
  unsigned long long *d_hist;
  // values_stats: every workgroup is resident for the whole launch and flushes its histogram at the
  // same moment; `spread` zeroed copies of the bucket array (workgroup b adds to copy b % spread) cut
  // the adds that queue on one address from 2048 to 128; finalize_kernel folds the copies
  unsigned long long *hist_spread;
  uint32_t spread;
};
uint32_t values_hist_copies(uint32_t n_bins);
constexpr uint32_t kHistSpread = 16;
// Counter stream v3's Box-Muller tables (tools/gen_bm_tables.py; smmc_capi.cpp checks these against the
// generated smmc_bm_tables.inc): sub-intervals per radius octave, sectors of the angle table, and the two
// constants of the residual angle delta = fma(y, K, -C).
constexpr uint32_t kBm3SubBits = 3, kBm3TrigBits = 11, kBm3AngleBits = 30;
constexpr float kBm3AngleK = 0x1.921fb6p-5f, kBm3AngleC = 0x1.9eb0b4p-5f;

// radix selection state: per requested rank, the key bits fixed so far and the rank
// relative to the values that share those bits
constexpr uint32_t kMaxRanks = 8;
struct SelectState {
  uint32_t prefix[kMaxRanks];
  unsigned long long rank[kMaxRanks];
  // ranks that share a prefix share one histogram ("group"): a value then costs at most
  // one LDS atomic per pass however many ranks were asked for
  uint32_t n_groups;
  uint32_t group_prefix[kMaxRanks];
  uint32_t group_of[kMaxRanks];
};

hipError_t launch_values_stats(const ValuesArgs &a, uint32_t grid, hipStream_t stream);
hipError_t launch_radix_hist(const float *values, uint64_t n, int pass, uint32_t n_ranks, const SelectState *st,
                             unsigned long long *g_hist, uint32_t grid, hipStream_t stream);
// also zeroes the part of g_hist the pass counted into (the array is zero between passes and calls)
hipError_t launch_radix_pick(int pass, uint32_t n_ranks, SelectState *st, unsigned long long *g_hist,
                             float *d_out, hipStream_t stream);

// Launch wrappers (defined in smmc_kernels.hip).  All asynchronous on `stream`.
// `div`: SMMC_DIV_* of smmc.h (how a launch divides by 100: simulate_path in smmc_kernels.hip)
hipError_t launch_paths(const KernelArgs &a, int div, uint32_t grid, size_t lds_bytes,
                        hipStream_t stream);
constexpr uint32_t kDenseMaxTable = 2048u;  // largest table drawn eight-per-block
// The process-wide switch of smmc_set_uniform_hi (default 1): read by every launch_paths, so a caller may change it
// between the launches of one process.
inline std::atomic<int> &paths_uniform_hi() {
  static std::atomic<int> on{1};
  return on;
}
// Which kernel launch_paths gives a launch (smmc_engine_paths_form): 1 = paths_hi_kernel, whose period loop takes the
// path id's bits 63..32 from a scalar register (smmc_kernels.hip, kPhiloxUniformHi), 0 = paths_kernel.  1 needs
// counter stream v3, Gaussian draws or a dense table, a range [first_path, first_path + n_paths) inside one multiple
// of 2^32 -- a range that wraps past 2^64 is not -- and the switch above not 0.  The outputs do not depend on it.
inline int paths_form(const KernelArgs &a) {
  if (a.stream == 2 || !a.n_paths) return 0;
  if (a.mode == SMMC_MODE_TABLE && a.table_len > kDenseMaxTable) return 0;
  const uint64_t last = a.first_path + (a.n_paths - 1);
  if (last < a.first_path || (last >> 32) != (a.first_path >> 32)) return 0;
  return paths_uniform_hi().load(std::memory_order_relaxed) ? 1 : 0;
}
// hist_acc: `spread` copies of n_bins bucket counts accumulated by the launch before; folded into the record and zeroed
// again (the engine keeps the array zero between launches: smmc_host.h, ZeroLease)
hipError_t launch_finalize(const BlockPartial *partials, uint32_t n_partials, smmc_stats *d_stats,
                           uint32_t n_bins, hipStream_t stream, unsigned long long *hist_acc, uint32_t spread);
hipError_t launch_keepdata(const KernelArgs &a, bool exact_div, int tile, int waves, uint32_t grid,
                           hipStream_t stream);
// comb form of keepdata (rows [0, 2048 n_super) of a call; see keepdata_comb_kernel)
hipError_t launch_keepdata_comb(const KernelArgs &a, bool exact_div, int blocks_per_step, uint32_t rows_per_stream,
                                uint64_t n_wave_chunks, uint64_t n_rows_total, int waves, uint32_t grid,
                                unsigned long long *next_chunk, hipStream_t stream);
hipError_t launch_final_column(const float *traj, uint64_t n_rows, uint32_t row_len, float *d_final, uint32_t grid,
                               hipStream_t stream);
size_t keepdata_comb_lds_bytes(uint32_t table_len, int waves, int stream);
uint32_t keepdata_draws(uint32_t table_len);
hipError_t launch_selftest(uint32_t lo, uint32_t hi, unsigned long long *d_count, uint32_t grid,
                           hipStream_t stream);
// draw_words_kernel (smmc_engine_selftest_draws): the multipliers that n >= 1 items of four given words yield in the
// launch's mode -- d_words n x 4, d_out n x keepdata_draws(a.table_len) -- through the path kernels' own draw
// functions and staged tables.  form 0: one item at a time; 1: two together (block_multipliers_multi's order).
hipError_t launch_draw_words(const KernelArgs &a, const uint32_t *d_words, uint64_t n, int form, float *d_out, uint32_t grid,
                             hipStream_t stream);
size_t paths_lds_bytes(uint32_t table_len, uint32_t n_bins, int stream);
// checkpoints_kernel (smmc_engine_simulate_checkpoints; counter stream v3 only).  a.partials: n_checkpoints x grid
// entries, [checkpoint][workgroup]; a.d_hist: n_checkpoints x a.n_bins counters, zero before the launch.  A workgroup
// walks chunks of wave_walk_group_paths(mode) consecutive paths.  launch_finalize_checkpoints folds both into the
// n_checkpoints packed records at d_records and leaves the counters zero.
hipError_t launch_checkpoints(const KernelArgs &a, const uint32_t *periods, uint32_t n_checkpoints, bool exact_div,
                              uint32_t grid, hipStream_t stream);
hipError_t launch_finalize_checkpoints(const BlockPartial *partials, uint32_t n_partials, uint32_t n_checkpoints,
                                       void *d_records, uint32_t n_bins, unsigned long long *hist_acc, hipStream_t stream);
// Paths per workgroup of checkpoints_kernel, cashflow_kernel and excursions_kernel alike: 64 per wave, eight waves in
// Gaussian mode (on one copy of the draw tables), four in table mode.
constexpr uint32_t wave_walk_group_paths(int32_t mode) { return mode == SMMC_MODE_TABLE ? 256u : 512u; }
size_t checkpoints_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_checkpoints, uint32_t n_bins);
// cashflow_kernel (smmc_engine_simulate_cashflow, csrc/smmc_cashflow.cpp; counter stream v3 only): the paths of
// paths_kernel with a withdrawal / contribution step after every period's return ("Cash flows").
struct CashflowArgs {
  float amount, fraction;   // every period's entries when `schedule` is null
  float floor;              // a path is depleted when !(value > floor)
  const float *schedule;    // device, nullable: amounts[stride] then fractions[stride]; entries beyond n_periods are 0
  uint32_t stride;          // n_periods rounded up to a multiple of 8 (whole Philox blocks are read)
  float *d_paid;            // nullable: n_paths totals paid out
  uint32_t *d_ruin_period;  // nullable: n_paths periods of depletion, 0 = never
  unsigned long long *d_depleted;  // nullable: n_periods + 1 counters, zero before the launch ([0]: never depleted)
};
// a.partials: `grid` entries (one per workgroup) or null; a.d_hist: a.n_bins counters, zero before the launch.  A
// workgroup walks chunks of wave_walk_group_paths(mode) consecutive paths.
hipError_t launch_cashflow(const KernelArgs &a, const CashflowArgs &c, bool exact_div, uint32_t grid, hipStream_t stream);
// d_out[i] = acc[i] for i < n, and leaves acc zero (the engine's accumulator between launches)
hipError_t launch_finalize_depleted(unsigned long long *acc, uint32_t n, unsigned long long *d_out, hipStream_t stream);
size_t cashflow_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_periods, uint32_t n_bins);
// cashflow_sweep_kernel (smmc_engine_simulate_cashflow_sweep, csrc/smmc_sweep.cpp; counter stream v3 only): c.n constant
// schedules stepped on ONE draw per period ("Cash-flow sweeps").  The kernel is compiled for 2, 4 and 8
// scenarios: entries n .. sweep_width(n) - 1 are copies of entry n - 1 and leave no output.
struct SweepArgs {
  uint32_t n;  // 1 .. SMMC_MAX_SWEEP: the scenarios whose outputs are written
  float amount[SMMC_MAX_SWEEP], fraction[SMMC_MAX_SWEEP], floor[SMMC_MAX_SWEEP];
  float *d_paid;                   // nullable: [n][n_paths]
  uint32_t *d_ruin_period;         // nullable: [n][n_paths]
  unsigned long long *d_depleted;  // nullable: [n][n_periods + 1] counters, zero before the launch
};
constexpr uint32_t sweep_width(uint32_t n) { return n <= 2u ? 2u : n <= 4u ? 4u : 8u; }
// a.d_final: [n][n_paths]; a.partials: [n][grid] entries or null; a.d_hist: [n][a.n_bins] counters, zero before the launch.
hipError_t launch_cashflow_sweep(const KernelArgs &a, const SweepArgs &c, bool exact_div, uint32_t grid, hipStream_t stream);
// Folds partials[scenario][n_partials] and hist_acc[scenario][n_bins] into the n_scenarios packed records at d_records and
// leaves the counters zero: finalize_checkpoints_kernel under the sweep's name (the depletion counts go through
// launch_finalize_depleted).
hipError_t launch_finalize_sweep(const BlockPartial *partials, uint32_t n_partials, uint32_t n_scenarios, void *d_records,
                                 uint32_t n_bins, unsigned long long *hist_acc, hipStream_t stream);
size_t cashflow_sweep_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_periods, uint32_t n_bins, uint32_t n_scenarios);
// excursions_kernel (smmc_engine_simulate_excursions, csrc/smmc_excursions.cpp; counter stream v3 only): the paths of
// paths_kernel with the running extremes, the deepest relative drawdown, the longest time under water and the first
// passage of two levels kept per lane ("Excursions").
struct ExcursionArgs {
  float lower, target;       // first_below: first t with v < lower; first_reach: first t with v >= target
  float drawdown_threshold;  // `below` of the drawdown record
  double dd_hist_inv;        // (double)n_bins: the drawdown histogram spans [0, 1)
  float *d_peak, *d_low, *d_drawdown;  // nullable, n_paths each (the final values go to KernelArgs::d_final)
  uint32_t *d_drawdown_period, *d_underwater, *d_first_below, *d_first_reach;  // nullable, n_paths each
  BlockPartial *dd_partials;        // nullable => no drawdown record; `grid` entries
  unsigned long long *d_dd_hist;    // nullable; a.n_bins counters, zero before the launch
  unsigned long long *d_below_at, *d_reach_at;  // nullable; n_periods + 1 counters each, zero before the launch
};
// a.partials / a.d_hist: the record of the final values, as launch_cashflow.  a.n_bins applies to both histograms.
hipError_t launch_excursions(const KernelArgs &a, const ExcursionArgs &x, bool exact_div, uint32_t grid, hipStream_t stream);
// (the count arrays are copied out, and the accumulator left zero, by launch_finalize_depleted)
size_t excursions_lds_bytes(int32_t mode, uint32_t table_len, uint32_t n_periods, uint32_t n_bins);
// blocks_kernel (smmc_engine_simulate_blocks, csrc/smmc_blocks.cpp; counter stream v3, table mode): the outputs of
// launch_paths for paths drawn in runs of block_len consecutive table entries ("Block bootstrap").
// `wide`: four shifted copies of the table in LDS, read 16 bytes at a time; else one copy read 4 bytes at a time.
// `grid` workgroups of kBlock threads, one partial each.
hipError_t launch_blocks(const KernelArgs &a, uint32_t block_len, bool wide, int div, uint32_t grid, hipStream_t stream);
size_t blocks_lds_bytes(uint32_t table_len, uint32_t n_bins, bool wide);
// stationary_kernel (smmc_engine_simulate_stationary, csrc/smmc_stationary.cpp; counter stream v3, table mode): the
// outputs of launch_paths for paths that start a new run of consecutive table entries with probability renew_q16 / 65536
// at every period ("Stationary bootstrap").  renew_q16 <= SMMC_RENEW_Q16_ONE; `grid` workgroups of kBlock
// threads, one partial each; one plain copy of the table in LDS.
hipError_t launch_stationary(const KernelArgs &a, uint32_t renew_q16, int div, uint32_t grid, hipStream_t stream);
size_t stationary_lds_bytes(uint32_t table_len, uint32_t n_bins);
// regimes_kernel (smmc_engine_simulate_regimes, csrc/smmc_regimes.cpp; counter stream v3, Gaussian mode): the outputs of
// launch_paths for paths whose multiplier is fma(scale[s], z, shift100[s]) in a hidden state s that leaves regime r with
// probability leave_q16[r] / 65536 at every period ("Regime-switching Gaussian paths").  a.gauss_std = 1.0f and
// a.gauss_shift100 = 0.0f (the staged draw yields standard normals, as launch_portfolio's); every q16 <=
// SMMC_REGIME_Q16_ONE; `grid` workgroups of kBlock threads, one partial each.
struct RegimeArgs {
  float scale[2];     // std[r]
  float shift100[2];  // 100.0f + mean[r], rounded once
  uint32_t leave_q16[2];
  uint32_t start1_q16;
};
hipError_t launch_regimes(const KernelArgs &a, const RegimeArgs &r, int div, uint32_t grid, hipStream_t stream);
size_t regimes_lds_bytes(uint32_t n_bins);
// portfolio_kernel (smmc_engine_simulate_portfolio, csrc/smmc_portfolio.cpp; counter stream v3 only): K jointly drawn
// assets per path, held with weights and rebalanced every `rebalance_every` periods ("Portfolios").
// Table mode: a.table_a is the asset table, a.table_len rows of portfolio_row_words(K) words (a = 100.0f + r, padding
// 0).  Gaussian mode: a.gauss_std = 1.0f and a.gauss_shift100 = 0.0f (the staged draw yields standard normals).
struct PortfolioArgs {
  uint32_t n_assets, rebalance_every;
  float weights[SMMC_MAX_ASSETS];
  float shift100[SMMC_MAX_ASSETS];                   // s_k = 100.0f + means[k]
  float factor[SMMC_MAX_ASSETS * SMMC_MAX_ASSETS];  // L, row-major
  float *d_holdings;                                 // nullable: n_assets x n_paths, asset-major
};
constexpr uint32_t portfolio_row_words(uint32_t n_assets) { return n_assets == 3u ? 4u : n_assets; }  // 1, 2 or 4
// a.partials: `grid` entries or null; a.d_hist: a.n_bins counters, zero before the launch.  A workgroup walks chunks of
// wave_walk_group_paths(mode) consecutive paths.
hipError_t launch_portfolio(const KernelArgs &a, const PortfolioArgs &p, bool exact_div, uint32_t grid, hipStream_t stream);
size_t portfolio_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_bins);
// portfolio_cashflow_kernel (smmc_engine_simulate_portfolio_cashflow, csrc/smmc_portfolio_cashflow.cpp; counter stream
// v3 only): portfolio_kernel's holdings and joint draws with cashflow_kernel's step on their sum after every period
// ("Portfolio cash flows").  p and c as launch_portfolio and launch_cashflow take them; a.partials, a.d_hist
// and c.d_depleted as launch_cashflow.
struct PortfolioCashflowArgs {
  PortfolioArgs p;
  CashflowArgs c;
};
hipError_t launch_portfolio_cashflow(const KernelArgs &a, const PortfolioCashflowArgs &x, bool exact_div, uint32_t grid,
                                     hipStream_t stream);
size_t portfolio_cashflow_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins);
// portfolio_cashflow_blocks_kernel (smmc_engine_simulate_portfolio_cashflow_blocks, csrc/smmc_portfolio_cashflow_blocks.cpp;
// counter stream v3, table mode): portfolio_cashflow_kernel's recurrence on runs of block_len consecutive rows of the asset
// table, each run starting at the row the portfolio's table stream draws ("Block-bootstrap plans").  p, c,
// a.partials, a.d_hist and c.d_depleted as launch_portfolio_cashflow; c.stride >= a.n_periods.
struct PortfolioCashflowBlocksArgs {
  PortfolioArgs p;
  CashflowArgs c;
  uint32_t block_len;  // L >= 1
};
// Rows as staged: row i holds table row i mod n_rows, so that a segment of 8 consecutive periods that begins at any row
// below n_rows reads on without a wrap.
constexpr uint32_t portfolio_cashflow_blocks_rows(uint32_t n_rows) { return n_rows + 7u; }
hipError_t launch_portfolio_cashflow_blocks(const KernelArgs &a, const PortfolioCashflowBlocksArgs &x, bool exact_div, uint32_t grid,
                                            hipStream_t stream);
// [portfolio_cashflow_blocks_rows(n_rows) padded rows][n_periods + 1 depletion counters][n_bins buckets][pad][the waves' partials]
size_t portfolio_cashflow_blocks_lds_bytes(uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins);
// portfolio_cashflow_stationary_kernel (smmc_engine_simulate_portfolio_cashflow_stationary,
// csrc/smmc_portfolio_cashflow_stationary.cpp; counter stream v3, table mode): portfolio_cashflow_kernel's recurrence on
// rows chosen by the stationary bootstrap -- the row the portfolio's table stream draws where a period's renewal field is
// below renew_q16, else the row behind the one before ("Stationary-bootstrap plans").  p, c, a.partials,
// a.d_hist and c.d_depleted as launch_portfolio_cashflow; c.stride >= a.n_periods.
struct PortfolioCashflowStationaryArgs {
  PortfolioArgs p;
  CashflowArgs c;
  uint32_t renew_q16;  // <= SMMC_RENEW_Q16_ONE
};
// (the launch and the LDS need are named for the runs' geometric lengths, not "stationary": tests/test_stationary_cpu.py
// lets only smmc_stationary.cpp refer to a symbol of that word)
hipError_t launch_portfolio_cashflow_geometric(const KernelArgs &a, const PortfolioCashflowStationaryArgs &x, bool exact_div, uint32_t grid,
                                                hipStream_t stream);
// [n_rows padded rows, one plain copy][n_periods + 1 depletion counters][n_bins buckets][pad][the waves' partials]
size_t portfolio_cashflow_geometric_lds_bytes(uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins);
// portfolio_cashflow_regimes_kernel (smmc_engine_simulate_portfolio_cashflow_regimes,
// csrc/smmc_portfolio_cashflow_regimes.cpp; counter stream v3, Gaussian mode): portfolio_cashflow_kernel's recurrence on
// multipliers of the regime a path is in -- regimes_kernel's hidden state, drawn from the same fields -- each regime with
// a shift and a factor of its own ("Regime-switching plans").  p gives n_assets, weights, rebalance_every and
// d_holdings; p.shift100 and p.factor are not read.  c, a.partials, a.d_hist and c.d_depleted as
// launch_portfolio_cashflow; a.gauss_std = 1.0f and a.gauss_shift100 = 0.0f; every q16 <= SMMC_REGIME_Q16_ONE.
struct PortfolioCashflowMarkovArgs {
  PortfolioArgs p;
  CashflowArgs c;
  float shift100[2][SMMC_MAX_ASSETS];                   // regime r: s_k = 100.0f + means[r][k]
  float factor[2][SMMC_MAX_ASSETS * SMMC_MAX_ASSETS];  // regime r: L_r, row-major
  uint32_t leave_q16[2];
  uint32_t start1_q16;
};
// (the launch, its arguments and the LDS need are named for the Markov chain, not for its states: tests/test_regimes_cpu.py
// lets only smmc_regimes.cpp refer to a symbol of that word)
hipError_t launch_portfolio_cashflow_markov(const KernelArgs &a, const PortfolioCashflowMarkovArgs &x, bool exact_div, uint32_t grid,
                                            hipStream_t stream);
// [v3 draw tables at scale 1][n_periods + 1 depletion counters][n_bins buckets][pad][the waves' partials]
size_t portfolio_cashflow_markov_lds_bytes(uint32_t n_periods, uint32_t n_bins);
// portfolio_cashflow_checkpoints_kernel (smmc_engine_simulate_portfolio_cashflow_checkpoints,
// csrc/smmc_portfolio_cashflow_checkpoints.cpp; counter stream v3 only): portfolio_cashflow_kernel's paths, with the
// record of their values after each of n chosen periods ("Portfolio cash-flow checkpoints").  p, c, a.partials,
// a.d_hist and c.d_depleted as launch_portfolio_cashflow; a.n_bins applies to the final record and to every checkpoint's.
struct PortfolioCashflowCheckpointsArgs {
  PortfolioArgs p;
  CashflowArgs c;
  uint32_t n;                              // 1 .. SMMC_MAX_CHECKPOINTS
  uint32_t periods[SMMC_MAX_CHECKPOINTS];  // strictly increasing, 1 .. n_periods; entries from n on: 0xffffffff
  BlockPartial *ck_partials;               // n x grid entries, [checkpoint][workgroup]
  unsigned long long *d_ck_hist;           // n x a.n_bins counters, zero before the launch; nullable when a.n_bins == 0
};
// launch_finalize_checkpoints folds x.ck_partials and x.d_ck_hist into the n packed records, launch_finalize the final one.
hipError_t launch_portfolio_cashflow_checkpoints(const KernelArgs &a, const PortfolioCashflowCheckpointsArgs &x, bool exact_div,
                                                 uint32_t grid, hipStream_t stream);
// [front: the padded rows or the draw tables, later the waves' checkpoint partials][n_periods + 1 depletion counters]
// [n_bins final buckets][n_checkpoints x n_bins checkpoint buckets][pad][the waves' partials of the final record]
size_t portfolio_cashflow_checkpoints_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins,
                                                uint32_t n_checkpoints);
// real_cashflow_kernel (smmc_engine_simulate_real_cashflow, csrc/smmc_real_cashflow.cpp; counter stream v3 only):
// portfolio_cashflow_kernel's step with the schedule's amounts and floor in money of period 0, indexed by a price index
// that the LAST series of the joint law compounds ("Real cash flows").  p is the law as launch_portfolio
// takes it, p.n_assets = K + 1 series wide (table rows included): K invested assets, then inflation in percent per
// period; p.weights[K] is 0 and p.d_holdings is K x n_paths.  c, a.partials, a.d_hist and c.d_depleted as
// launch_portfolio_cashflow; the record is of the REAL final values.  LDS: portfolio_cashflow_lds_bytes at width K + 1.
struct RealCashflowArgs {
  PortfolioArgs p;
  CashflowArgs c;
  float *d_final_real;  // nullable: n_paths final values divided by the final index
  float *d_index;       // nullable: n_paths price indices after the last period
};
hipError_t launch_real_cashflow(const KernelArgs &a, const RealCashflowArgs &x, bool exact_div, uint32_t grid, hipStream_t stream);
// guardrails_kernel (smmc_engine_simulate_guardrails, csrc/smmc_guardrails.cpp; counter stream v3 only):
// portfolio_cashflow_kernel's paths with a constant starting amount that a review after every review_every-th period
// adjusts per path ("Guardrails").  p as launch_portfolio takes it; a.partials and a.d_hist as
// launch_cashflow.  Always the IEEE divide: the amount varies per path.
struct GuardrailsArgs {
  PortfolioArgs p;
  uint32_t review_every;  // E; 0: never
  float amount;           // A0: the amount in force until a review changes it
  float index;            // multiplies the amount at every review
  float upper, lower;     // the bands, fractions of the value after the withdrawal
  float cut, raise;       // the factors of a cut and of a raise
  float amount_min, amount_max;
  float floor;            // a path is depleted when !(value > floor)
  float *d_paid;            // nullable: n_paths totals paid out
  uint32_t *d_ruin_period;  // nullable: n_paths periods of depletion, 0 = never
  float *d_amount_last, *d_amount_lowest;  // nullable: n_paths each
  uint32_t *d_cuts, *d_raises;             // nullable: n_paths each
  unsigned long long *d_depleted;               // nullable: n_periods + 1 counters, zero before the launch ([0]: never depleted)
  unsigned long long *d_cuts_at, *d_raises_at;  // nullable: n_periods + 1 counters each, zero before the launch ([0] stays 0)
};
hipError_t launch_guardrails(const KernelArgs &a, const GuardrailsArgs &x, uint32_t grid, hipStream_t stream);
// [the padded rows or the draw tables][three arrays of n_periods + 1 counters: depleted, cuts, raises][n_bins buckets]
// [pad][the waves' partials]
size_t guardrails_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins);
// glide_kernel (smmc_engine_simulate_glide, csrc/smmc_glide.cpp; counter stream v3 only, K = 2, 3, 4):
// portfolio_cashflow_kernel's paths with target weights that change along the plan ("Glide paths").  p and c
// as launch_portfolio_cashflow takes them; p.weights are the targets of period 0 and until the first change.  The
// changes that fall inside the plan are flattened into `table`, one GlideEntry per change in the order they take effect
// and one more behind them that is never read into the weights (next = 0, weights 0): a launch without a change has a
// table of that one entry.
struct GlideEntry {  // 32 bytes, one scalar load
  uint32_t next;                   // periods from this change to the next one; 0: there is none, the countdown never ends
  float weights[SMMC_MAX_ASSETS];  // the targets from this change on; entries k >= K are 0
  uint32_t pad[3];                 // 0
};
static_assert(sizeof(GlideEntry) == 32, "a change is one 32-byte scalar load");
struct GlideArgs {
  PortfolioArgs p;
  CashflowArgs c;
  uint32_t first;           // periods until the first change: after[0]; 0: no change inside the plan
  const GlideEntry *table;  // device, 32-byte aligned, never null
};
hipError_t launch_glide(const KernelArgs &a, const GlideArgs &x, bool exact_div, uint32_t grid, hipStream_t stream);
// allocation_sweep_kernel (smmc_engine_simulate_allocation_sweep, csrc/smmc_allocation_sweep.cpp; counter stream v3
// only): n constant-schedule strategies (weights, rebalance_every, amount, fraction, floor) stepped on ONE joint draw
// per period ("Allocation sweeps").  p: the law as launch_portfolio takes it (n_assets, shift100, factor;
// p.weights and p.rebalance_every are not read), p.d_holdings: [n][n_assets][n_paths].  The kernel is compiled for 4 and
// 8 scenarios: entries n .. allocation_sweep_width(n) - 1 are copies of entry n - 1 and leave no output.
struct AllocationSweepArgs {
  PortfolioArgs p;
  uint32_t n;  // 1 .. SMMC_MAX_SWEEP: the scenarios whose outputs are written
  float weights[SMMC_MAX_SWEEP][SMMC_MAX_ASSETS];
  uint32_t rebalance_every[SMMC_MAX_SWEEP];
  float amount[SMMC_MAX_SWEEP], fraction[SMMC_MAX_SWEEP], floor[SMMC_MAX_SWEEP];
  float *d_paid;                   // nullable: [n][n_paths]
  uint32_t *d_ruin_period;         // nullable: [n][n_paths]
  unsigned long long *d_depleted;  // nullable: [n][n_periods + 1] counters, zero before the launch
};
constexpr uint32_t allocation_sweep_width(uint32_t n) { return n <= 4u ? 4u : 8u; }
// a.d_final: [n][n_paths]; a.partials: [n][grid] entries or null; a.d_hist: [n][a.n_bins] counters, zero before the
// launch (folded by launch_finalize_sweep, the depletion counts by launch_finalize_depleted).
hipError_t launch_allocation_sweep(const KernelArgs &a, const AllocationSweepArgs &x, bool exact_div, uint32_t grid, hipStream_t stream);
size_t allocation_sweep_lds_bytes(int32_t mode, uint32_t n_rows, uint32_t n_assets, uint32_t n_periods, uint32_t n_bins, uint32_t n_scenarios);
size_t keepdata_lds_bytes(uint32_t table_len, int tile, int waves, int stream);
size_t bm_tables_bytes(int stream);  // 2 | 3
hipError_t static_lds_bytes(size_t *bytes);  // of the kernels that address the v3 tables absolutely: 0

}  // namespace smmc
