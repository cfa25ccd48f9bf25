// blocks_args.cpp -- the argument checks of smmc_engine_simulate_blocks, its _to_host form and
// smmc_engine_blocks_divide_kind (include/smmc.h) without a GPU: csrc/smmc_blocks.cpp and the library's other host
// units over tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any
// device work, so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error(); TEST
// INFRASTRUCTURE, driven by tests/test_blocks_cpu.py.  Prints one line per case: "<name> <return code> <length of the
// error text>", then "kind:<case> <SMMC_DIV_*>" lines, then "sizes ...", then "blocks_args: done".
#include <cstdio>
#include <cstring>
#include <vector>

#include "smmc.h"

static smmc_sim make_sim(int32_t mode, uint32_t n_periods, uint32_t n_bins, uint32_t flags) {
  smmc_sim s;
  std::memset(&s, 0, sizeof s);
  s.struct_size = sizeof s;
  s.mode = mode;
  s.seed = 7;
  s.n_paths = 1000;
  s.n_periods = n_periods;
  s.initial_capital = 1000.0f;
  s.gauss_mean = 0.5f;
  s.gauss_std = 0.8f;
  s.n_bins = n_bins;
  s.hist_lo = 0.0f;
  s.hist_hi = 5000.0f;
  s.below_threshold = 1000.0f;
  s.flags = flags;
  return s;
}

static smmc_blocks make_blocks(uint32_t block_len) {
  smmc_blocks b;
  std::memset(&b, 0, sizeof b);
  b.struct_size = sizeof b;
  b.block_len = block_len;
  b.kind = SMMC_BLOCKS_CIRCULAR;
  return b;
}

static void report(const char *name, int rc) {
  std::printf("%s %d %zu\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0));
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr, *no_table = nullptr, *big_table = nullptr, *redo = nullptr, *calm = nullptr;
  for (smmc_engine **p : {&e, &no_table, &big_table, &redo, &calm})
    if (smmc_engine_create(0, nullptr, p) != SMMC_OK) {
      std::printf("engine_create failed: %s\n", smmc_last_error());
      return 1;
    }
  const float table[3] = {1.0f, -2.0f, 0.5f};
  if (smmc_engine_set_table(e, table, 3) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);
  if (smmc_engine_set_table(big_table, largest.data(), SMMC_MAX_TABLE) != SMMC_OK) return 1;
  const float redo_table[8] = {100.0f, 100.0f, 100.0f, 100.0f, 100.0f, -50.0f, -50.0f, -50.0f};
  if (smmc_engine_set_table(redo, redo_table, 8) != SMMC_OK) return 1;
  const float calm_table[2] = {1.0f, -1.0f};
  if (smmc_engine_set_table(calm, calm_table, 2) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats_raw[64 + 8 * 4096];
  static uint64_t hist[4096];
  smmc_stats st;

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim &s, const smmc_blocks *b) {
      if (entry == 0) return smmc_engine_simulate_blocks(eng, &s, b, nullptr, nullptr, nullptr, stats_raw);
      if (entry == 1) return smmc_engine_simulate_blocks_to_host(eng, &s, b, nullptr, nullptr, nullptr, nullptr, &st, hist);
      return smmc_engine_blocks_divide_kind(eng, &s, b);
    };
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    char name[96];
    auto run = [&](const char *what, int rc) {
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc);
    };
    const smmc_sim ok = make_sim(SMMC_MODE_TABLE, 360, 100, 0);
    const smmc_blocks b12 = make_blocks(12);
    run("mode_gaussian", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0), &b12));
    run("no_table", call(no_table, ok, &b12));
    run("stream_v2", call(e, make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_V2), &b12));
    run("stream_ref", call(e, make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF), &b12));
    smmc_blocks bad = make_blocks(0);
    run("block_len_zero", call(e, ok, &bad));
    bad = b12;
    bad.struct_size = sizeof bad - 4;
    run("struct_size_wrong", call(e, ok, &bad));
    bad = b12;
    bad.kind = 1;
    run("kind_not_circular", call(e, ok, &bad));
    bad = b12;
    bad.reserved = 1;
    run("reserved_not_zero", call(e, ok, &bad));
    run("blocks_null", call(e, ok, nullptr));
    run("engine_null", call(nullptr, ok, &b12));
    run("n_bins_above_max", call(e, make_sim(SMMC_MODE_TABLE, 360, SMMC_MAX_BINS + 1, 0), &b12));
    if (entry < 2) {
      // a valid request passes every argument check; what stops it here is that this build has no kernel
      run("valid", call(e, ok, &b12));
      const smmc_blocks huge = make_blocks(0xFFFFFFFFu);  // L may exceed T and n_periods
      run("valid_block_len_max", call(e, ok, &huge));
      run("valid_largest_table", call(big_table, make_sim(SMMC_MODE_TABLE, 360, SMMC_MAX_BINS, 0), &b12));
    }
  }
  // which divide a launch uses: the rule of smmc_engine_divide_kind(e, sim, 0), whatever the block length
  const smmc_blocks b4 = make_blocks(4), b1 = make_blocks(1);
  const smmc_sim s360 = make_sim(SMMC_MODE_TABLE, 360, 0, 0);
  std::printf("kind:redo_table %d %d\n", smmc_engine_blocks_divide_kind(redo, &s360, &b4), smmc_engine_divide_kind(redo, &s360, 0));
  std::printf("kind:calm_table %d %d\n", smmc_engine_blocks_divide_kind(calm, &s360, &b4), smmc_engine_divide_kind(calm, &s360, 0));
  std::printf("kind:calm_table_L1 %d %d\n", smmc_engine_blocks_divide_kind(calm, &s360, &b1), smmc_engine_divide_kind(calm, &s360, 0));
  // bounds come from the extremes alone: the S&P 500's best and worst month (+42.2 %, -29.7 %) over 360 periods
  smmc_engine *sp = nullptr;
  const float sp_table[3] = {42.2f, -29.7f, 0.6f};
  if (smmc_engine_create(0, nullptr, &sp) != SMMC_OK || smmc_engine_set_table(sp, sp_table, 3) != SMMC_OK) return 1;
  const smmc_blocks b12k = make_blocks(12);
  std::printf("kind:best_and_worst_month %d %d\n", smmc_engine_blocks_divide_kind(sp, &s360, &b12k), smmc_engine_divide_kind(sp, &s360, 0));
  smmc_engine_destroy(sp);
  const smmc_sim exact = make_sim(SMMC_MODE_TABLE, 360, 0, SMMC_FLAG_EXACT_DIV);
  std::printf("kind:exact_flag %d %d\n", smmc_engine_blocks_divide_kind(calm, &exact, &b4), smmc_engine_divide_kind(calm, &exact, 0));
  std::printf("sizes %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_blocks));
  for (smmc_engine *p : {e, no_table, big_table, redo, calm}) smmc_engine_destroy(p);
  std::printf("blocks_args: done\n");
  return 0;
}
