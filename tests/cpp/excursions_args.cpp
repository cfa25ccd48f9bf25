// excursions_args.cpp -- the argument checks of smmc_engine_simulate_excursions and its _to_host form
// (include/smmc.h) without a GPU: csrc/smmc_excursions.cpp, csrc/smmc_cashflow.cpp and csrc/smmc_capi.cpp over
// tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the two launch stubs.  Every check runs before any device
// work, so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error(); TEST
// INFRASTRUCTURE, driven by tests/test_excursions_cpu.py.  Prints one line per case: "<name> <return code> <length
// of the error text>", then "sizes ...", then "excursions_args: done".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

static smmc_excursions make_x(float lower, float target, float threshold) {
  smmc_excursions x;
  std::memset(&x, 0, sizeof x);
  x.struct_size = sizeof x;
  x.lower = lower;
  x.target = target;
  x.drawdown_threshold = threshold;
  return x;
}

static void report(const char *name, int rc) {
  std::printf("%s %d %zu\n", name, rc, rc ? std::strlen(smmc_last_error()) : static_cast<size_t>(0));
  if (rc) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr;
  if (smmc_engine_create(0, nullptr, &e) != SMMC_OK) {
    std::printf("engine_create failed: %s\n", smmc_last_error());
    return 1;
  }
  smmc_engine *no_table = nullptr, *big_table = nullptr;
  if (smmc_engine_create(0, nullptr, &no_table) != SMMC_OK) return 1;
  if (smmc_engine_create(0, nullptr, &big_table) != SMMC_OK) return 1;
  const float table[3] = {1.0f, -2.0f, 0.5f};
  if (smmc_engine_set_table(e, table, 3) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);
  if (smmc_engine_set_table(big_table, largest.data(), SMMC_MAX_TABLE) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096], dd_stats[64 + 8 * 4096];
  static uint64_t below_at[SMMC_MAX_EXCURSION_PERIODS + 2], reach_at[SMMC_MAX_EXCURSION_PERIODS + 2];
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  smmc_excursion_outputs out;
  std::memset(&out, 0, sizeof out);
  out.struct_size = sizeof out;
  out.stats = stats;
  out.drawdown_stats = dd_stats;
  out.first_below_at = below_at;
  out.first_reach_at = reach_at;

  for (int to_host = 0; to_host < 2; ++to_host) {
    auto call = [&](smmc_engine *eng, const smmc_sim &s, const smmc_excursions *x, const smmc_excursion_outputs *o) {
      return to_host ? smmc_engine_simulate_excursions_to_host(eng, &s, x, o) : smmc_engine_simulate_excursions(eng, &s, x, o);
    };
    const char *tag = to_host ? "to_host" : "device";
    char name[96];
    auto run = [&](const char *what, int rc) {
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc);
    };
    const smmc_sim ok = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_excursions x = make_x(800.0f, 2000.0f, 0.2f);
    run("x_null", call(e, ok, nullptr, &out));
    run("out_null", call(e, ok, &x, nullptr));
    smmc_excursions bad = x;
    bad.struct_size = sizeof bad - 4;
    run("x_struct_size_wrong", call(e, ok, &bad, &out));
    smmc_excursion_outputs bad_out = out;
    bad_out.struct_size = sizeof bad_out - 8;
    run("out_struct_size_wrong", call(e, ok, &x, &bad_out));
    run("n_periods_zero", call(e, make_sim(SMMC_MODE_GAUSSIAN, 0, 100, 0), &x, &out));
    run("n_periods_above_max", call(e, make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_EXCURSION_PERIODS + 1, 100, 0), &x, &out));
    bad = make_x(nan, 2000.0f, 0.2f);
    run("lower_nan", call(e, ok, &bad, &out));
    bad = make_x(800.0f, nan, 0.2f);
    run("target_nan", call(e, ok, &bad, &out));
    bad = make_x(800.0f, 2000.0f, nan);
    run("drawdown_threshold_nan", call(e, ok, &bad, &out));
    run("stream_ref", call(e, make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF), &x, &out));
    run("stream_v2", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2), &x, &out));
    run("table_mode_without_table", call(no_table, make_sim(SMMC_MODE_TABLE, 360, 100, 0), &x, &out));
    run("n_bins_above_max", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0), &x, &out));
    smmc_sim s = ok;
    s.hist_lo = 10.0f;
    s.hist_hi = 10.0f;
    run("histogram_range_empty", call(e, s, &x, &out));
    run("engine_null", call(nullptr, ok, &x, &out));
    // the largest table, the most periods and the most buckets together: 64 + 32 + 32 KiB of LDS
    run("lds_above_the_limit", call(big_table, make_sim(SMMC_MODE_TABLE, SMMC_MAX_EXCURSION_PERIODS, SMMC_MAX_BINS, 0), &x, &out));
    s = ok;
    s.n_paths = 1ull << 60;
    smmc_excursion_outputs records_only = out;  // no per-path output: nothing of that size is ever allocated
    run("paths_per_workgroup_2_pow_32", call(e, s, &x, &records_only));
    // a valid request passes every argument check; what stops it here is that this build has no kernel
    run("valid", call(e, ok, &x, &out));
    bad = make_x(-inf, inf, inf);  // infinite levels are allowed: never below, never reached
    run("valid_infinite_levels", call(e, ok, &bad, &out));
    run("valid_max_periods", call(e, make_sim(SMMC_MODE_TABLE, SMMC_MAX_EXCURSION_PERIODS, 0, 0), &x, &out));
  }
  std::printf("sizes %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_excursions), sizeof(smmc_excursion_outputs));
  smmc_engine_destroy(big_table);
  smmc_engine_destroy(no_table);
  smmc_engine_destroy(e);
  std::printf("excursions_args: done\n");
  return 0;
}
