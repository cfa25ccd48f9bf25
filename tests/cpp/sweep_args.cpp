// sweep_args.cpp -- the argument checks and the divide rule of smmc_engine_simulate_cashflow_sweep, its _to_host form
// and smmc_engine_cashflow_sweep_divide_kind (include/smmc.h) without a GPU: csrc/smmc_sweep.cpp, csrc/smmc_cashflow.cpp
// and csrc/smmc_capi.cpp over tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp, tests/cpp/cashflow_launch_stub.cpp and
// tests/cpp/sweep_launch_stub.cpp.  Every check runs before any device work, so each bad request must come back as
// SMMC_ERR_INVALID with a text in smmc_last_error() and without a launch; TEST INFRASTRUCTURE, driven by
// tests/test_sweep_cpu.py.  Prints one line per case: "<name> <return code> <length of the error text> <launches>" and
// under it "#   <text>", then the divide rule's answers as "kind:<name> <kind>", then "sweep_args: done".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"

extern "C" int sweep_stub_launches();

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

static smmc_cashflow make_cf(float amount, float fraction, float floor) {
  smmc_cashflow c;
  std::memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.amount = amount;
  c.fraction = fraction;
  c.floor = floor;
  return c;
}

// amounts 0, 2, 3, 4, 5, 6, 8, 12 with floor 0.01: every scenario FAST by the single call's rule
static std::vector<smmc_cashflow> amounts_sweep(uint32_t n) {
  const float am[8] = {0.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f, 8.0f, 12.0f};
  std::vector<smmc_cashflow> v;
  for (uint32_t s = 0; s < n; ++s) v.push_back(make_cf(am[s % 8], 0.0f, 0.01f));
  return v;
}

static void report(const char *name, int rc, int launches) {
  std::printf("%s %d %zu %d\n", name, rc, rc ? std::strlen(smmc_last_error()) : static_cast<size_t>(0), launches);
  if (rc) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr;
  if (smmc_engine_create(0, nullptr, &e) != SMMC_OK) {
    std::printf("engine_create failed: %s\n", smmc_last_error());
    return 1;
  }
  smmc_engine *no_table = nullptr;
  if (smmc_engine_create(0, nullptr, &no_table) != SMMC_OK) return 1;
  const float table[3] = {1.0f, -2.0f, 0.5f};
  if (smmc_engine_set_table(e, table, 3) != SMMC_OK) return 1;
  static uint64_t stats[SMMC_MAX_SWEEP * (8 + 4096)];
  static uint64_t depleted[SMMC_MAX_SWEEP_COUNTERS + 16];
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> per_period(360, 1.0f);

  for (int entry = 0; entry < 3; ++entry) {
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    auto call = [&](smmc_engine *eng, const smmc_sim &s, const smmc_cashflow *c, uint32_t n, bool want_stats = true) {
      void *st = want_stats ? stats : nullptr;
      if (entry == 0) return smmc_engine_simulate_cashflow_sweep(eng, &s, c, n, nullptr, nullptr, nullptr, st, depleted);
      if (entry == 1) return smmc_engine_simulate_cashflow_sweep_to_host(eng, &s, c, n, nullptr, nullptr, nullptr, st, depleted);
      return smmc_engine_cashflow_sweep_divide_kind(eng, &s, c, n);
    };
    char name[96];
    auto run = [&](const char *what, int rc, int before) {
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, sweep_stub_launches() - before);
    };
#define RUN(what, expr)                       \
  do {                                        \
    const int before = sweep_stub_launches(); \
    run(what, (expr), before);                \
  } while (0)
    const smmc_sim ok = make_sim(SMMC_MODE_GAUSSIAN, 360, 64, 0);
    std::vector<smmc_cashflow> sc = amounts_sweep(8);
    // what the sweep itself refuses
    RUN("scenarios_null", call(e, ok, nullptr, 8));
    RUN("no_scenarios", call(e, ok, sc.data(), 0));
    RUN("nine_scenarios", call(e, ok, amounts_sweep(9).data(), 9));
    sc = amounts_sweep(8);
    sc[5].amounts = per_period.data();
    RUN("scenario_with_amounts", call(e, ok, sc.data(), 8));
    sc = amounts_sweep(3);
    sc[2].fractions = per_period.data();
    RUN("scenario_with_fractions", call(e, ok, sc.data(), 3));
    // what smmc_engine_simulate_cashflow refuses, in one scenario (the last: every one is looked at) or in the sim
    sc = amounts_sweep(8);
    sc[7].struct_size = sizeof(smmc_cashflow) - 4;
    RUN("struct_size_wrong", call(e, ok, sc.data(), 8));
    sc = amounts_sweep(8);
    sc[7].floor = -0.5f;
    RUN("floor_negative", call(e, ok, sc.data(), 8));
    sc[7].floor = inf;
    RUN("floor_infinite", call(e, ok, sc.data(), 8));
    sc[7].floor = nan;
    RUN("floor_nan", call(e, ok, sc.data(), 8));
    sc = amounts_sweep(5);
    sc[4].amount = nan;
    RUN("amount_nan", call(e, ok, sc.data(), 5));
    sc = amounts_sweep(2);
    sc[0].fraction = -inf;
    RUN("fraction_infinite", call(e, ok, sc.data(), 2));
    sc = amounts_sweep(8);
    RUN("n_periods_zero", call(e, make_sim(SMMC_MODE_GAUSSIAN, 0, 64, 0), sc.data(), 8));
    RUN("n_periods_above_max", call(e, make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 0, 0), sc.data(), 1));
    RUN("stream_ref", call(e, make_sim(SMMC_MODE_TABLE, 360, 64, SMMC_FLAG_STREAM_REF), sc.data(), 8));
    RUN("stream_v2", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, 64, SMMC_FLAG_STREAM_V2), sc.data(), 8));
    RUN("table_mode_without_table", call(no_table, make_sim(SMMC_MODE_TABLE, 360, 64, 0), sc.data(), 8));
    RUN("n_bins_above_max", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0), sc.data(), 1));
    smmc_sim s = ok;
    s.hist_lo = 10.0f;
    s.hist_hi = 10.0f;
    RUN("histogram_range_empty", call(e, s, sc.data(), 8));
    RUN("engine_null", call(nullptr, ok, sc.data(), 8));
    s = ok;
    s.struct_size = sizeof s - 8;
    RUN("sim_struct_size_wrong", call(e, s, sc.data(), 8));
    if (entry < 2) {
      // the counter cap: 8 x (1000 + 1 + 64) = 8520 > 8192; 7 x 1065 = 7455 passes; without statistics the buckets do
      // not count: 8 x 1001 = 8008 passes
      const smmc_sim p1000 = make_sim(SMMC_MODE_GAUSSIAN, 1000, 64, 0);
      RUN("counter_cap_8_x_1000_64_bins", call(e, p1000, sc.data(), 8));
      RUN("valid_7_x_1000_64_bins", call(e, p1000, sc.data(), 7));
      RUN("valid_8_x_1000_no_stats", call(e, p1000, sc.data(), 8, false));
      RUN("counter_cap_2_x_max_periods", call(e, make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, 0, 0), sc.data(), 2));
      RUN("valid_1_x_max_periods", call(e, make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, 0, 0), sc.data(), 1));
      s = ok;
      s.n_paths = 1ull << 46;  // 4 fake CUs: at most 32 workgroups
      RUN("paths_per_workgroup", call(e, s, sc.data(), 8));
      // valid requests pass every check; what stops them here is that this build has no kernel
      RUN("valid_8", call(e, ok, sc.data(), 8));
      RUN("valid_3", call(e, ok, sc.data(), 3));
      RUN("valid_1", call(e, ok, sc.data(), 1));
      RUN("valid_5_table", call(e, make_sim(SMMC_MODE_TABLE, 1000, 64, 0), sc.data(), 5));
      if (entry == 0) {
        RUN("final_misaligned", smmc_engine_simulate_cashflow_sweep(e, &ok, sc.data(), 8, reinterpret_cast<float *>(2), nullptr, nullptr,
                                                                    nullptr, nullptr));
        RUN("depleted_at_misaligned", smmc_engine_simulate_cashflow_sweep(e, &ok, sc.data(), 8, nullptr, nullptr, nullptr, nullptr,
                                                                          reinterpret_cast<uint64_t *>(4)));
      }
    }
#undef RUN
  }

  // the divide rule (include/smmc.h): SMMC_DIV_FAST = 0, SMMC_DIV_EXACT = 1
  auto kind = [&](const char *what, const smmc_sim &s, const std::vector<smmc_cashflow> &c) {
    std::printf("kind:%s %d\n", what, smmc_engine_cashflow_sweep_divide_kind(e, &s, c.data(), static_cast<uint32_t>(c.size())));
  };
  const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
  std::vector<smmc_cashflow> sc = amounts_sweep(8);
  kind("all_fast", g, sc);
  kind("all_fast_table", make_sim(SMMC_MODE_TABLE, 360, 0, 0), sc);
  kind("exact_flag", make_sim(SMMC_MODE_GAUSSIAN, 360, 0, SMMC_FLAG_EXACT_DIV), sc);
  sc[3] = make_cf(4.0f, 0.0f, 0.0f);  // an amount with floor 0: a live value can come arbitrarily close to 0
  kind("one_exact_among_eight", g, sc);
  sc = amounts_sweep(8);
  sc[7] = make_cf(0.0f, 1.5f, 0.01f);
  kind("last_exact", g, sc);
  sc = amounts_sweep(1);
  kind("single_fast", g, sc);
  sc[0] = make_cf(6.0f, 0.0f, 0.0f);
  kind("single_exact", g, sc);
  sc = {make_cf(0.0f, 0.004f, 0.0f), make_cf(-100.0f, 0.0f, 0.0f), make_cf(3.0f, 0.002f, 0.01f)};
  kind("mixed_all_fast", g, sc);
  std::printf("sizes %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_cashflow));
  std::printf("constants %d %d %d\n", SMMC_MAX_SWEEP, SMMC_MAX_SWEEP_COUNTERS, SMMC_ABI_VERSION);
  smmc_engine_destroy(no_table);
  smmc_engine_destroy(e);
  std::printf("sweep_args: done\n");
  return 0;
}
