// cashflow_args.cpp -- the argument checks of smmc_engine_simulate_cashflow and its _to_host form
// (include/smmc.h) without a GPU: csrc/smmc_cashflow.cpp and csrc/smmc_capi.cpp over tests/cpp/fake_hip.cpp,
// tests/cpp/launch_fake.cpp and tests/cpp/cashflow_launch_stub.cpp.  Every check runs before any device work, so
// each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error(); TEST INFRASTRUCTURE,
// driven by tests/test_cashflow_cpu.py.  Prints one line per case: "<name> <return code> <length of the error
// text>", then the divide rule's answers as "divide:<name> <kind> 0", then "cashflow_args: done".
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

static smmc_cashflow make_cf(float amount, float fraction, float floor) {
  smmc_cashflow c;
  std::memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.amount = amount;
  c.fraction = fraction;
  c.floor = floor;
  return c;
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
  smmc_engine *no_table = nullptr;
  if (smmc_engine_create(0, nullptr, &no_table) != SMMC_OK) return 1;
  const float table[3] = {1.0f, -2.0f, 0.5f};
  if (smmc_engine_set_table(e, table, 3) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> good(360, 1.0f), bad_amounts(360, 1.0f), bad_fractions(360, 0.001f);
  bad_amounts[359] = inf;
  bad_fractions[17] = nan;

  for (int to_host = 0; to_host < 2; ++to_host) {
    auto call = [&](smmc_engine *eng, const smmc_sim &s, const smmc_cashflow *c) {
      return to_host ? smmc_engine_simulate_cashflow_to_host(eng, &s, c, nullptr, nullptr, nullptr, stats, depleted)
                     : smmc_engine_simulate_cashflow(eng, &s, c, nullptr, nullptr, nullptr, stats, depleted);
    };
    const char *tag = to_host ? "to_host" : "device";
    char name[96];
    auto run = [&](const char *what, int rc) {
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc);
    };
    const smmc_sim ok = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_cashflow cf = make_cf(6.0f, 0.0f, 0.01f);
    run("cf_null", call(e, ok, nullptr));
    smmc_cashflow c = cf;
    c.struct_size = sizeof c - 4;
    run("struct_size_wrong", call(e, ok, &c));
    run("n_periods_zero", call(e, make_sim(SMMC_MODE_GAUSSIAN, 0, 100, 0), &cf));
    run("n_periods_above_max", call(e, make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0), &cf));
    c = make_cf(6.0f, 0.0f, -0.5f);
    run("floor_negative", call(e, ok, &c));
    c = make_cf(6.0f, 0.0f, inf);
    run("floor_infinite", call(e, ok, &c));
    c = make_cf(6.0f, 0.0f, nan);
    run("floor_nan", call(e, ok, &c));
    c = make_cf(nan, 0.0f, 0.01f);
    run("amount_nan", call(e, ok, &c));
    c = make_cf(6.0f, -inf, 0.01f);
    run("fraction_infinite", call(e, ok, &c));
    c = cf;
    c.amounts = bad_amounts.data();
    run("amounts_entry_infinite", call(e, ok, &c));
    c = cf;
    c.fractions = bad_fractions.data();
    run("fractions_entry_nan", call(e, ok, &c));
    run("stream_ref", call(e, make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF), &cf));
    run("stream_v2", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2), &cf));
    run("table_mode_without_table", call(no_table, make_sim(SMMC_MODE_TABLE, 360, 100, 0), &cf));
    run("n_bins_above_max", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0), &cf));
    smmc_sim s = ok;
    s.hist_lo = 10.0f;
    s.hist_hi = 10.0f;
    run("histogram_range_empty", call(e, s, &cf));
    run("engine_null", call(nullptr, ok, &cf));
    // a valid request passes every argument check; what stops it here is that this build has no kernel
    c = cf;
    c.amounts = good.data();
    run("valid_constant", call(e, ok, &cf));
    run("valid_arrays", call(e, ok, &c));
    run("valid_max_periods", call(e, make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, 0, 0), &cf));
  }

  // the divide rule (include/smmc.h): SMMC_DIV_FAST = 0, SMMC_DIV_EXACT = 1
  auto divide = [&](const char *what, const smmc_sim &s, const smmc_cashflow &c) {
    std::printf("divide:%s %d 0\n", what, smmc_engine_cashflow_divide_kind(e, &s, &c));
  };
  const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
  divide("zero_flow", g, make_cf(0.0f, 0.0f, 0.0f));                    // the no-cash-flow proof, as a special case
  divide("fraction_only_floor_0", g, make_cf(0.0f, 0.004f, 0.0f));      // shrinks geometrically: still bounded below
  divide("amount_floor_0", g, make_cf(6.0f, 0.0f, 0.0f));               // a live value can come arbitrarily close to 0
  divide("amount_floor_cent", g, make_cf(6.0f, 0.0f, 0.01f));           // ... not with a floor
  divide("collapse_floor_cent", g, make_cf(0.0f, 0.5f, 0.01f));
  divide("fraction_half_floor_0", g, make_cf(0.0f, 0.5f, 0.0f));        // 2^-360 by the bound
  divide("fraction_negative", g, make_cf(0.0f, -0.01f, 0.01f));
  divide("fraction_above_one", g, make_cf(0.0f, 1.5f, 0.01f));
  divide("contribution", g, make_cf(-100.0f, 0.0f, 0.0f));
  divide("contribution_huge", g, make_cf(-1e36f, 0.0f, 0.0f));          // the upper bound counts what is paid in
  divide("tiny_floor", g, make_cf(6.0f, 0.0f, 1e-30f));
  divide("exact_flag", make_sim(SMMC_MODE_GAUSSIAN, 360, 0, SMMC_FLAG_EXACT_DIV), make_cf(6.0f, 0.0f, 0.01f));
  divide("table", make_sim(SMMC_MODE_TABLE, 360, 0, 0), make_cf(6.0f, 0.0f, 0.01f));
  std::printf("sizes %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_cashflow));
  smmc_engine_destroy(no_table);
  smmc_engine_destroy(e);
  std::printf("cashflow_args: done\n");
  return 0;
}
