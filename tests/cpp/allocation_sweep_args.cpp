// allocation_sweep_args.cpp -- the argument checks and the divide rule of smmc_engine_simulate_allocation_sweep, its
// _to_host form and smmc_engine_allocation_sweep_divide_kind (include/smmc.h) without a GPU:
// csrc/smmc_allocation_sweep.cpp and the library's other host units over tests/cpp/fake_hip.cpp,
// tests/cpp/launch_fake.cpp, the existing launch stubs and tests/cpp/allocation_sweep_launch_stub.cpp.  Every check runs
// before any device work, so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error() and
// without a launch; TEST INFRASTRUCTURE, driven by tests/test_allocation_sweep_cpu.py (built with
// -fsanitize=address,undefined and run directly).  Prints one line per case: "<name> <return code> <length of the error
// text> <launches the call made>" and the text behind "#", then "kind:<case> <SMMC_DIV_*>", "ran:<case> <return code>
// <1: the launch asked for the IEEE divide>", "padding:...", "lease:..." and "sizes ..." lines, then
// "allocation_sweep_args: done".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"
#include "smmc_internal.h"

extern "C" int fake_allocation_sweep_launches(void);
extern "C" int fake_allocation_sweep_last_exact(void);
extern "C" const void *fake_allocation_sweep_last_args(void);
extern "C" float fake_path_value(uint64_t id, uint32_t key0, uint32_t key1, uint32_t n_periods, float capital);

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

// two assets with the given first weight; Gaussian fields as asked: (means 0.5, 0.2; L = [[4, 0], [0.9, 1.2]]) or all zero
static smmc_portfolio make_pf(bool gaussian, uint32_t every, float w0) {
  smmc_portfolio p;
  std::memset(&p, 0, sizeof p);
  p.struct_size = sizeof p;
  p.n_assets = 2;
  p.rebalance_every = every;
  p.weights[0] = w0;
  p.weights[1] = 1.0f - w0;
  if (gaussian) {
    p.means[0] = 0.5f;
    p.means[1] = 0.2f;
    p.factor[0] = 4.0f;
    p.factor[SMMC_MAX_ASSETS] = 0.9f;
    p.factor[SMMC_MAX_ASSETS + 1] = 1.2f;
  }
  return p;
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

// n strategies: first weights 1, 0.875, 0.75, ... (exact in binary32), R = 12, 0, 1, 5, ..., amounts 2 .. 5.5, floor 0.01: every
// scenario FAST by the single call's rule at 36 periods
struct Scenarios {
  std::vector<smmc_portfolio> pf;
  std::vector<smmc_cashflow> cf;
};
static Scenarios strategies(bool gaussian, uint32_t n) {
  const uint32_t every[4] = {12, 0, 1, 5};
  Scenarios s;
  for (uint32_t i = 0; i < n; ++i) {
    s.pf.push_back(make_pf(gaussian, every[i % 4], 1.0f - 0.125f * static_cast<float>(i % 8)));
    s.cf.push_back(make_cf(2.0f + 0.5f * static_cast<float>(i % 8), 0.0f, 0.01f));
  }
  return s;
}

static void report(const char *name, int rc, int launches) {
  std::printf("%s %d %zu %d\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0), launches);
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr, *no_table = nullptr, *three = nullptr;
  for (smmc_engine **p : {&e, &no_table, &three})
    if (smmc_engine_create(0, nullptr, p) != SMMC_OK) {
      std::printf("engine_create failed: %s\n", smmc_last_error());
      return 1;
    }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float rows2[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};         // 3 rows x 2 assets
  if (smmc_engine_set_asset_table(e, rows2, 3, 2) != SMMC_OK) return 1;  // note: e has NO single-series table
  if (smmc_engine_set_asset_table(three, rows2, 2, 3) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[SMMC_MAX_SWEEP * (64 + 8 * 4096)];
  alignas(8) static uint64_t depleted[SMMC_MAX_SWEEP_COUNTERS + 16];
  static float finals[8000], holdings[16000], paid[8000];
  static uint32_t ruin[8000];
  std::vector<float> per_period(360, 1.0f);

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c, uint32_t n,
                    const smmc_allocation_sweep_outputs *o) {
      if (entry == 0) return smmc_engine_simulate_allocation_sweep(eng, s, p, c, n, o);
      if (entry == 1) return smmc_engine_simulate_allocation_sweep_to_host(eng, s, p, c, n, o);
      return smmc_engine_allocation_sweep_divide_kind(eng, s, p, c, n);
    };
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    smmc_allocation_sweep_outputs out;
    std::memset(&out, 0, sizeof out);
    out.struct_size = sizeof out;
    out.d_final = finals;
    out.d_holdings = holdings;
    out.d_paid = paid;
    out.d_ruin_period = ruin;
    out.d_stats = stats;
    out.d_depleted_at = depleted;
    char name[96];
    auto run = [&](const char *what, smmc_engine *eng, const smmc_sim *s, const Scenarios *sc, uint32_t n,
                   const smmc_allocation_sweep_outputs *o) {
      const int before = fake_allocation_sweep_launches();
      const int rc = call(eng, s, sc ? sc->pf.data() : nullptr, sc ? sc->cf.data() : nullptr, n, o);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_allocation_sweep_launches() - before);
    };
    const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 64, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 64, 0);
    const Scenarios t8 = strategies(false, 8), g8 = strategies(true, 8);
    Scenarios sc;
    smmc_sim s;
    // what the sweep itself refuses
    {
      const int before = fake_allocation_sweep_launches();
      std::snprintf(name, sizeof name, "%s:pfs_null", tag);
      report(name, call(e, &gau, nullptr, g8.cf.data(), 8, &out), fake_allocation_sweep_launches() - before);
      std::snprintf(name, sizeof name, "%s:cfs_null", tag);
      report(name, call(e, &gau, g8.pf.data(), nullptr, 8, &out), fake_allocation_sweep_launches() - before);
    }
    run("no_scenarios", e, &gau, &g8, 0, &out);
    sc = strategies(true, 9);
    run("nine_scenarios", e, &gau, &sc, 9, &out);
    sc = g8, sc.cf[5].amounts = per_period.data();
    run("scenario_with_amounts", e, &gau, &sc, 8, &out);
    sc = strategies(true, 3), sc.cf[2].fractions = per_period.data();
    run("scenario_with_fractions", e, &gau, &sc, 3, &out);
    sc = g8, sc.pf[6].n_assets = 1, sc.pf[6].weights[0] = 1.0f, sc.pf[6].weights[1] = 0.0f, sc.pf[6].factor[SMMC_MAX_ASSETS] = 0.0f,
    sc.pf[6].factor[SMMC_MAX_ASSETS + 1] = 0.0f, sc.pf[6].means[1] = 0.0f;
    run("law_n_assets_differs", e, &gau, &sc, 8, &out);
    sc = g8, sc.pf[3].means[1] = 0.25f;
    run("law_means_differ", e, &gau, &sc, 8, &out);
    sc = g8, sc.pf[7].factor[SMMC_MAX_ASSETS] = 0.8f;
    run("law_factor_differs", e, &gau, &sc, 8, &out);
    sc = g8, sc.pf[2].means[0] = -0.0f, sc.pf[0].means[0] = 0.0f, sc.pf[1].means[0] = 0.0f;  // bit for bit: -0 is not +0
    for (uint32_t i = 3; i < 8; ++i) sc.pf[i].means[0] = 0.0f;
    run("law_means_differ_in_sign_of_zero", e, &gau, &sc, 8, &out);
    // what the portfolio call refuses, in one scenario (the last: every one is looked at) or in the sim
    run("engine_null", nullptr, &gau, &g8, 8, &out);
    run("sim_null", e, nullptr, &g8, 8, &out);
    s = gau, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &g8, 8, &out);
    sc = g8, sc.pf[7].struct_size = sizeof(smmc_portfolio) + 4;
    run("portfolio_struct_size_wrong", e, &gau, &sc, 8, &out);
    sc = g8;
    for (auto &p : sc.pf) p.n_assets = 0;
    run("no_assets", e, &gau, &sc, 8, &out);
    sc = g8, sc.pf[7].reserved = 1;
    run("reserved_not_zero", e, &gau, &sc, 8, &out);
    sc = g8, sc.pf[7].weights[0] = -0.1f, sc.pf[7].weights[1] = 1.1f;
    run("weight_negative", e, &gau, &sc, 8, &out);
    sc = g8, sc.pf[4].weights[1] = nan;
    run("weight_nan", e, &gau, &sc, 8, &out);
    sc = g8, sc.pf[7].weights[1] = 0.1251f;
    run("weights_do_not_sum_to_one", e, &gau, &sc, 8, &out);
    run("table_mode_without_asset_table", no_table, &tab, &t8, 8, &out);
    run("asset_table_of_other_width", three, &tab, &t8, 8, &out);
    run("gaussian_fields_in_table_mode", e, &tab, &g8, 8, &out);
    sc = g8;
    for (auto &p : sc.pf) p.factor[1] = 0.5f;
    run("factor_above_diagonal", e, &gau, &sc, 8, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 64, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &t8, 8, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 64, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &g8, 8, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &g8, 1, &out);
    s = gau, s.hist_lo = 10.0f, s.hist_hi = 10.0f;
    run("histogram_range_empty", e, &s, &g8, 8, &out);
    s = gau, s.mode = 7;
    run("unknown_mode", e, &s, &g8, 8, &out);
    // what the cash-flow call refuses
    sc = g8, sc.cf[7].struct_size = sizeof(smmc_cashflow) + 8;
    run("cashflow_struct_size_wrong", e, &gau, &sc, 8, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 0, 64, 0);
    run("no_periods", e, &s, &g8, 8, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 0, 0);
    run("too_many_periods", e, &s, &g8, 1, &out);
    sc = g8, sc.cf[7].floor = -1.0f;
    run("floor_negative", e, &gau, &sc, 8, &out);
    sc = g8, sc.cf[7].floor = nan;
    run("floor_nan", e, &gau, &sc, 8, &out);
    sc = strategies(true, 5), sc.cf[4].amount = inf;
    run("amount_infinite", e, &gau, &sc, 5, &out);
    sc = strategies(true, 2), sc.cf[0].fraction = nan;
    run("fraction_nan", e, &gau, &sc, 2, &out);
    if (entry < 2) {
      run("outputs_null", e, &gau, &g8, 8, nullptr);
      smmc_allocation_sweep_outputs o = out;
      o.struct_size = sizeof o - 8;
      run("outputs_struct_size_wrong", e, &gau, &g8, 8, &o);
      o = out, o.reserved = 3;
      run("outputs_reserved_not_zero", e, &gau, &g8, 8, &o);
      // the counter cap: 8 x (1000 + 1 + 64) = 8520 > 8192; 7 x 1065 = 7455 passes; without the records the buckets do
      // not count: 8 x 1001 = 8008 passes
      const smmc_sim p1000 = make_sim(SMMC_MODE_GAUSSIAN, 1000, 64, 0);
      run("counter_cap_8_x_1000_64_bins", e, &p1000, &g8, 8, &out);
      run("valid_7_x_1000_64_bins", e, &p1000, &g8, 7, &out);
      o = out, o.d_stats = nullptr;
      run("valid_8_x_1000_no_stats", e, &p1000, &g8, 8, &o);
      s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, 0, 0);
      run("counter_cap_2_x_max_periods", e, &s, &t8, 2, &out);
      run("valid_1_x_max_periods", e, &s, &t8, 1, &out);
      s = gau, s.n_paths = 1ull << 50;
      run("paths_per_workgroup", e, &s, &g8, 8, &out);
      if (entry == 0) {
        o = out, o.d_holdings = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(holdings) + 2);
        run("holdings_misaligned", e, &gau, &g8, 8, &o);
        o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
        run("depleted_at_misaligned", e, &gau, &g8, 8, &o);
      }
      // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
      run("valid_8_gaussian", e, &gau, &g8, 8, &out);
      run("valid_8_table", e, &tab, &t8, 8, &out);
      run("valid_5", e, &gau, &g8, 5, &out);
      run("valid_4", e, &tab, &t8, 4, &out);
      run("valid_3", e, &gau, &g8, 3, &out);
      run("valid_1", e, &tab, &t8, 1, &out);
      smmc_allocation_sweep_outputs none;
      std::memset(&none, 0, sizeof none);
      none.struct_size = sizeof none;
      run("valid_no_outputs", e, &tab, &t8, 8, &none);
      s = gau, s.n_paths = 0;
      o = out, o.d_stats = nullptr, o.d_depleted_at = nullptr;  // the launch stubs have no kernel that folds or copies the counts
      run("valid_no_paths", e, &s, &g8, 8, &o);               // nothing to launch: SMMC_OK
    }
  }

  // which divide a sweep uses: SMMC_DIV_FAST = 0 iff every scenario's own rule says so, else SMMC_DIV_EXACT = 1
  auto kind = [&](const char *what, const smmc_sim &s, const Scenarios &sc) {
    std::printf("kind:%s %d\n", what, smmc_engine_allocation_sweep_divide_kind(e, &s, sc.pf.data(), sc.cf.data(), static_cast<uint32_t>(sc.pf.size())));
  };
  const smmc_sim t360 = make_sim(SMMC_MODE_TABLE, 360, 0, 0), g36 = make_sim(SMMC_MODE_GAUSSIAN, 36, 0, 0),
                 g360 = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
  Scenarios sc = strategies(false, 8);
  bool each_fast = true;
  for (uint32_t i = 0; i < 8; ++i)
    each_fast = each_fast && smmc_engine_portfolio_cashflow_divide_kind(e, &t360, &sc.pf[i], &sc.cf[i]) == SMMC_DIV_FAST;
  std::printf("kind:each_of_the_eight_alone %d\n", each_fast ? 0 : 1);
  kind("all_fast_table", t360, sc);
  kind("all_fast_gaussian_36", g36, strategies(true, 8));
  kind("gaussian_360", g360, strategies(true, 8));  // the single call's rule: 128.5 %, 360 times
  kind("exact_flag", make_sim(SMMC_MODE_TABLE, 360, 0, SMMC_FLAG_EXACT_DIV), sc);
  sc.cf[3] = make_cf(4.0f, 0.004f, 0.01f);  // a fraction: unproven
  kind("one_exact_among_eight", t360, sc);
  sc = strategies(false, 8), sc.cf[7] = make_cf(4.0f, 0.0f, 0.0f);  // rebalanced (R = 5) without a floor
  kind("last_exact", t360, sc);
  sc = strategies(false, 1);
  kind("single_fast", t360, sc);
  sc.cf[0] = make_cf(0.0f, 0.004f, 0.01f);
  kind("single_exact", t360, sc);

  // the form a launch is given is the form the rule names
  {
    smmc_allocation_sweep_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_final = finals;
    sc = strategies(false, 8);
    int rc = smmc_engine_simulate_allocation_sweep(e, &t360, sc.pf.data(), sc.cf.data(), 8, &o);
    std::printf("ran:fast %d %d\n", rc, fake_allocation_sweep_last_exact());
    sc.cf[3] = make_cf(4.0f, 0.004f, 0.01f);
    rc = smmc_engine_simulate_allocation_sweep(e, &t360, sc.pf.data(), sc.cf.data(), 8, &o);
    std::printf("ran:exact %d %d\n", rc, fake_allocation_sweep_last_exact());
    // padding: a request of S scenarios reaches the launch with x.n = S and entries S .. 7 copies of entry S - 1
    for (uint32_t S : {1u, 3u, 4u, 5u, 8u}) {
      sc = strategies(false, S);
      rc = smmc_engine_simulate_allocation_sweep(e, &t360, sc.pf.data(), sc.cf.data(), S, &o);
      const smmc::AllocationSweepArgs &x = *static_cast<const smmc::AllocationSweepArgs *>(fake_allocation_sweep_last_args());
      bool real = x.n == S && x.p.n_assets == 2, copies = true;
      for (uint32_t i = 0; i < SMMC_MAX_SWEEP; ++i) {
        const uint32_t from = i < S ? i : S - 1;
        const bool same = std::memcmp(x.weights[i], sc.pf[from].weights, sizeof x.weights[i]) == 0 &&
                          x.rebalance_every[i] == sc.pf[from].rebalance_every && x.amount[i] == sc.cf[from].amount &&
                          x.fraction[i] == sc.cf[from].fraction && x.floor[i] == sc.cf[from].floor;
        (i < S ? real : copies) = (i < S ? real : copies) && same;
      }
      std::printf("padding:%u %d %d %d %u\n", S, rc, real ? 1 : 0, copies ? 1 : 0, smmc::allocation_sweep_width(S));
    }
  }

  // the accumulator lease: a call whose launch fails has taken the engine's accumulator (buckets and depletion counters of
  // every scenario) and not given it back clean; the next user (a plain simulate through tests/cpp/launch_fake.cpp) must
  // still get its own buckets
  {
    smmc_engine *l = nullptr;
    const float table[3] = {1.0f, -2.0f, 0.5f};
    if (smmc_engine_create(0, nullptr, &l) != SMMC_OK || smmc_engine_set_table(l, table, 3) != SMMC_OK) return 1;
    smmc_sim s = make_sim(SMMC_MODE_TABLE, 36, 16, 0);
    s.n_paths = 5000;
    s.hist_lo = 400.0f;
    s.hist_hi = 2100.0f;
    std::vector<float> out(s.n_paths);
    std::vector<uint64_t> hist(16), again(16), want(16, 0);
    smmc_stats st;
    for (uint64_t i = 0; i < s.n_paths; ++i) {
      const float v = fake_path_value(i, 7, 0, 36, 1000.0f);
      if (v >= s.hist_lo && v < s.hist_hi) want[std::min<int>(15, static_cast<int>((static_cast<double>(v) - 400.0) * (16.0 / 1700.0)))] += 1;
    }
    const int first = smmc_engine_simulate_to_host(l, &s, out.data(), nullptr, nullptr, nullptr, &st, hist.data());
    smmc_allocation_sweep_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_stats = stats;
    o.d_depleted_at = depleted;
    const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 36, 16, 0);
    const Scenarios g8 = strategies(true, 8);
    const int failed = smmc_engine_simulate_allocation_sweep(l, &g, g8.pf.data(), g8.cf.data(), 8, &o);
    const int second = smmc_engine_simulate_to_host(l, &s, out.data(), nullptr, nullptr, nullptr, &st, again.data());
    std::printf("lease:after_failed_launch %d %d %d %d %d\n", first, failed, second, hist == want ? 1 : 0, again == want ? 1 : 0);
    smmc_engine_destroy(l);
  }

  std::printf("sizes %zu %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_cashflow), sizeof(smmc_allocation_sweep_outputs));
  std::printf("constants %d %d %d\n", SMMC_MAX_SWEEP, SMMC_MAX_SWEEP_COUNTERS, SMMC_ABI_VERSION);
  for (smmc_engine *p : {e, no_table, three}) smmc_engine_destroy(p);
  std::printf("allocation_sweep_args: done\n");
  return 0;
}
