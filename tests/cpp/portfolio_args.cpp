// portfolio_args.cpp -- the argument checks of smmc_engine_set_asset_table, smmc_engine_simulate_portfolio, its _to_host
// form and smmc_engine_portfolio_divide_kind (include/smmc.h) without a GPU: csrc/smmc_portfolio.cpp and the library's
// other host units over tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before
// any device work, so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error() and without
// a launch; TEST INFRASTRUCTURE, driven by tests/test_portfolio_cpu.py.  Prints one line per case: "<name> <return code>
// <length of the error text> <launches the call made>" and the text behind "#", then "kind:<case> <SMMC_DIV_*>",
// "lease:...", "slots:..." and "sizes ..." lines, then "portfolio_args: done".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"

extern "C" int fake_portfolio_launches(void);
extern "C" size_t fake_hip_live_allocations(void);
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

// 60 / 40, Gaussian fields as asked: (means 0.5, 0.2; L = [[4, 0], [0.9, 1.2]]) or all zero for table mode
static smmc_portfolio make_pf(bool gaussian, uint32_t every) {
  smmc_portfolio p;
  std::memset(&p, 0, sizeof p);
  p.struct_size = sizeof p;
  p.n_assets = 2;
  p.rebalance_every = every;
  p.weights[0] = 0.6f;
  p.weights[1] = 0.4f;
  if (gaussian) {
    p.means[0] = 0.5f;
    p.means[1] = 0.2f;
    p.factor[0] = 4.0f;
    p.factor[SMMC_MAX_ASSETS] = 0.9f;
    p.factor[SMMC_MAX_ASSETS + 1] = 1.2f;
  }
  return p;
}

static void report(const char *name, int rc, int launches) {
  std::printf("%s %d %zu %d\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0), launches);
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr, *no_table = nullptr, *three = nullptr, *big = nullptr;
  for (smmc_engine **p : {&e, &no_table, &three, &big})
    if (smmc_engine_create(0, nullptr, p) != SMMC_OK) {
      std::printf("engine_create failed: %s\n", smmc_last_error());
      return 1;
    }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float rows2[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};            // 3 rows x 2 assets
  const float rows3[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};            // 2 rows x 3 assets
  if (smmc_engine_set_asset_table(e, rows2, 3, 2) != SMMC_OK) return 1;     // note: e has NO single-series table
  if (smmc_engine_set_asset_table(three, rows3, 2, 3) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);                   // 4096 rows x 4 assets: 64 KiB of LDS
  if (smmc_engine_set_asset_table(big, largest.data(), SMMC_MAX_TABLE / 4, 4) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  static float finals[1000], holdings[4000];

  // smmc_engine_set_asset_table's own refusals
  report("set:engine_null", smmc_engine_set_asset_table(nullptr, rows2, 3, 2), 0);
  report("set:table_null", smmc_engine_set_asset_table(e, nullptr, 3, 2), 0);
  report("set:no_rows", smmc_engine_set_asset_table(e, rows2, 0, 2), 0);
  report("set:no_assets", smmc_engine_set_asset_table(e, rows2, 3, 0), 0);
  report("set:five_assets", smmc_engine_set_asset_table(e, rows2, 1, 5), 0);
  report("set:too_large", smmc_engine_set_asset_table(e, largest.data(), SMMC_MAX_TABLE / 4 + 1, 4), 0);

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_portfolio_outputs *o) {
      if (entry == 0) return smmc_engine_simulate_portfolio(eng, s, p, o);
      if (entry == 1) return smmc_engine_simulate_portfolio_to_host(eng, s, p, o);
      return smmc_engine_portfolio_divide_kind(eng, s, p);
    };
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    smmc_portfolio_outputs out;
    std::memset(&out, 0, sizeof out);
    out.struct_size = sizeof out;
    out.d_final = finals;
    out.d_holdings = holdings;
    out.d_stats = stats;
    char name[96];
    auto run = [&](const char *what, smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_portfolio_outputs *o) {
      const int before = fake_portfolio_launches();
      const int rc = call(eng, s, p, o);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_portfolio_launches() - before);
    };
    const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 100, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
    smmc_portfolio p;
    smmc_sim s;
    run("engine_null", nullptr, &gau, &pg, &out);
    run("sim_null", e, nullptr, &pg, &out);
    s = gau, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &pg, &out);
    run("portfolio_null", e, &gau, nullptr, &out);
    p = pg, p.struct_size = sizeof p + 4;
    run("portfolio_struct_size_wrong", e, &gau, &p, &out);
    p = pg, p.n_assets = 0;
    run("no_assets", e, &gau, &p, &out);
    p = pg, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &gau, &p, &out);
    p = pg, p.reserved = 1;
    run("reserved_not_zero", e, &gau, &p, &out);
    p = pg, p.weights[0] = -0.1f, p.weights[1] = 1.1f;
    run("weight_negative", e, &gau, &p, &out);
    p = pg, p.weights[0] = nan;
    run("weight_nan", e, &gau, &p, &out);
    p = pg, p.weights[1] = inf;
    run("weight_infinite", e, &gau, &p, &out);
    p = pg, p.weights[0] = 0.5f, p.weights[1] = 0.3f, p.weights[2] = 0.2f;
    run("weight_beyond_assets", e, &gau, &p, &out);
    p = pg, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &gau, &p, &out);
    run("table_mode_without_asset_table", no_table, &tab, &pt, &out);
    run("asset_table_of_other_width", three, &tab, &pt, &out);
    run("gaussian_fields_in_table_mode", e, &tab, &pg, &out);
    p = pg, p.means[1] = nan;
    run("mean_nan", e, &gau, &p, &out);
    p = pg, p.factor[SMMC_MAX_ASSETS] = inf;
    run("factor_infinite", e, &gau, &p, &out);
    p = pg, p.factor[1] = 0.5f;
    run("factor_above_diagonal", e, &gau, &p, &out);
    p = pg, p.factor[2 * SMMC_MAX_ASSETS + 2] = 1.0f;
    run("factor_beyond_assets", e, &gau, &p, &out);
    p = pg, p.means[3] = 0.1f;
    run("mean_beyond_assets", e, &gau, &p, &out);
    p = pg, p.factor[SMMC_MAX_ASSETS + 1] = -1.2f;
    run("diagonal_negative", e, &gau, &p, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pt, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pg, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &pg, &out);
    s = gau, s.hist_lo = 10.0f, s.hist_hi = 10.0f;
    run("histogram_range_empty", e, &s, &pg, &out);
    s = gau, s.mode = 7;
    run("unknown_mode", e, &s, &pg, &out);
    if (entry < 2) {
      run("outputs_null", e, &gau, &pg, nullptr);
      smmc_portfolio_outputs o = out;
      o.struct_size = sizeof o - 8;
      run("outputs_struct_size_wrong", e, &gau, &pg, &o);
      o = out, o.reserved = 3;
      run("outputs_reserved_not_zero", e, &gau, &pg, &o);
      // the largest request there is -- 4096 rows x 4 words and 4096 buckets, 80 KiB -- fits the 128 KiB an engine
      // assumes at the least, so the LDS refusal cannot be reached with valid arguments
      p = pt, p.n_assets = 4, p.weights[0] = p.weights[1] = p.weights[2] = p.weights[3] = 0.25f;
      s = make_sim(SMMC_MODE_TABLE, 360, SMMC_MAX_BINS, 0);
      run("valid_largest_table", big, &s, &p, &out);
      s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0), s.n_paths = 1ull << 50;
      run("paths_per_workgroup", e, &s, &pg, &out);
      // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
      run("valid_table", e, &tab, &pt, &out);
      run("valid_gaussian", e, &gau, &pg, &out);
      p = pt, p.rebalance_every = 0;
      run("valid_buy_and_hold", e, &tab, &p, &out);
      s = gau, s.n_paths = 0;
      run("valid_no_paths", e, &s, &pg, &out);  // nothing to launch: SMMC_OK and an empty record
    }
  }

  // which divide a launch uses: SMMC_DIV_FAST = 0, SMMC_DIV_EXACT = 1, never SMMC_DIV_CHECKED
  auto kind = [&](const char *what, smmc_engine *eng, const smmc_sim &s, const smmc_portfolio &p) {
    std::printf("kind:%s %d\n", what, smmc_engine_portfolio_divide_kind(eng, &s, &p));
  };
  const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
  kind("table_calm", e, make_sim(SMMC_MODE_TABLE, 360, 0, 0), pt);
  kind("gaussian_calm_36", e, make_sim(SMMC_MODE_GAUSSIAN, 36, 0, 0), pg);
  kind("gaussian_calm_360", e, make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0), pg);  // 100.5 - 7 * 4 = 72.5 %, 360 times: 2^-167
  kind("exact_flag", e, make_sim(SMMC_MODE_GAUSSIAN, 360, 0, SMMC_FLAG_EXACT_DIV), pg);
  smmc_engine *dbl = nullptr;
  const float doubling[4] = {100.0f, 0.2f, -2.0f, 0.4f};  // one +100 % month in column 0
  if (smmc_engine_create(0, nullptr, &dbl) != SMMC_OK || smmc_engine_set_asset_table(dbl, doubling, 2, 2) != SMMC_OK) return 1;
  kind("table_doubling_360", dbl, make_sim(SMMC_MODE_TABLE, 360, 0, 0), pt);
  kind("table_doubling_36", dbl, make_sim(SMMC_MODE_TABLE, 36, 0, 0), pt);
  smmc_engine_destroy(dbl);
  smmc_portfolio wide = pg;
  wide.factor[0] = 20.0f;  // 100.5 - 7 * 20 < 0: a multiplier may change sign
  kind("gaussian_may_go_negative", e, make_sim(SMMC_MODE_GAUSSIAN, 2, 0, 0), wide);
  smmc_portfolio tiny = pg;
  tiny.weights[0] = 1.0f - 1e-7f, tiny.weights[1] = 1e-30f;  // a positive holding below the divide's domain
  kind("gaussian_tiny_weight", e, make_sim(SMMC_MODE_GAUSSIAN, 12, 0, 0), tiny);
  smmc_portfolio zero = pg;
  zero.weights[0] = 1.0f, zero.weights[1] = 0.0f;  // a holding of exactly 0 is safe
  kind("gaussian_zero_weight", e, make_sim(SMMC_MODE_GAUSSIAN, 36, 0, 0), zero);
  smmc_sim no_capital = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
  no_capital.initial_capital = 0.0f;
  kind("no_capital", e, no_capital, pg);

  // the accumulator lease: a portfolio call whose launch fails has taken the engine's bucket accumulator and not given
  // it back clean; the next user (a plain simulate through tests/cpp/launch_fake.cpp) must still get its own buckets
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
    smmc_portfolio_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_stats = stats;
    const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 36, 16, 0);
    const int failed = smmc_engine_simulate_portfolio(l, &g, &pg, &o);
    const int second = smmc_engine_simulate_to_host(l, &s, out.data(), nullptr, nullptr, nullptr, &st, again.data());
    std::printf("lease:after_failed_launch %d %d %d %d %d\n", first, failed, second, hist == want ? 1 : 0, again == want ? 1 : 0);
    smmc_engine_destroy(l);
  }

  // the extension slots: cash flows (a staged schedule) and the asset table on ONE engine; both are found again, and
  // smmc_engine_destroy gives back every allocation of both
  {
    const size_t live_before = fake_hip_live_allocations();
    smmc_engine *x = nullptr;
    if (smmc_engine_create(0, nullptr, &x) != SMMC_OK) return 1;
    const size_t live_engine = fake_hip_live_allocations();
    const int set1 = smmc_engine_set_asset_table(x, rows2, 3, 2);
    const size_t live_table = fake_hip_live_allocations();
    std::vector<float> amounts(360, 1.0f);
    smmc_cashflow cf;
    std::memset(&cf, 0, sizeof cf);
    cf.struct_size = sizeof cf;
    cf.amounts = amounts.data();
    cf.floor = 0.01f;
    const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
    static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
    const int cf1 = smmc_engine_simulate_cashflow(x, &g, &cf, nullptr, nullptr, nullptr, nullptr, depleted);  // stages, then no kernel
    const size_t live_both = fake_hip_live_allocations();
    const int cf2 = smmc_engine_simulate_cashflow(x, &g, &cf, nullptr, nullptr, nullptr, nullptr, depleted);  // finds its slot again
    const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 0, 0);
    const int kind_after = smmc_engine_portfolio_divide_kind(x, &tab, &pt);                                     // ... and so does the table
    const int set2 = smmc_engine_set_asset_table(x, rows2, 3, 2);
    const size_t live_steady = fake_hip_live_allocations();
    smmc_engine_destroy(x);
    std::printf("slots:two_owners %d %d %d %d %d %zu %zu %zu %zu\n", set1, cf1, cf2, kind_after, set2, live_table - live_engine,
                live_both - live_table, live_steady - live_both, fake_hip_live_allocations() - live_before);
  }

  std::printf("sizes %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_portfolio_outputs));
  for (smmc_engine *p : {e, no_table, three, big}) smmc_engine_destroy(p);
  std::printf("portfolio_args: done\n");
  return 0;
}
