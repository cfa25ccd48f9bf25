// real_cashflow_args.cpp -- the argument checks and the divide rule of smmc_engine_simulate_real_cashflow, its _to_host
// form and smmc_engine_real_cashflow_divide_kind (include/smmc.h) without a GPU: csrc/smmc_real_cashflow.cpp and the
// library's other host units over tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check
// runs before any device work, so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error()
// and without a launch; TEST INFRASTRUCTURE, driven by tests/test_real_cashflow_cpu.py (built with
// -fsanitize=address,undefined and run directly).  Prints one line per case: "<name> <return code> <length of the error
// text> <launches the call made>" and the text behind "#", then "kind:<case> <SMMC_DIV_*>", "ran:<case> <return code>
// <1: the launch asked for the IEEE divide>", "lease:..." and "sizes ..." lines, then "real_cashflow_args: done".
// The requests hold K = 2 assets; the joint law is three series wide and its last series is inflation.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"

extern "C" int fake_real_cashflow_launches(void);
extern "C" int fake_real_cashflow_last_exact(void);
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

// 60 / 40 and an inflation series; Gaussian fields as asked: (means 0.5, 0.2, 0.25; L = [[4, 0, 0], [0.9, 1.2, 0], [0.1,
// 0.05, 0.4]]) or all zero for table mode
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
    p.means[2] = 0.25f;
    p.factor[0] = 4.0f;
    p.factor[SMMC_MAX_ASSETS] = 0.9f;
    p.factor[SMMC_MAX_ASSETS + 1] = 1.2f;
    p.factor[2 * SMMC_MAX_ASSETS] = 0.1f;
    p.factor[2 * SMMC_MAX_ASSETS + 1] = 0.05f;
    p.factor[2 * SMMC_MAX_ASSETS + 2] = 0.4f;
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

static void report(const char *name, int rc, int launches) {
  std::printf("%s %d %zu %d\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0), launches);
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr, *no_table = nullptr, *two = nullptr, *big = nullptr;
  for (smmc_engine **p : {&e, &no_table, &two, &big})
    if (smmc_engine_create(0, nullptr, p) != SMMC_OK) {
      std::printf("engine_create failed: %s\n", smmc_last_error());
      return 1;
    }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float rows3[9] = {1.0f, 0.2f, 0.3f, -2.0f, 0.4f, 0.2f, 0.5f, -0.3f, -0.1f};  // 3 rows x (2 assets, inflation)
  const float rows2[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};                     // 3 rows x 2: the assets alone
  if (smmc_engine_set_asset_table(e, rows3, 3, 3) != SMMC_OK) return 1;  // note: e has NO single-series table
  if (smmc_engine_set_asset_table(two, rows2, 3, 2) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);                // 4096 rows x (3 assets, inflation): 64 KiB of LDS
  if (smmc_engine_set_asset_table(big, largest.data(), SMMC_MAX_TABLE / 4, 4) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  alignas(8) static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
  static float finals[1000], reals[1000], index[1000], holdings[4000], paid[1000];
  static uint32_t ruin[1000];
  std::vector<float> steady(SMMC_MAX_CASHFLOW_PERIODS, 3.0f), bad_amounts(360, 3.0f), bad_fractions(360, 0.001f);
  bad_amounts[200] = nan;
  bad_fractions[359] = inf;

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c,
                    const smmc_real_cashflow_outputs *o) {
      if (entry == 0) return smmc_engine_simulate_real_cashflow(eng, s, p, c, o);
      if (entry == 1) return smmc_engine_simulate_real_cashflow_to_host(eng, s, p, c, o);
      return smmc_engine_real_cashflow_divide_kind(eng, s, p, c);
    };
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    smmc_real_cashflow_outputs out;
    std::memset(&out, 0, sizeof out);
    out.struct_size = sizeof out;
    out.d_final = finals;
    out.d_final_real = reals;
    out.d_index = index;
    out.d_holdings = holdings;
    out.d_paid = paid;
    out.d_ruin_period = ruin;
    out.d_stats = stats;
    out.d_depleted_at = depleted;
    char name[96];
    auto run = [&](const char *what, smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c,
                   const smmc_real_cashflow_outputs *o) {
      const int before = fake_real_cashflow_launches();
      const int rc = call(eng, s, p, c, o);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_real_cashflow_launches() - before);
    };
    const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 100, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
    const smmc_cashflow cf = make_cf(3.0f, 0.001f, 0.01f);
    smmc_portfolio p;
    smmc_cashflow c;
    smmc_sim s;
    // what the portfolio call refuses
    run("engine_null", nullptr, &gau, &pg, &cf, &out);
    run("sim_null", e, nullptr, &pg, &cf, &out);
    s = gau, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &pg, &cf, &out);
    run("portfolio_null", e, &gau, nullptr, &cf, &out);
    p = pg, p.struct_size = sizeof p + 4;
    run("portfolio_struct_size_wrong", e, &gau, &p, &cf, &out);
    p = pg, p.n_assets = 0;
    run("no_assets", e, &gau, &p, &cf, &out);
    p = pg, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &gau, &p, &cf, &out);
    p = pg, p.n_assets = SMMC_MAX_ASSETS, p.weights[0] = p.weights[1] = p.weights[2] = p.weights[3] = 0.25f;
    run("four_assets_leave_no_series_for_inflation", e, &gau, &p, &cf, &out);
    p = pg, p.weights[0] = 0.5f, p.weights[1] = 0.3f, p.weights[2] = 0.2f;
    run("inflation_weighted", e, &gau, &p, &cf, &out);
    p = pt, p.weights[0] = 0.5f, p.weights[1] = 0.3f, p.weights[2] = 0.2f;
    run("inflation_weighted_table", e, &tab, &p, &cf, &out);
    p = pg, p.reserved = 1;
    run("reserved_not_zero", e, &gau, &p, &cf, &out);
    p = pg, p.weights[0] = -0.1f, p.weights[1] = 1.1f;
    run("weight_negative", e, &gau, &p, &cf, &out);
    p = pg, p.weights[0] = nan;
    run("weight_nan", e, &gau, &p, &cf, &out);
    p = pg, p.weights[1] = inf;
    run("weight_infinite", e, &gau, &p, &cf, &out);
    p = pg, p.weights[0] = 0.5f, p.weights[1] = 0.3f, p.weights[3] = 0.2f;
    run("weight_beyond_the_law", e, &gau, &p, &cf, &out);
    p = pg, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &gau, &p, &cf, &out);
    run("table_mode_without_asset_table", no_table, &tab, &pt, &cf, &out);
    run("asset_table_of_the_assets_alone", two, &tab, &pt, &cf, &out);
    run("asset_table_of_other_width", big, &tab, &pt, &cf, &out);
    run("gaussian_fields_in_table_mode", e, &tab, &pg, &cf, &out);
    p = pg, p.means[1] = nan;
    run("mean_nan", e, &gau, &p, &cf, &out);
    p = pg, p.factor[SMMC_MAX_ASSETS] = inf;
    run("factor_infinite", e, &gau, &p, &cf, &out);
    p = pg, p.factor[1] = 0.5f;
    run("factor_above_diagonal", e, &gau, &p, &cf, &out);
    p = pg, p.factor[3 * SMMC_MAX_ASSETS + 3] = 1.0f;
    run("factor_beyond_the_law", e, &gau, &p, &cf, &out);
    p = pg, p.means[3] = 0.1f;
    run("mean_beyond_the_law", e, &gau, &p, &cf, &out);
    p = pg, p.factor[SMMC_MAX_ASSETS + 1] = -1.2f;
    run("diagonal_negative", e, &gau, &p, &cf, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pt, &cf, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pg, &cf, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &pg, &cf, &out);
    s = gau, s.hist_lo = 10.0f, s.hist_hi = 10.0f;
    run("histogram_range_empty", e, &s, &pg, &cf, &out);
    s = gau, s.mode = 7;
    run("unknown_mode", e, &s, &pg, &cf, &out);
    // what the cash-flow call refuses
    run("cashflow_null", e, &gau, &pg, nullptr, &out);
    c = cf, c.struct_size = sizeof c + 8;
    run("cashflow_struct_size_wrong", e, &gau, &pg, &c, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 0, 100, 0);
    run("no_periods", e, &s, &pg, &cf, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0);
    run("too_many_periods", e, &s, &pg, &cf, &out);
    c = cf, c.floor = -1.0f;
    run("floor_negative", e, &gau, &pg, &c, &out);
    c = cf, c.floor = nan;
    run("floor_nan", e, &gau, &pg, &c, &out);
    c = cf, c.amount = inf;
    run("amount_infinite", e, &gau, &pg, &c, &out);
    c = cf, c.fraction = nan;
    run("fraction_nan", e, &gau, &pg, &c, &out);
    c = cf, c.amounts = bad_amounts.data();
    run("amounts_entry_nan", e, &gau, &pg, &c, &out);
    c = cf, c.fractions = bad_fractions.data();
    run("fractions_entry_infinite", e, &gau, &pg, &c, &out);
    if (entry < 2) {
      run("outputs_null", e, &gau, &pg, &cf, nullptr);
      smmc_real_cashflow_outputs o = out;
      o.struct_size = sizeof o - 8;
      run("outputs_struct_size_wrong", e, &gau, &pg, &cf, &o);
      o = out, o.reserved = 3;
      run("outputs_reserved_not_zero", e, &gau, &pg, &cf, &o);
      s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0), s.n_paths = 1ull << 50;
      run("paths_per_workgroup", e, &s, &pg, &cf, &out);
      if (entry == 0) {
        o = out, o.d_paid = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(paid) + 2);
        run("paid_misaligned", e, &gau, &pg, &cf, &o);
        o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
        run("depleted_at_misaligned", e, &gau, &pg, &cf, &o);
      }
      // the largest request there is -- 4096 rows x 4 words, 4097 depletion counters and 4096 buckets, 96 KiB -- fits the
      // 128 KiB an engine assumes at the least, so the LDS refusal cannot be reached with valid arguments
      p = pt, p.n_assets = 3, p.weights[0] = 0.5f, p.weights[1] = p.weights[2] = 0.25f;
      s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, SMMC_MAX_BINS, 0);
      c = cf, c.amounts = steady.data();
      run("valid_largest", big, &s, &p, &c, &out);
      // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
      run("valid_table", e, &tab, &pt, &cf, &out);
      run("valid_gaussian", e, &gau, &pg, &cf, &out);
      p = pt, p.rebalance_every = 0;
      run("valid_buy_and_hold", e, &tab, &p, &cf, &out);
      p = pg, p.means[2] = 0.0f, p.factor[2 * SMMC_MAX_ASSETS] = p.factor[2 * SMMC_MAX_ASSETS + 1] = p.factor[2 * SMMC_MAX_ASSETS + 2] = 0.0f;
      run("valid_no_inflation", e, &gau, &p, &cf, &out);
      c = cf, c.amounts = steady.data(), c.fractions = steady.data();
      run("valid_varying", e, &tab, &pt, &c, &out);
      smmc_real_cashflow_outputs none;
      std::memset(&none, 0, sizeof none);
      none.struct_size = sizeof none;
      run("valid_no_outputs", e, &tab, &pt, &cf, &none);
      s = gau, s.n_paths = 0;
      o = out, o.d_depleted_at = nullptr;  // tests/cpp/cashflow_launch_stub.cpp has no kernel that copies the counts out
      run("valid_no_paths", e, &s, &pg, &cf, &o);  // nothing to launch: SMMC_OK and an empty record
    }
  }

  // which divide a launch uses: SMMC_DIV_FAST = 0, SMMC_DIV_EXACT = 1, never SMMC_DIV_CHECKED
  auto kind = [&](const char *what, smmc_engine *eng, const smmc_sim &s, const smmc_portfolio &p, const smmc_cashflow &c) {
    std::printf("kind:%s %d\n", what, smmc_engine_real_cashflow_divide_kind(eng, &s, &p, &c));
  };
  const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12), hold = make_pf(false, 0);
  const smmc_sim t360 = make_sim(SMMC_MODE_TABLE, 360, 0, 0), g36 = make_sim(SMMC_MODE_GAUSSIAN, 36, 0, 0),
                 g360 = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
  std::vector<float> paying_in(360, -5.0f), mixed(360, -5.0f), zeros(360, 0.0f), rising(360, 3.0f);
  for (int t = 0; t < 360; t += 7) paying_in[t] = 0.0f;
  mixed[300] = 0.5f;  // one withdrawal among the contributions
  for (int t = 0; t < 360; ++t) rising[t] = 3.0f + 0.01f * t;
  smmc_cashflow c;
  // contributions only, the index inside its window: the one shape the rule proves
  kind("zero_flows_table", e, t360, pt, make_cf(0.0f, 0.0f, 0.0f));
  kind("contributions_table", e, t360, pt, make_cf(-10.0f, 0.0f, 0.0f));
  kind("contributions_floor_table", e, t360, pt, make_cf(-10.0f, 0.0f, 0.01f));
  c = make_cf(0.0f, 0.0f, 0.01f), c.amounts = paying_in.data();
  kind("contributions_varying_table", e, t360, pt, c);
  c.fractions = zeros.data();
  kind("contributions_varying_zero_fractions", e, t360, pt, c);
  kind("contributions_gaussian_36", e, g36, pg, make_cf(-10.0f, 0.0f, 0.0f));
  kind("contributions_gaussian_360", e, g360, pg, make_cf(-10.0f, 0.0f, 0.0f));  // asset 0: 72.5 %, 360 times: 2^-167
  kind("contributions_too_large", e, t360, pt, make_cf(-1e37f, 0.0f, 0.0f));     // 360 of them overflow the window
  c = make_cf(0.0f, 0.0f, 0.0f), c.amounts = mixed.data();
  kind("one_withdrawal_among_contributions", e, t360, pt, c);
  // the parent's second shape, one constant withdrawal, is NOT proven here: the nominal amount varies with the index
  kind("withdrawal_floor_rebalanced", e, t360, pt, make_cf(4.0f, 0.0f, 0.01f));
  kind("withdrawal_floor_gaussian_36", e, g36, pg, make_cf(4.0f, 0.0f, 0.01f));
  kind("withdrawal_no_floor_buy_and_hold", e, t360, hold, make_cf(4.0f, 0.0f, 0.0f));
  smmc_portfolio zero = pt;
  zero.weights[0] = 1.0f, zero.weights[1] = 0.0f;  // a holding of exactly 0 is safe
  kind("contributions_zero_weight", e, t360, zero, make_cf(-4.0f, 0.0f, 0.01f));
  smmc_portfolio tiny = pt;
  tiny.weights[0] = 1.0f - 1e-7f, tiny.weights[1] = 1e-30f;  // a share below the divide's domain
  kind("contributions_tiny_weight", e, t360, tiny, make_cf(-4.0f, 0.0f, 0.01f));
  kind("fraction", e, t360, pt, make_cf(0.0f, 0.004f, 0.01f));
  kind("contribution_and_fraction", e, t360, pt, make_cf(-4.0f, 0.004f, 0.01f));
  c = make_cf(0.0f, 0.0f, 0.01f), c.amounts = rising.data();
  kind("varying_withdrawals", e, t360, pt, c);
  kind("exact_flag", e, make_sim(SMMC_MODE_TABLE, 360, 0, SMMC_FLAG_EXACT_DIV), pt, make_cf(-10.0f, 0.0f, 0.0f));
  // the index window: a +100 % month of inflation 360 times is 2^360, 36 times 2^36; a -50 % month likewise below
  const smmc_sim t36 = make_sim(SMMC_MODE_TABLE, 36, 0, 0);
  smmc_engine *dbl = nullptr, *halving = nullptr, *asset_dbl = nullptr;
  const float doubling[6] = {1.0f, 0.2f, 100.0f, -2.0f, 0.4f, 0.2f};  // one +100 % month in the inflation column
  const float halves[6] = {1.0f, 0.2f, -50.0f, -2.0f, 0.4f, 0.2f};    // one -50 % month in the inflation column
  const float asset[6] = {100.0f, 0.2f, 0.3f, -2.0f, 0.4f, 0.2f};     // one +100 % month in column 0
  if (smmc_engine_create(0, nullptr, &dbl) != SMMC_OK || smmc_engine_set_asset_table(dbl, doubling, 2, 3) != SMMC_OK) return 1;
  if (smmc_engine_create(0, nullptr, &halving) != SMMC_OK || smmc_engine_set_asset_table(halving, halves, 2, 3) != SMMC_OK) return 1;
  if (smmc_engine_create(0, nullptr, &asset_dbl) != SMMC_OK || smmc_engine_set_asset_table(asset_dbl, asset, 2, 3) != SMMC_OK) return 1;
  kind("inflation_doubling_360", dbl, t360, pt, make_cf(-10.0f, 0.0f, 0.0f));
  kind("inflation_doubling_36", dbl, t36, pt, make_cf(-10.0f, 0.0f, 0.0f));
  kind("inflation_halving_360", halving, t360, pt, make_cf(-10.0f, 0.0f, 0.0f));
  kind("inflation_halving_36", halving, t36, pt, make_cf(-10.0f, 0.0f, 0.0f));
  // 36 contributions of 1e27 are 2^95; raised with prices that double 36 times they pass 2^127, with tame prices they do not
  kind("contributions_inflated_too_large", dbl, t36, pt, make_cf(-1e27f, 0.0f, 0.0f));
  kind("contributions_large_tame_inflation", e, t36, pt, make_cf(-1e27f, 0.0f, 0.0f));
  kind("table_doubling_360", asset_dbl, t360, pt, make_cf(-10.0f, 0.0f, 0.0f));
  kind("table_doubling_36", asset_dbl, t36, pt, make_cf(-10.0f, 0.0f, 0.0f));
  for (smmc_engine *p : {dbl, halving, asset_dbl}) smmc_engine_destroy(p);
  smmc_portfolio wide = pg;
  wide.factor[0] = 20.0f;  // 100.5 - 7 * 20 < 0: a multiplier may change sign
  kind("gaussian_may_go_negative", e, make_sim(SMMC_MODE_GAUSSIAN, 2, 0, 0), wide, make_cf(-4.0f, 0.0f, 0.01f));
  wide = pg, wide.factor[2 * SMMC_MAX_ASSETS + 2] = 20.0f;  // the same for the inflation series
  kind("inflation_may_go_negative", e, make_sim(SMMC_MODE_GAUSSIAN, 2, 0, 0), wide, make_cf(-4.0f, 0.0f, 0.01f));
  smmc_sim no_capital = t360;
  no_capital.initial_capital = 0.0f;
  kind("no_capital", e, no_capital, pt, make_cf(-10.0f, 0.0f, 0.0f));

  // the form a launch is given is the form the rule names
  {
    smmc_real_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_final = finals;
    int rc = smmc_engine_simulate_real_cashflow(e, &t360, &pt, &(c = make_cf(-4.0f, 0.0f, 0.01f)), &o);
    std::printf("ran:fast %d %d\n", rc, fake_real_cashflow_last_exact());
    rc = smmc_engine_simulate_real_cashflow(e, &t360, &pt, &(c = make_cf(4.0f, 0.004f, 0.01f)), &o);
    std::printf("ran:exact %d %d\n", rc, fake_real_cashflow_last_exact());
  }

  // the accumulator lease: a call whose launch fails has taken the engine's accumulator (buckets and depletion counters)
  // and not given it back clean; the next user (a plain simulate through tests/cpp/launch_fake.cpp) must still get its
  // own buckets
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
    smmc_real_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_stats = stats;
    o.d_depleted_at = depleted;
    const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 36, 16, 0);
    const smmc_cashflow cf = make_cf(4.0f, 0.0f, 0.01f);
    const int failed = smmc_engine_simulate_real_cashflow(l, &g, &pg, &cf, &o);
    const int second = smmc_engine_simulate_to_host(l, &s, out.data(), nullptr, nullptr, nullptr, &st, again.data());
    std::printf("lease:after_failed_launch %d %d %d %d %d\n", first, failed, second, hist == want ? 1 : 0, again == want ? 1 : 0);
    smmc_engine_destroy(l);
  }

  std::printf("sizes %zu %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_cashflow), sizeof(smmc_real_cashflow_outputs));
  for (smmc_engine *p : {e, no_table, two, big}) smmc_engine_destroy(p);
  std::printf("real_cashflow_args: done\n");
  return 0;
}
