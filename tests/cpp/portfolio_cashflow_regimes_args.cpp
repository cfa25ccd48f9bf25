// portfolio_cashflow_regimes_args.cpp -- the argument checks and the divide rule of
// smmc_engine_simulate_portfolio_cashflow_regimes, its _to_host form and smmc_engine_portfolio_cashflow_regimes_divide_kind
// (include/smmc.h) without a GPU: csrc/smmc_portfolio_cashflow_regimes.cpp and the library's other host units over
// tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any device work, so each
// bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error() and without a launch; TEST
// INFRASTRUCTURE, driven by tests/test_portfolio_cashflow_regimes_cpu.py (built with -fsanitize=address,undefined and run
// directly).  Prints one line per case: "<name> <return code> <length of the error text> <launches the call made>" and the
// text behind "#", then "kind:<case> <this call's SMMC_DIV_*>", "union:<case> <regime 0 alone> <regime 1 alone> <both>",
// "ran:<case> <return code> <1: the launch asked for the IEEE divide> <the start1_q16 it was given>" and "sizes ..." lines,
// then "portfolio_cashflow_regimes_args: done".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"

extern "C" int fake_portfolio_cashflow_regimes_launches(void);
extern "C" int fake_portfolio_cashflow_regimes_last_exact(void);
extern "C" uint32_t fake_portfolio_cashflow_regimes_last_start(void);
extern "C" int fake_portfolio_cashflow_launches(void);
namespace smmc {
extern size_t portfolio_cashflow_regimes_stub_extra_lds;  // tests/cpp/portfolio_cashflow_regimes_launch_stub.cpp
}

static smmc_sim make_sim(int32_t mode, uint32_t n_periods, uint32_t n_bins, uint32_t flags) {
  smmc_sim s;
  std::memset(&s, 0, sizeof s);
  s.struct_size = sizeof s;
  s.mode = mode;
  s.seed = 7;
  s.n_paths = 1000;
  s.n_periods = n_periods;
  s.initial_capital = 1000.0f;
  s.gauss_mean = std::numeric_limits<float>::quiet_NaN();  // not read
  s.gauss_std = -1.0f;                                     // not read
  s.n_bins = n_bins;
  s.hist_lo = 0.0f;
  s.hist_hi = 5000.0f;
  s.below_threshold = 1000.0f;
  s.flags = flags;
  return s;
}

static smmc_portfolio make_pf(uint32_t every) {  // 60 / 40, the Gaussian fields all zero
  smmc_portfolio p;
  std::memset(&p, 0, sizeof p);
  p.struct_size = sizeof p;
  p.n_assets = 2;
  p.rebalance_every = every;
  p.weights[0] = 0.6f;
  p.weights[1] = 0.4f;
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

// two calm regimes of two assets: bull (0.8, 0.3; L = [[4, 0], [0.9, 1.2]]) and bear (-1.5, -0.2; L = [[7, 0], [-1.1, 2]])
static smmc_portfolio_regimes make_rg(uint32_t l0, uint32_t l1, uint32_t start) {
  smmc_portfolio_regimes r;
  std::memset(&r, 0, sizeof r);
  r.struct_size = sizeof r;
  r.leave_q16[0] = l0;
  r.leave_q16[1] = l1;
  r.start1_q16 = start;
  r.means[0][0] = 0.8f, r.means[0][1] = 0.3f;
  r.means[1][0] = -1.5f, r.means[1][1] = -0.2f;
  r.factor[0][0] = 4.0f, r.factor[0][SMMC_MAX_ASSETS] = 0.9f, r.factor[0][SMMC_MAX_ASSETS + 1] = 1.2f;
  r.factor[1][0] = 7.0f, r.factor[1][SMMC_MAX_ASSETS] = -1.1f, r.factor[1][SMMC_MAX_ASSETS + 1] = 2.0f;
  return r;
}

static void report(const char *name, int rc, int launches) {
  std::printf("%s %d %zu %d\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0), launches);
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr;
  if (smmc_engine_create(0, nullptr, &e) != SMMC_OK) {
    std::printf("engine_create failed: %s\n", smmc_last_error());
    return 1;
  }
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  alignas(8) static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
  static float finals[1000], holdings[4000], paid[1000];
  static uint32_t ruin[1000];
  std::vector<float> steady(SMMC_MAX_CASHFLOW_PERIODS, 3.0f);

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_portfolio_regimes *r, const smmc_cashflow *c,
                    const smmc_portfolio_cashflow_outputs *o) {
      if (entry == 0) return smmc_engine_simulate_portfolio_cashflow_regimes(eng, s, p, r, c, o);
      if (entry == 1) return smmc_engine_simulate_portfolio_cashflow_regimes_to_host(eng, s, p, r, c, o);
      return smmc_engine_portfolio_cashflow_regimes_divide_kind(eng, s, p, r, c);
    };
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    smmc_portfolio_cashflow_outputs out;
    std::memset(&out, 0, sizeof out);
    out.struct_size = sizeof out;
    out.d_final = finals;
    out.d_holdings = holdings;
    out.d_paid = paid;
    out.d_ruin_period = ruin;
    out.d_stats = stats;
    out.d_depleted_at = depleted;
    char name[96];
    auto run = [&](const char *what, smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_portfolio_regimes *r,
                   const smmc_cashflow *c, const smmc_portfolio_cashflow_outputs *o) {
      const int before = fake_portfolio_cashflow_regimes_launches() + fake_portfolio_cashflow_launches();
      const int rc = call(eng, s, p, r, c, o);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_portfolio_cashflow_regimes_launches() + fake_portfolio_cashflow_launches() - before);
    };
    const smmc_sim gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_portfolio pf = make_pf(12);
    const smmc_cashflow cf = make_cf(3.0f, 0.001f, 0.01f);
    const smmc_portfolio_regimes rg = make_rg(1638, 8192, 16384);
    smmc_portfolio p;
    smmc_cashflow c;
    smmc_sim s;
    smmc_portfolio_regimes r;
    // what the parent refuses of sim, pf and cf
    run("engine_null", nullptr, &gau, &pf, &rg, &cf, &out);
    run("sim_null", e, nullptr, &pf, &rg, &cf, &out);
    s = gau, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &pf, &rg, &cf, &out);
    run("portfolio_null", e, &gau, nullptr, &rg, &cf, &out);
    p = pf, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &gau, &p, &rg, &cf, &out);
    p = pf, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &gau, &p, &rg, &cf, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &pf, &rg, &cf, &out);
    run("cashflow_null", e, &gau, &pf, &rg, nullptr, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 0, 100, 0);
    run("no_periods", e, &s, &pf, &rg, &cf, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0);
    run("too_many_periods", e, &s, &pf, &rg, &cf, &out);
    c = cf, c.floor = -1.0f;
    run("floor_negative", e, &gau, &pf, &rg, &c, &out);
    c = cf, c.fraction = nan;
    run("fraction_nan", e, &gau, &pf, &rg, &c, &out);
    // this call's own: the mode, the stream, pf's Gaussian fields, rg
    s = make_sim(SMMC_MODE_TABLE, 360, 100, 0);
    run("table_mode", e, &s, &pf, &rg, &cf, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pf, &rg, &cf, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pf, &rg, &cf, &out);
    p = pf, p.means[1] = 0.25f;
    run("portfolio_means_set", e, &gau, &p, &rg, &cf, &out);
    p = pf, p.factor[SMMC_MAX_ASSETS] = 0.5f;
    run("portfolio_factor_set", e, &gau, &p, &rg, &cf, &out);
    run("regimes_null", e, &gau, &pf, nullptr, &cf, &out);
    r = rg, r.struct_size = sizeof r + 4;
    run("regimes_struct_size_wrong", e, &gau, &pf, &r, &cf, &out);
    r = make_rg(SMMC_REGIME_Q16_ONE + 1u, 8192, 0);
    run("leave0_above_one", e, &gau, &pf, &r, &cf, &out);
    r = make_rg(1638, 0xffffffffu, 0);
    run("leave1_all_ones", e, &gau, &pf, &r, &cf, &out);
    r = make_rg(1638, 8192, SMMC_REGIME_Q16_ONE + 1u);
    run("start_above_one", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.means[0][1] = nan;
    run("mean_nan", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.means[1][0] = inf;
    run("mean_infinite_in_regime_1", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.means[1][2] = 0.5f;
    run("mean_beyond_n_assets", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.factor[1][SMMC_MAX_ASSETS] = nan;
    run("factor_nan", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.factor[0][1] = 0.5f;
    run("factor_above_diagonal", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.factor[1][2 * SMMC_MAX_ASSETS] = 0.5f;
    run("factor_beyond_n_assets", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.factor[1][SMMC_MAX_ASSETS + 1] = -2.0f;
    run("factor_negative_diagonal", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.reserved[0] = 1;
    run("regimes_reserved0_not_zero", e, &gau, &pf, &r, &cf, &out);
    r = rg, r.reserved[1] = 7;
    run("regimes_reserved1_not_zero", e, &gau, &pf, &r, &cf, &out);
    if (entry < 2) {
      run("outputs_null", e, &gau, &pf, &rg, &cf, nullptr);
      smmc_portfolio_cashflow_outputs o = out;
      o.struct_size = sizeof o - 8;
      run("outputs_struct_size_wrong", e, &gau, &pf, &rg, &cf, &o);
      o = out, o.reserved = 3;
      run("outputs_reserved_not_zero", e, &gau, &pf, &rg, &cf, &o);
      s = gau, s.n_paths = 1ull << 50;
      run("paths_per_workgroup", e, &s, &pf, &rg, &cf, &out);
      if (entry == 0) {
        o = out, o.d_paid = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(paid) + 2);
        run("paid_misaligned", e, &gau, &pf, &rg, &cf, &o);
        o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
        run("depleted_at_misaligned", e, &gau, &pf, &rg, &cf, &o);
      }
    }
    // the largest request fits any device the library runs on: the stub's LDS need is raised beyond it for this one case
    s = make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS, SMMC_MAX_BINS, 0);
    c = cf, c.amounts = steady.data();
    smmc::portfolio_cashflow_regimes_stub_extra_lds = size_t(1) << 20;
    run("lds_too_small", e, &s, &pf, &rg, &c, &out);
    smmc::portfolio_cashflow_regimes_stub_extra_lds = 0;
    if (entry < 2) {
      run("valid_largest", e, &s, &pf, &rg, &c, &out);
      // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
      run("valid", e, &gau, &pf, &rg, &cf, &out);
      r = make_rg(0, 0, 0);
      run("valid_never_left", e, &gau, &pf, &r, &cf, &out);
      r = make_rg(SMMC_REGIME_Q16_ONE, SMMC_REGIME_Q16_ONE, SMMC_REGIME_Q16_ONE);
      run("valid_always_left", e, &gau, &pf, &r, &cf, &out);
      s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_EXACT_DIV);
      run("valid_exact_div_flag", e, &s, &pf, &rg, &cf, &out);
      c = cf, c.amounts = steady.data(), c.fractions = steady.data();
      run("valid_varying", e, &gau, &pf, &rg, &c, &out);
      smmc_portfolio_cashflow_outputs none;
      std::memset(&none, 0, sizeof none);
      none.struct_size = sizeof none;
      run("valid_no_outputs", e, &gau, &pf, &rg, &cf, &none);
      s = gau, s.n_paths = 0;
      smmc_portfolio_cashflow_outputs o = out;
      o.d_depleted_at = nullptr;  // the launch stubs have no kernel that copies the counts out
      run("valid_no_paths", e, &s, &pf, &rg, &cf, &o);  // nothing to launch: SMMC_OK and an empty record
    }
  }

  // the divide rule on the union of the two regimes' bounds
  const smmc_portfolio pf = make_pf(12), hold = make_pf(0);
  // 120 periods: the bear regime's best month is 100 - 1.5 + 7 * 7 = 147.5, and 360 of those leave binary32 (the rule's own bound)
  const smmc_sim g120 = make_sim(SMMC_MODE_GAUSSIAN, 120, 0, 0), exact = make_sim(SMMC_MODE_GAUSSIAN, 120, 0, SMMC_FLAG_EXACT_DIV);
  const smmc_sim g360 = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
  const smmc_portfolio_regimes calm = make_rg(1638, 8192, 16384);
  smmc_portfolio_regimes wild = make_rg(0, 0, 0);  // regime 1 can never be entered; its lower bound is below 0: 100 - 1.5 - 7 * 15
  wild.factor[1][0] = 15.0f;
  const smmc_cashflow floor_withdrawal = make_cf(4.0f, 0.0f, 0.01f);
  auto kind = [&](const char *name, const smmc_sim &s, const smmc_portfolio &p, const smmc_portfolio_regimes &r, const smmc_cashflow &c) {
    std::printf("kind:%s %d\n", name, smmc_engine_portfolio_cashflow_regimes_divide_kind(e, &s, &p, &r, &c));
  };
  kind("both_calm", g120, pf, calm, floor_withdrawal);
  kind("both_calm_zero_flows", g120, pf, calm, make_cf(0.0f, 0.0f, 0.0f));
  kind("both_calm_contributions", g120, pf, calm, make_cf(-10.0f, 0.0f, 0.0f));
  kind("both_calm_no_floor_rebalanced", g120, pf, calm, make_cf(4.0f, 0.0f, 0.0f));
  kind("both_calm_no_floor_buy_and_hold", g120, hold, calm, make_cf(4.0f, 0.0f, 0.0f));
  kind("regime_never_entered_without_bounds", g120, pf, wild, floor_withdrawal);
  kind("both_calm_too_many_periods", g360, pf, calm, floor_withdrawal);
  kind("exact_flag", exact, pf, calm, floor_withdrawal);
  kind("fraction", g120, pf, calm, make_cf(0.0f, 0.004f, 0.01f));

  // Each regime alone FAST through a different condition of the rule, the union EXACT.  One constant contribution (all
  // paid in, constant): the rule proves FAST either from the worst asset's shrinking over P periods (condition A) or, per
  // asset, from the least holding that enters a product (condition B).  Capital 1, weights (1 - 2^-20, 2^-20), amount
  // -2^-41, buy and hold, P = 5.  Regime 0: asset 1's lower bound is about 0.2 (B fails for asset 1: its least holding
  // 2^-86 times 0.2 is below 2^-88), asset 0 calm (A holds: five periods at 0.2 / 100 shrink by 2^-45).  Regime 1: asset
  // 0's lower bound is about 0.01 (A fails: five periods at 0.01 / 100 shrink by 2^-66 from 2^-20), asset 1's is 1 or
  // more (B holds for both).  The union has both low bounds: A fails as in regime 1, B as in regime 0.
  {
    smmc_sim s = make_sim(SMMC_MODE_GAUSSIAN, 5, 0, 0);
    s.initial_capital = 1.0f;
    smmc_portfolio p = make_pf(0);
    p.weights[1] = std::ldexp(1.0f, -20);
    p.weights[0] = 1.0f - p.weights[1];
    const smmc_cashflow c = make_cf(-std::ldexp(1.0f, -41), 0.0f, 0.0f);
    // lower bound of a lone diagonal entry d at mean 0: 100 - 7 * nextafter(d) - 1e-3
    const float to_0_2 = static_cast<float>((100.0 - 0.2 - 1e-3) / 7.0), to_0_01 = static_cast<float>((100.0 - 0.01 - 1e-3) / 7.0);
    smmc_portfolio_regimes both;
    std::memset(&both, 0, sizeof both);
    both.struct_size = sizeof both;
    both.leave_q16[0] = both.leave_q16[1] = 8192;
    both.factor[0][0] = 1.0f, both.factor[0][SMMC_MAX_ASSETS + 1] = to_0_2;
    both.factor[1][0] = to_0_01, both.factor[1][SMMC_MAX_ASSETS + 1] = 1.0f;
    smmc_portfolio_regimes only0 = both, only1 = both;
    std::memcpy(only0.factor[1], both.factor[0], sizeof both.factor[0]);
    std::memcpy(only1.factor[0], both.factor[1], sizeof both.factor[1]);
    std::printf("union:different_conditions %d %d %d\n", smmc_engine_portfolio_cashflow_regimes_divide_kind(e, &s, &p, &only0, &c),
                smmc_engine_portfolio_cashflow_regimes_divide_kind(e, &s, &p, &only1, &c),
                smmc_engine_portfolio_cashflow_regimes_divide_kind(e, &s, &p, &both, &c));
    // the parent says the same of each regime's law alone
    for (int r = 0; r < 2; ++r) {
      smmc_portfolio law = p;
      std::memcpy(law.factor, both.factor[r], sizeof law.factor);
      smmc_sim plain = s;
      plain.gauss_mean = 0.0f, plain.gauss_std = 1.0f;
      std::printf("parent:regime_%d %d\n", r, smmc_engine_portfolio_cashflow_divide_kind(e, &plain, &law, &c));
    }
  }
  // the launch is given the form the rule names, and the probabilities
  {
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_final = finals;
    const smmc_portfolio_regimes a = make_rg(1638, 8192, 12), b = make_rg(1638, 8192, 77);
    int rc = smmc_engine_simulate_portfolio_cashflow_regimes(e, &g120, &pf, &a, &floor_withdrawal, &o);
    std::printf("ran:fast %d %d %u\n", rc, fake_portfolio_cashflow_regimes_last_exact(), fake_portfolio_cashflow_regimes_last_start());
    const smmc_cashflow slow = make_cf(0.0f, 0.004f, 0.01f);
    rc = smmc_engine_simulate_portfolio_cashflow_regimes(e, &g120, &pf, &b, &slow, &o);
    std::printf("ran:exact %d %d %u\n", rc, fake_portfolio_cashflow_regimes_last_exact(), fake_portfolio_cashflow_regimes_last_start());
    rc = smmc_engine_simulate_portfolio_cashflow_regimes(e, &exact, &pf, &b, &floor_withdrawal, &o);
    std::printf("ran:exact_flag %d %d %u\n", rc, fake_portfolio_cashflow_regimes_last_exact(), fake_portfolio_cashflow_regimes_last_start());
  }
  std::printf("sizes %zu %zu %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_cashflow), sizeof(smmc_portfolio_regimes),
              sizeof(smmc_portfolio_cashflow_outputs));
  smmc_engine_destroy(e);
  std::printf("portfolio_cashflow_regimes_args: done\n");
  return 0;
}
