// portfolio_cashflow_stationary_args.cpp -- the argument checks and the divide rule of
// smmc_engine_simulate_portfolio_cashflow_stationary, its _to_host form and
// smmc_engine_portfolio_cashflow_stationary_divide_kind (include/smmc.h) without a GPU:
// csrc/smmc_portfolio_cashflow_stationary.cpp and the library's other host units over tests/cpp/fake_hip.cpp,
// tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any device work, so each bad request must come
// back as SMMC_ERR_INVALID with a text in smmc_last_error() and without a launch; TEST INFRASTRUCTURE, driven by
// tests/test_portfolio_cashflow_stationary_cpu.py (built with -fsanitize=address,undefined and run directly).  Prints one
// line per case: "<name> <return code> <length of the error text> <launches the call made>" and the text behind "#", then
// "kind:<case>:<q> <this call's SMMC_DIV_*> <the parent's>", "ran:<case> <return code> <1: the launch asked for the IEEE
// divide> <the renew_q16 it was given>" and "sizes ..." lines, then "portfolio_cashflow_stationary_args: done".
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"

extern "C" int fake_portfolio_cashflow_stationary_launches(void);
extern "C" int fake_portfolio_cashflow_stationary_last_exact(void);
extern "C" uint32_t fake_portfolio_cashflow_stationary_last_renew(void);
extern "C" int fake_portfolio_cashflow_launches(void);
namespace smmc {
extern size_t portfolio_cashflow_stationary_stub_extra_lds;  // tests/cpp/portfolio_cashflow_stationary_launch_stub.cpp
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

static smmc_cashflow make_cf(float amount, float fraction, float floor) {
  smmc_cashflow c;
  std::memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.amount = amount;
  c.fraction = fraction;
  c.floor = floor;
  return c;
}

static smmc_stationary make_st(uint32_t q) {
  smmc_stationary st;
  std::memset(&st, 0, sizeof st);
  st.struct_size = sizeof st;
  st.renew_q16 = q;
  return st;
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
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float rows[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};
  if (smmc_engine_set_asset_table(e, rows, 3, 2) != SMMC_OK) return 1;  // note: e has NO single-series table
  if (smmc_engine_set_asset_table(three, rows, 2, 3) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);  // 4096 rows x 4 assets
  if (smmc_engine_set_asset_table(big, largest.data(), SMMC_MAX_TABLE / 4, 4) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  alignas(8) static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
  static float finals[1000], holdings[4000], paid[1000];
  static uint32_t ruin[1000];
  std::vector<float> steady(SMMC_MAX_CASHFLOW_PERIODS, 3.0f);

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c, const smmc_stationary *st,
                    const smmc_portfolio_cashflow_outputs *o) {
      if (entry == 0) return smmc_engine_simulate_portfolio_cashflow_stationary(eng, s, p, c, st, o);
      if (entry == 1) return smmc_engine_simulate_portfolio_cashflow_stationary_to_host(eng, s, p, c, st, o);
      return smmc_engine_portfolio_cashflow_stationary_divide_kind(eng, s, p, c, st);
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
    auto run = [&](const char *what, smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c,
                   const smmc_stationary *st, const smmc_portfolio_cashflow_outputs *o) {
      const int before = fake_portfolio_cashflow_stationary_launches() + fake_portfolio_cashflow_launches();
      const int rc = call(eng, s, p, c, st, o);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_portfolio_cashflow_stationary_launches() + fake_portfolio_cashflow_launches() - before);
    };
    const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 100, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
    const smmc_cashflow cf = make_cf(3.0f, 0.001f, 0.01f);
    const smmc_stationary q12 = make_st(5461);
    smmc_portfolio p;
    smmc_cashflow c;
    smmc_sim s;
    smmc_stationary st;
    // what the portfolio call refuses (the whole list runs in tests/cpp/portfolio_cashflow_blocks_args.cpp: the check is lent)
    run("engine_null", nullptr, &tab, &pt, &cf, &q12, &out);
    run("sim_null", e, nullptr, &pt, &cf, &q12, &out);
    run("portfolio_null", e, &tab, nullptr, &cf, &q12, &out);
    p = pt, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &tab, &p, &cf, &q12, &out);
    p = pt, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &tab, &p, &cf, &q12, &out);
    run("table_mode_without_asset_table", no_table, &tab, &pt, &cf, &q12, &out);
    run("asset_table_of_other_width", three, &tab, &pt, &cf, &q12, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pt, &cf, &q12, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pt, &cf, &q12, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &pt, &cf, &q12, &out);
    // what the cash-flow call refuses
    run("cashflow_null", e, &tab, &pt, nullptr, &q12, &out);
    s = make_sim(SMMC_MODE_TABLE, 0, 100, 0);
    run("no_periods", e, &s, &pt, &cf, &q12, &out);
    s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0);
    run("too_many_periods", e, &s, &pt, &cf, &q12, &out);
    c = cf, c.floor = -1.0f;
    run("floor_negative", e, &tab, &pt, &c, &q12, &out);
    c = cf, c.fraction = nan;
    run("fraction_nan", e, &tab, &pt, &c, &q12, &out);
    // this call's own: what the stationary bootstrap refuses, the mode among it
    run("gaussian_mode", e, &gau, &pg, &cf, &q12, &out);
    run("stationary_null", e, &tab, &pt, &cf, nullptr, &out);
    st = q12, st.struct_size = sizeof st + 4;
    run("stationary_struct_size_wrong", e, &tab, &pt, &cf, &st, &out);
    st = make_st(SMMC_RENEW_Q16_ONE + 1u);
    run("renew_above_one", e, &tab, &pt, &cf, &st, &out);
    st = make_st(0xffffffffu);
    run("renew_all_ones", e, &tab, &pt, &cf, &st, &out);
    st = q12, st.reserved[0] = 1;
    run("stationary_reserved0_not_zero", e, &tab, &pt, &cf, &st, &out);
    st = q12, st.reserved[1] = 7;
    run("stationary_reserved1_not_zero", e, &tab, &pt, &cf, &st, &out);
    // the order: the portfolio's refusal before the schedule's before the stationary argument's
    p = pt, p.n_assets = 0;
    c = cf, c.floor = -1.0f;
    st = make_st(SMMC_RENEW_Q16_ONE + 1u);
    run("order_portfolio_first", e, &tab, &p, &c, &st, &out);
    run("order_schedule_before_stationary", e, &tab, &pt, &c, &st, &out);
    run("order_stationary_struct_before_mode", e, &gau, &pg, &cf, nullptr, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2);
    run("order_portfolios_stream_before_the_mode", e, &s, &pg, &cf, &q12, &out);
    if (entry < 2) {
      run("outputs_null", e, &tab, &pt, &cf, &q12, nullptr);
      smmc_portfolio_cashflow_outputs o = out;
      o.struct_size = sizeof o - 8;
      run("outputs_struct_size_wrong", e, &tab, &pt, &cf, &q12, &o);
      o = out, o.reserved = 3;
      run("outputs_reserved_not_zero", e, &tab, &pt, &cf, &q12, &o);
      run("order_stationary_before_outputs", e, &tab, &pt, &cf, &st, nullptr);
      s = tab, s.n_paths = 1ull << 50;
      run("paths_per_workgroup", e, &s, &pt, &cf, &q12, &out);
      if (entry == 0) {
        o = out, o.d_paid = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(paid) + 2);
        run("paid_misaligned", e, &tab, &pt, &cf, &q12, &o);
        o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
        run("depleted_at_misaligned", e, &tab, &pt, &cf, &q12, &o);
      }
      // the largest request fits any device the library runs on: the stub's LDS need is raised beyond it for this one case
      p = pt, p.n_assets = 4, p.weights[0] = p.weights[1] = p.weights[2] = p.weights[3] = 0.25f;
      s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, SMMC_MAX_BINS, 0);
      c = cf, c.amounts = steady.data();
      smmc::portfolio_cashflow_stationary_stub_extra_lds = size_t(1) << 20;
      run("lds_too_small", big, &s, &p, &c, &q12, &out);
      smmc::portfolio_cashflow_stationary_stub_extra_lds = 0;
      run("valid_largest", big, &s, &p, &c, &q12, &out);
      // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
      run("valid_table", e, &tab, &pt, &cf, &q12, &out);
      st = make_st(0);
      run("valid_never", e, &tab, &pt, &cf, &st, &out);
      st = make_st(SMMC_RENEW_Q16_ONE);
      run("valid_always", e, &tab, &pt, &cf, &st, &out);
      s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_EXACT_DIV);
      run("valid_exact_div_flag", e, &s, &pt, &cf, &q12, &out);
      c = cf, c.amounts = steady.data(), c.fractions = steady.data();
      run("valid_varying", e, &tab, &pt, &c, &q12, &out);
      smmc_portfolio_cashflow_outputs none;
      std::memset(&none, 0, sizeof none);
      none.struct_size = sizeof none;
      run("valid_no_outputs", e, &tab, &pt, &cf, &q12, &none);
      s = tab, s.n_paths = 0;
      o = out, o.d_depleted_at = nullptr;  // the launch stubs have no kernel that copies the counts out
      run("valid_no_paths", e, &s, &pt, &cf, &q12, &o);  // nothing to launch: SMMC_OK and an empty record
    }
  }

  // which divide a launch uses: what the parent's rule says of (sim, pf, cf), for every renewal probability
  const smmc_portfolio pt = make_pf(false, 12), hold = make_pf(false, 0);
  const smmc_sim t360 = make_sim(SMMC_MODE_TABLE, 360, 0, 0), exact = make_sim(SMMC_MODE_TABLE, 360, 0, SMMC_FLAG_EXACT_DIV);
  std::vector<float> paying_in(360, -5.0f), rising(360, 3.0f);
  for (int t = 0; t < 360; ++t) rising[t] = 3.0f + 0.01f * t;
  smmc_cashflow varying_in = make_cf(0.0f, 0.0f, 0.01f), varying_out = make_cf(0.0f, 0.0f, 0.01f);
  varying_in.amounts = paying_in.data();
  varying_out.amounts = rising.data();
  struct Request {
    const char *name;
    smmc_sim s;
    smmc_portfolio p;
    smmc_cashflow c;
  };
  const Request grid[] = {{"zero_flows", t360, pt, make_cf(0.0f, 0.0f, 0.0f)},
                          {"contributions", t360, pt, make_cf(-10.0f, 0.0f, 0.0f)},
                          {"contributions_varying", t360, pt, varying_in},
                          {"withdrawal_floor_rebalanced", t360, pt, make_cf(4.0f, 0.0f, 0.01f)},
                          {"withdrawal_no_floor_rebalanced", t360, pt, make_cf(4.0f, 0.0f, 0.0f)},
                          {"withdrawal_no_floor_buy_and_hold", t360, hold, make_cf(4.0f, 0.0f, 0.0f)},
                          {"fraction", t360, pt, make_cf(0.0f, 0.004f, 0.01f)},
                          {"varying_withdrawals", t360, pt, varying_out},
                          {"exact_flag", exact, pt, make_cf(4.0f, 0.0f, 0.01f)}};
  for (const Request &r : grid)
    for (uint32_t q : {0u, 1u, 5461u, 65535u, 65536u}) {
      const smmc_stationary st = make_st(q);
      std::printf("kind:%s:%u %d %d\n", r.name, q, smmc_engine_portfolio_cashflow_stationary_divide_kind(e, &r.s, &r.p, &r.c, &st),
                  smmc_engine_portfolio_cashflow_divide_kind(e, &r.s, &r.p, &r.c));
    }
  // the launch is given the form the rule names, and the renewal probability
  {
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_final = finals;
    const smmc_stationary a = make_st(12), b = make_st(77);
    const smmc_cashflow fast = make_cf(4.0f, 0.0f, 0.01f), slow = make_cf(0.0f, 0.004f, 0.01f);
    int rc = smmc_engine_simulate_portfolio_cashflow_stationary(e, &t360, &pt, &fast, &a, &o);
    std::printf("ran:fast %d %d %u\n", rc, fake_portfolio_cashflow_stationary_last_exact(), fake_portfolio_cashflow_stationary_last_renew());
    rc = smmc_engine_simulate_portfolio_cashflow_stationary(e, &t360, &pt, &slow, &b, &o);
    std::printf("ran:exact %d %d %u\n", rc, fake_portfolio_cashflow_stationary_last_exact(), fake_portfolio_cashflow_stationary_last_renew());
    rc = smmc_engine_simulate_portfolio_cashflow_stationary(e, &exact, &pt, &fast, &b, &o);
    std::printf("ran:exact_flag %d %d %u\n", rc, fake_portfolio_cashflow_stationary_last_exact(), fake_portfolio_cashflow_stationary_last_renew());
  }
  std::printf("sizes %zu %zu %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_cashflow), sizeof(smmc_stationary),
              sizeof(smmc_portfolio_cashflow_outputs));
  for (smmc_engine *p : {e, no_table, three, big}) smmc_engine_destroy(p);
  std::printf("portfolio_cashflow_stationary_args: done\n");
  return 0;
}
