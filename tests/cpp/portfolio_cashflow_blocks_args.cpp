// portfolio_cashflow_blocks_args.cpp -- the argument checks and the divide rule of
// smmc_engine_simulate_portfolio_cashflow_blocks, its _to_host form and smmc_engine_portfolio_cashflow_blocks_divide_kind
// (include/smmc.h) without a GPU: csrc/smmc_portfolio_cashflow_blocks.cpp and the library's other host units over
// tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any device work, so
// each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error() and without a launch; TEST
// INFRASTRUCTURE, driven by tests/test_portfolio_cashflow_blocks_cpu.py (built with -fsanitize=address,undefined and run
// directly).  Prints one line per case: "<name> <return code> <length of the error text> <launches the call made>" and the
// text behind "#", then "kind:<case> <this call's SMMC_DIV_*> <the parent's>", "ran:<case> <return code> <1: the launch
// asked for the IEEE divide> <the block length it was given>", "staged:...", "lease:..." and "sizes ..." lines, then
// "portfolio_cashflow_blocks_args: done".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"
#include "smmc_internal.h"

extern "C" int fake_portfolio_cashflow_blocks_launches(void);
extern "C" int fake_portfolio_cashflow_blocks_last_exact(void);
extern "C" uint32_t fake_portfolio_cashflow_blocks_last_block_len(void);
extern "C" const void *fake_portfolio_cashflow_blocks_last_kernel_args(void);
extern "C" const void *fake_portfolio_cashflow_blocks_last_args(void);
extern "C" int fake_portfolio_cashflow_launches(void);
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

static smmc_cashflow make_cf(float amount, float fraction, float floor) {
  smmc_cashflow c;
  std::memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.amount = amount;
  c.fraction = fraction;
  c.floor = floor;
  return c;
}

static smmc_blocks make_blocks(uint32_t len) {
  smmc_blocks b;
  std::memset(&b, 0, sizeof b);
  b.struct_size = sizeof b;
  b.block_len = len;
  b.kind = SMMC_BLOCKS_CIRCULAR;
  return b;
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
  const float rows2[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};         // 3 rows x 2 assets
  const float rows3[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};         // 2 rows x 3 assets
  if (smmc_engine_set_asset_table(e, rows2, 3, 2) != SMMC_OK) return 1;  // note: e has NO single-series table
  if (smmc_engine_set_asset_table(three, rows3, 2, 3) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);                // 4096 rows x 4 assets: 64 KiB of LDS, and 112 bytes more
  if (smmc_engine_set_asset_table(big, largest.data(), SMMC_MAX_TABLE / 4, 4) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  alignas(8) static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
  static float finals[1000], holdings[4000], paid[1000];
  static uint32_t ruin[1000];
  std::vector<float> steady(SMMC_MAX_CASHFLOW_PERIODS, 3.0f), bad_amounts(360, 3.0f), bad_fractions(360, 0.001f);
  bad_amounts[200] = nan;
  bad_fractions[359] = inf;

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c, const smmc_blocks *b,
                    const smmc_portfolio_cashflow_outputs *o) {
      if (entry == 0) return smmc_engine_simulate_portfolio_cashflow_blocks(eng, s, p, c, b, o);
      if (entry == 1) return smmc_engine_simulate_portfolio_cashflow_blocks_to_host(eng, s, p, c, b, o);
      return smmc_engine_portfolio_cashflow_blocks_divide_kind(eng, s, p, c, b);
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
                   const smmc_blocks *b, const smmc_portfolio_cashflow_outputs *o) {
      const int before = fake_portfolio_cashflow_blocks_launches() + fake_portfolio_cashflow_launches();
      const int rc = call(eng, s, p, c, b, o);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_portfolio_cashflow_blocks_launches() + fake_portfolio_cashflow_launches() - before);
    };
    const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 100, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
    const smmc_cashflow cf = make_cf(3.0f, 0.001f, 0.01f);
    const smmc_blocks bl = make_blocks(12);
    smmc_portfolio p;
    smmc_cashflow c;
    smmc_sim s;
    smmc_blocks b;
    // what the portfolio call refuses
    run("engine_null", nullptr, &tab, &pt, &cf, &bl, &out);
    run("sim_null", e, nullptr, &pt, &cf, &bl, &out);
    s = tab, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &pt, &cf, &bl, &out);
    run("portfolio_null", e, &tab, nullptr, &cf, &bl, &out);
    p = pt, p.struct_size = sizeof p + 4;
    run("portfolio_struct_size_wrong", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.n_assets = 0;
    run("no_assets", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.reserved = 1;
    run("reserved_not_zero", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.weights[0] = -0.1f, p.weights[1] = 1.1f;
    run("weight_negative", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.weights[0] = nan;
    run("weight_nan", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.weights[1] = inf;
    run("weight_infinite", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.weights[0] = 0.5f, p.weights[1] = 0.3f, p.weights[2] = 0.2f;
    run("weight_beyond_assets", e, &tab, &p, &cf, &bl, &out);
    p = pt, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &tab, &p, &cf, &bl, &out);
    run("table_mode_without_asset_table", no_table, &tab, &pt, &cf, &bl, &out);
    run("asset_table_of_other_width", three, &tab, &pt, &cf, &bl, &out);
    run("gaussian_fields_in_table_mode", e, &tab, &pg, &cf, &bl, &out);
    p = pg, p.means[1] = nan;
    run("mean_nan", e, &gau, &p, &cf, &bl, &out);
    p = pg, p.factor[1] = 0.5f;
    run("factor_above_diagonal", e, &gau, &p, &cf, &bl, &out);
    p = pg, p.factor[SMMC_MAX_ASSETS + 1] = -1.2f;
    run("diagonal_negative", e, &gau, &p, &cf, &bl, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pt, &cf, &bl, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pt, &cf, &bl, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &pt, &cf, &bl, &out);
    s = tab, s.hist_lo = 10.0f, s.hist_hi = 10.0f;
    run("histogram_range_empty", e, &s, &pt, &cf, &bl, &out);
    s = tab, s.mode = 7;
    run("unknown_mode", e, &s, &pt, &cf, &bl, &out);
    // what the cash-flow call refuses
    run("cashflow_null", e, &tab, &pt, nullptr, &bl, &out);
    c = cf, c.struct_size = sizeof c + 8;
    run("cashflow_struct_size_wrong", e, &tab, &pt, &c, &bl, &out);
    s = make_sim(SMMC_MODE_TABLE, 0, 100, 0);
    run("no_periods", e, &s, &pt, &cf, &bl, &out);
    s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0);
    run("too_many_periods", e, &s, &pt, &cf, &bl, &out);
    c = cf, c.floor = -1.0f;
    run("floor_negative", e, &tab, &pt, &c, &bl, &out);
    c = cf, c.floor = nan;
    run("floor_nan", e, &tab, &pt, &c, &bl, &out);
    c = cf, c.amount = inf;
    run("amount_infinite", e, &tab, &pt, &c, &bl, &out);
    c = cf, c.fraction = nan;
    run("fraction_nan", e, &tab, &pt, &c, &bl, &out);
    c = cf, c.amounts = bad_amounts.data();
    run("amounts_entry_nan", e, &tab, &pt, &c, &bl, &out);
    c = cf, c.fractions = bad_fractions.data();
    run("fractions_entry_infinite", e, &tab, &pt, &c, &bl, &out);
    // this call's own: the mode, and what the block bootstrap refuses for blocks
    run("gaussian_mode", e, &gau, &pg, &cf, &bl, &out);
    run("blocks_null", e, &tab, &pt, &cf, nullptr, &out);
    b = bl, b.struct_size = sizeof b + 4;
    run("blocks_struct_size_wrong", e, &tab, &pt, &cf, &b, &out);
    b = bl, b.block_len = 0;
    run("block_len_zero", e, &tab, &pt, &cf, &b, &out);
    b = bl, b.kind = 1;
    run("blocks_kind_unknown", e, &tab, &pt, &cf, &b, &out);
    b = bl, b.reserved = 5;
    run("blocks_reserved_not_zero", e, &tab, &pt, &cf, &b, &out);
    if (entry < 2) {
      run("outputs_null", e, &tab, &pt, &cf, &bl, nullptr);
      smmc_portfolio_cashflow_outputs o = out;
      o.struct_size = sizeof o - 8;
      run("outputs_struct_size_wrong", e, &tab, &pt, &cf, &bl, &o);
      o = out, o.reserved = 3;
      run("outputs_reserved_not_zero", e, &tab, &pt, &cf, &bl, &o);
      s = tab, s.n_paths = 1ull << 50;
      run("paths_per_workgroup", e, &s, &pt, &cf, &bl, &out);
      if (entry == 0) {
        o = out, o.d_paid = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(paid) + 2);
        run("paid_misaligned", e, &tab, &pt, &cf, &bl, &o);
        o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
        run("depleted_at_misaligned", e, &tab, &pt, &cf, &bl, &o);
      }
      // the largest table -- 4096 + 7 rows x 4 words, 4097 depletion counters and 4096 buckets, 96 KiB -- fits the 128 KiB
      // an engine assumes at the least, so the LDS refusal cannot be reached with valid arguments
      p = pt, p.n_assets = 4, p.weights[0] = p.weights[1] = p.weights[2] = p.weights[3] = 0.25f;
      s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, SMMC_MAX_BINS, 0);
      c = cf, c.amounts = steady.data();
      run("valid_largest", big, &s, &p, &c, &bl, &out);
      // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
      run("valid_table", e, &tab, &pt, &cf, &bl, &out);
      b = make_blocks(1);
      run("valid_block_len_one", e, &tab, &pt, &cf, &b, &out);
      b = make_blocks(0xffffffffu);
      run("valid_block_len_largest", e, &tab, &pt, &cf, &b, &out);
      s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_EXACT_DIV);
      run("valid_exact_div_flag", e, &s, &pt, &cf, &bl, &out);
      p = pt, p.rebalance_every = 0;
      run("valid_buy_and_hold", e, &tab, &p, &cf, &bl, &out);
      c = cf, c.amounts = steady.data(), c.fractions = steady.data();
      run("valid_varying", e, &tab, &pt, &c, &bl, &out);
      smmc_portfolio_cashflow_outputs none;
      std::memset(&none, 0, sizeof none);
      none.struct_size = sizeof none;
      run("valid_no_outputs", e, &tab, &pt, &cf, &bl, &none);
      s = tab, s.n_paths = 0;
      o = out, o.d_depleted_at = nullptr;  // tests/cpp/cashflow_launch_stub.cpp has no kernel that copies the counts out
      run("valid_no_paths", e, &s, &pt, &cf, &bl, &o);  // nothing to launch: SMMC_OK and an empty record
    }
  }

  // which divide a launch uses: what the parent's rule says of (sim, pf, cf), for every block length
  const smmc_portfolio pt = make_pf(false, 12), hold = make_pf(false, 0);
  const smmc_sim t360 = make_sim(SMMC_MODE_TABLE, 360, 0, 0), t36 = make_sim(SMMC_MODE_TABLE, 36, 0, 0);
  {
    std::vector<float> paying_in(360, -5.0f), rising(360, 3.0f);
    for (int t = 0; t < 360; ++t) rising[t] = 3.0f + 0.01f * t;
    smmc_cashflow varying_in = make_cf(0.0f, 0.0f, 0.01f), varying_out = make_cf(0.0f, 0.0f, 0.01f);
    varying_in.amounts = paying_in.data();
    varying_out.amounts = rising.data();
    smmc_engine *dbl = nullptr;
    const float doubling[4] = {100.0f, 0.2f, -2.0f, 0.4f};  // one +100 % month in column 0
    if (smmc_engine_create(0, nullptr, &dbl) != SMMC_OK || smmc_engine_set_asset_table(dbl, doubling, 2, 2) != SMMC_OK) return 1;
    struct Request {
      const char *name;
      smmc_engine *eng;
      smmc_sim s;
      smmc_portfolio p;
      smmc_cashflow c;
    };
    const Request grid[] = {{"zero_flows", e, t360, pt, make_cf(0.0f, 0.0f, 0.0f)},
                            {"contributions", e, t360, pt, make_cf(-10.0f, 0.0f, 0.0f)},
                            {"contributions_varying", e, t360, pt, varying_in},
                            {"contributions_too_large", e, t360, pt, make_cf(-1e37f, 0.0f, 0.0f)},
                            {"withdrawal_floor_rebalanced", e, t360, pt, make_cf(4.0f, 0.0f, 0.01f)},
                            {"withdrawal_no_floor_rebalanced", e, t360, pt, make_cf(4.0f, 0.0f, 0.0f)},
                            {"withdrawal_no_floor_buy_and_hold", e, t360, hold, make_cf(4.0f, 0.0f, 0.0f)},
                            {"withdrawal_tiny_floor", e, t360, pt, make_cf(4.0f, 0.0f, 1e-30f)},
                            {"fraction", e, t360, pt, make_cf(0.0f, 0.004f, 0.01f)},
                            {"varying_withdrawals", e, t360, pt, varying_out},
                            {"exact_flag", e, make_sim(SMMC_MODE_TABLE, 360, 0, SMMC_FLAG_EXACT_DIV), pt, make_cf(-10.0f, 0.0f, 0.0f)},
                            {"table_doubling_360", dbl, t360, pt, make_cf(4.0f, 0.0f, 0.01f)},
                            {"table_doubling_36", dbl, t36, pt, make_cf(4.0f, 0.0f, 0.01f)}};
    for (const Request &r : grid)
      for (uint32_t len : {1u, 3u, 12u, 360u, 5000u}) {
        const smmc_blocks b = make_blocks(len);
        std::printf("kind:%s:%u %d %d\n", r.name, len, smmc_engine_portfolio_cashflow_blocks_divide_kind(r.eng, &r.s, &r.p, &r.c, &b),
                    smmc_engine_portfolio_cashflow_divide_kind(r.eng, &r.s, &r.p, &r.c));
      }
    smmc_engine_destroy(dbl);
  }

  // the form and the block length a launch is given are what the rule and the request name; the rest of the launch's
  // arguments is what the request says
  {
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_final = finals;
    smmc_cashflow c;
    smmc_blocks b = make_blocks(12);
    int rc = smmc_engine_simulate_portfolio_cashflow_blocks(e, &t360, &pt, &(c = make_cf(4.0f, 0.0f, 0.01f)), &b, &o);
    std::printf("ran:fast %d %d %u\n", rc, fake_portfolio_cashflow_blocks_last_exact(), fake_portfolio_cashflow_blocks_last_block_len());
    b = make_blocks(77);
    rc = smmc_engine_simulate_portfolio_cashflow_blocks(e, &t360, &pt, &(c = make_cf(4.0f, 0.004f, 0.01f)), &b, &o);
    std::printf("ran:exact %d %d %u\n", rc, fake_portfolio_cashflow_blocks_last_exact(), fake_portfolio_cashflow_blocks_last_block_len());
    const smmc_sim flagged = make_sim(SMMC_MODE_TABLE, 360, 0, SMMC_FLAG_EXACT_DIV);
    rc = smmc_engine_simulate_portfolio_cashflow_blocks(e, &flagged, &pt, &(c = make_cf(4.0f, 0.0f, 0.01f)), &b, &o);
    std::printf("ran:exact_flag %d %d %u\n", rc, fake_portfolio_cashflow_blocks_last_exact(), fake_portfolio_cashflow_blocks_last_block_len());

    smmc_portfolio_cashflow_outputs all = o;
    all.d_holdings = holdings, all.d_paid = paid, all.d_ruin_period = ruin, all.d_stats = stats, all.d_depleted_at = depleted;
    const smmc_sim s = make_sim(SMMC_MODE_TABLE, 77, 32, 0);
    const smmc_portfolio p5 = make_pf(false, 5);
    b = make_blocks(9);
    rc = smmc_engine_simulate_portfolio_cashflow_blocks(e, &s, &p5, &(c = make_cf(4.0f, 0.002f, 0.5f)), &b, &all);
    const smmc::PortfolioCashflowBlocksArgs &x = *static_cast<const smmc::PortfolioCashflowBlocksArgs *>(fake_portfolio_cashflow_blocks_last_args());
    const smmc::KernelArgs &a = *static_cast<const smmc::KernelArgs *>(fake_portfolio_cashflow_blocks_last_kernel_args());
    std::printf("staged:rc %d\n", rc == SMMC_ERR_HIP ? 1 : 0);
    std::printf("staged:plan %d\n", x.block_len == 9 && x.p.n_assets == 2 && x.p.rebalance_every == 5 && x.p.weights[0] == 0.6f &&
                                        x.p.weights[1] == 0.4f && x.c.amount == 4.0f && x.c.fraction == 0.002f && x.c.floor == 0.5f && !x.c.schedule
                                    ? 1 : 0);
    std::printf("staged:sim %d\n", a.mode == SMMC_MODE_TABLE && a.table_len == 3 && a.table_a && a.n_periods == 77 && a.n_paths == 1000 &&
                                       a.n_bins == 32 && a.stream == 3 && a.initial_capital == 1000.0f
                                   ? 1 : 0);
    std::printf("staged:outputs %d\n", a.d_final == finals && x.p.d_holdings == holdings && x.c.d_paid == paid && x.c.d_ruin_period == ruin &&
                                           a.partials && a.d_hist && x.c.d_depleted && x.c.d_depleted >= a.d_hist + SMMC_MAX_BINS
                                       ? 1 : 0);
    rc = smmc_engine_simulate_portfolio_cashflow_blocks(e, &s, &p5, &(c = make_cf(4.0f, 0.002f, 0.5f)), &b, &o);
    std::printf("staged:nothing_asked %d\n", a.d_final == finals && !x.p.d_holdings && !x.c.d_paid && !x.c.d_ruin_period && !a.partials &&
                                                 !a.d_hist && !x.c.d_depleted && a.n_bins == 0
                                             ? 1 : 0);
  }

  // the accumulator lease: a call whose launch fails has taken the engine's accumulator (buckets and depletion counters)
  // and not given it back clean; the next user (a plain simulate through tests/cpp/launch_fake.cpp) must still get its
  // own buckets
  {
    smmc_engine *l = nullptr;
    const float table[3] = {1.0f, -2.0f, 0.5f};
    if (smmc_engine_create(0, nullptr, &l) != SMMC_OK || smmc_engine_set_table(l, table, 3) != SMMC_OK ||
        smmc_engine_set_asset_table(l, rows2, 3, 2) != SMMC_OK)
      return 1;
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
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_stats = stats;
    o.d_depleted_at = depleted;
    const smmc_sim g = make_sim(SMMC_MODE_TABLE, 36, 16, 0);
    const smmc_cashflow cf = make_cf(4.0f, 0.0f, 0.01f);
    const smmc_blocks b = make_blocks(12);
    const int failed = smmc_engine_simulate_portfolio_cashflow_blocks(l, &g, &pt, &cf, &b, &o);
    const int second = smmc_engine_simulate_to_host(l, &s, out.data(), nullptr, nullptr, nullptr, &st, again.data());
    std::printf("lease:after_failed_launch %d %d %d %d %d\n", first, failed, second, hist == want ? 1 : 0, again == want ? 1 : 0);
    smmc_engine_destroy(l);
  }

  std::printf("sizes %zu %zu %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_cashflow), sizeof(smmc_blocks),
              sizeof(smmc_portfolio_cashflow_outputs));
  for (smmc_engine *p : {e, no_table, three, big}) smmc_engine_destroy(p);
  std::printf("portfolio_cashflow_blocks_args: done\n");
  return 0;
}
