// glide_args.cpp -- the argument checks, the divide rule and the flattened change table of smmc_engine_simulate_glide, its
// _to_host form and smmc_engine_glide_divide_kind (include/smmc.h) without a GPU: csrc/smmc_glide.cpp and the library's
// other host units over tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before
// any device work, so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error() and without a
// launch; TEST INFRASTRUCTURE, driven by tests/test_glide_cpu.py (built with -fsanitize=address,undefined and run
// directly).  Prints one line per case: "<name> <return code> <length of the error text> <launches the call made>" and
// the text behind "#", then "staged:<what> <1: the launch got what the request says>", "divide:<what> <kind>",
// "lease:..." and "sizes ..." lines, then "glide_args: done".
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"
#include "smmc_internal.h"

extern "C" int fake_glide_launches(void);
extern "C" int fake_glide_last_exact(void);
extern "C" const void *fake_glide_last_kernel_args(void);
extern "C" const void *fake_glide_last_args(void);
extern "C" const void *fake_glide_last_table(void);
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

// 60 / 40; Gaussian fields as asked (means 0.5, 0.2; L = [[4, 0], [0.9, 1.2]]) or all zero for table mode
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

static smmc_cashflow make_cf(float amount, float floor) {
  smmc_cashflow c;
  std::memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.amount = amount;
  c.floor = floor;
  return c;
}

static smmc_glide make_gl(uint32_t n, const uint32_t *after, const float *rows) {
  smmc_glide g;
  std::memset(&g, 0, sizeof g);
  g.struct_size = sizeof g;
  g.n_changes = n;
  g.after = after;
  g.weights = rows;
  return g;
}

static void report(const char *name, int rc, int launches) {
  std::printf("%s %d %zu %d\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0), launches);
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr, *no_table = nullptr, *one = nullptr, *big = nullptr;
  for (smmc_engine **p : {&e, &no_table, &one, &big})
    if (smmc_engine_create(0, nullptr, p) != SMMC_OK) {
      std::printf("engine_create failed: %s\n", smmc_last_error());
      return 1;
    }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float rows2[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};  // 3 rows x 2 assets
  const float rows1[3] = {1.0f, -2.0f, 0.5f};                     // 3 rows x 1 asset
  if (smmc_engine_set_asset_table(e, rows2, 3, 2) != SMMC_OK) return 1;
  if (smmc_engine_set_asset_table(one, rows1, 3, 1) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);  // 8192 rows x 2 assets: 64 KiB of LDS
  if (smmc_engine_set_asset_table(big, largest.data(), SMMC_MAX_TABLE / 2, 2) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  alignas(8) static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
  static float finals[1000], holdings[4000], paid[1000];
  static uint32_t ruin[1000];

  smmc_portfolio_cashflow_outputs out;
  std::memset(&out, 0, sizeof out);
  out.struct_size = sizeof out;
  out.d_final = finals;
  out.d_holdings = holdings;
  out.d_paid = paid;
  out.d_ruin_period = ruin;
  out.d_stats = stats;
  out.d_depleted_at = depleted;

  const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 100, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
  const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
  const smmc_cashflow cf = make_cf(4.0f, 0.01f);
  // a glide from 60 / 40 to 30 / 70 in three steps, on the rebalance periods
  const uint32_t after3[3] = {120, 240, 348};
  const float rows[3 * SMMC_MAX_ASSETS] = {0.5f, 0.5f, 0, 0, 0.4f, 0.6f, 0, 0, 0.3f, 0.7f, 0, 0};
  const smmc_glide gl = make_gl(3, after3, rows);
  std::vector<uint32_t> after_most(SMMC_MAX_GLIDE_CHANGES + 1);
  std::vector<float> rows_most((SMMC_MAX_GLIDE_CHANGES + 1) * SMMC_MAX_ASSETS, 0.0f);
  for (uint32_t c = 0; c <= SMMC_MAX_GLIDE_CHANGES; ++c) {
    after_most[c] = c + 1u;
    rows_most[c * SMMC_MAX_ASSETS] = c % 2 ? 0.25f : 0.75f;
    rows_most[c * SMMC_MAX_ASSETS + 1] = c % 2 ? 0.75f : 0.25f;
  }

  for (int entry = 0; entry < 3; ++entry) {
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    char name[96];
    auto run = [&](const char *what, smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c, const smmc_glide *g,
                   const smmc_portfolio_cashflow_outputs *o) {
      const int before = fake_glide_launches() + fake_portfolio_cashflow_launches();
      const int rc = entry == 0   ? smmc_engine_simulate_glide(eng, s, p, c, g, o)
                     : entry == 1 ? smmc_engine_simulate_glide_to_host(eng, s, p, c, g, o)
                                  : smmc_engine_glide_divide_kind(eng, s, p, c, g);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_glide_launches() + fake_portfolio_cashflow_launches() - before);
    };
    smmc_portfolio p;
    smmc_cashflow c;
    smmc_glide g;
    smmc_sim s;
    uint32_t after[3];
    float w[3 * SMMC_MAX_ASSETS];
    auto fresh = [&] {
      std::memcpy(after, after3, sizeof after);
      std::memcpy(w, rows, sizeof w);
      g = make_gl(3, after, w);
    };
    // what the parent refuses for sim, pf and cf
    run("engine_null", nullptr, &gau, &pg, &cf, &gl, &out);
    run("sim_null", e, nullptr, &pg, &cf, &gl, &out);
    s = gau, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &pg, &cf, &gl, &out);
    run("portfolio_null", e, &gau, nullptr, &cf, &gl, &out);
    p = pg, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &gau, &p, &cf, &gl, &out);
    p = pg, p.weights[0] = -0.1f, p.weights[1] = 1.1f;
    run("weight_negative", e, &gau, &p, &cf, &gl, &out);
    p = pg, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &gau, &p, &cf, &gl, &out);
    run("table_mode_without_asset_table", no_table, &tab, &pt, &cf, &gl, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pt, &cf, &gl, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pg, &cf, &gl, &out);
    run("cashflow_null", e, &gau, &pg, nullptr, &gl, &out);
    c = cf, c.struct_size = sizeof c + 4;
    run("cashflow_struct_size_wrong", e, &gau, &pg, &c, &gl, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 0, 100, 0);
    run("no_periods", e, &s, &pg, &cf, &gl, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0);
    run("too_many_periods", e, &s, &pg, &cf, &gl, &out);
    c = cf, c.floor = -1.0f;
    run("floor_negative", e, &gau, &pg, &c, &gl, &out);
    c = cf, c.amount = nan;
    run("amount_nan", e, &gau, &pg, &c, &gl, &out);
    c = cf, c.fraction = inf;
    run("fraction_infinite", e, &gau, &pg, &c, &gl, &out);
    // the glide itself
    run("glide_null", e, &gau, &pg, &cf, nullptr, &out);
    g = gl, g.struct_size = sizeof g + 8;
    run("glide_struct_size_wrong", e, &gau, &pg, &cf, &g, &out);
    g = make_gl(SMMC_MAX_GLIDE_CHANGES + 1, after_most.data(), rows_most.data());
    run("too_many_changes", e, &gau, &pg, &cf, &g, &out);
    g = gl, g.after = nullptr;
    run("after_null", e, &gau, &pg, &cf, &g, &out);
    g = gl, g.weights = nullptr;
    run("weights_null", e, &gau, &pg, &cf, &g, &out);
    fresh(), after[0] = 0;
    run("after_zero", e, &gau, &pg, &cf, &g, &out);
    fresh(), after[1] = after[0];
    run("after_repeated", e, &gau, &pg, &cf, &g, &out);
    fresh(), after[2] = after[1] - 1;
    run("after_decreasing", e, &gau, &pg, &cf, &g, &out);
    fresh(), w[SMMC_MAX_ASSETS] = -0.1f, w[SMMC_MAX_ASSETS + 1] = 1.1f;
    run("row_weight_negative", e, &gau, &pg, &cf, &g, &out);
    fresh(), w[2 * SMMC_MAX_ASSETS] = nan;
    run("row_weight_nan", e, &gau, &pg, &cf, &g, &out);
    fresh(), w[1] = inf;
    run("row_weight_infinite", e, &gau, &pg, &cf, &g, &out);
    fresh(), w[0] = 0.25f, w[1] = 0.5f, w[2] = 0.25f;
    run("row_weight_beyond_the_assets", e, &gau, &pg, &cf, &g, &out);
    fresh(), w[SMMC_MAX_ASSETS + 1] = 0.6001f;
    run("row_does_not_sum_to_one", e, &gau, &pg, &cf, &g, &out);
    // a bad row beyond the last period is a bad row all the same
    s = make_sim(SMMC_MODE_GAUSSIAN, 100, 100, 0);
    fresh(), w[2 * SMMC_MAX_ASSETS] = 0.9f;
    run("row_beyond_the_plan_does_not_sum_to_one", e, &s, &pg, &cf, &g, &out);
    p = make_pf(false, 12), p.n_assets = 1, p.weights[0] = 1.0f, p.weights[1] = 0.0f;
    run("one_asset_row_not_one", one, &tab, &p, &cf, &gl, &out);
    if (entry < 2) {
      // the outputs, the launch's size
      run("outputs_null", e, &gau, &pg, &cf, &gl, nullptr);
      smmc_portfolio_cashflow_outputs o = out;
      o.struct_size = sizeof o - 8;
      run("outputs_struct_size_wrong", e, &gau, &pg, &cf, &gl, &o);
      o = out, o.reserved = 3;
      run("outputs_reserved_not_zero", e, &gau, &pg, &cf, &gl, &o);
      s = gau, s.n_paths = 1ull << 50;
      run("paths_per_workgroup", e, &s, &pg, &cf, &gl, &out);
      // 8192 rows x 2 words are 64 KiB, 4097 counters 16 KiB and 4096 buckets 16 KiB: the largest request fits, as the parent's
      s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, SMMC_MAX_BINS, 0);
      run("valid_largest_lds", big, &s, &pt, &cf, &gl, &out);
    }
    if (entry == 0) {
      smmc_portfolio_cashflow_outputs o = out;
      o.d_paid = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(paid) + 2);
      run("paid_misaligned", e, &gau, &pg, &cf, &gl, &o);
      o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
      run("depleted_at_misaligned", e, &gau, &pg, &cf, &gl, &o);
    }
    // a valid request passes every argument check; what stops a simulate here is that this build has no kernel: ONE launch
    run("valid_table", e, &tab, &pt, &cf, &gl, &out);
    run("valid_gaussian", e, &gau, &pg, &cf, &gl, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_EXACT_DIV);
    run("valid_exact_div_flag", e, &s, &pg, &cf, &gl, &out);
    g = make_gl(0, nullptr, nullptr);
    run("valid_no_changes", e, &gau, &pg, &cf, &g, &out);
    g = make_gl(SMMC_MAX_GLIDE_CHANGES, after_most.data(), rows_most.data());
    run("valid_most_changes", e, &gau, &pg, &cf, &g, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 100, 100, 0);
    run("valid_changes_beyond_the_plan", e, &s, &pg, &cf, &gl, &out);
    const uint32_t a1[1] = {1};
    const float r1[SMMC_MAX_ASSETS] = {1.0f, 0, 0, 0};
    g = make_gl(1, a1, r1);
    p = make_pf(false, 12), p.n_assets = 1, p.weights[0] = 1.0f, p.weights[1] = 0.0f;
    run("valid_one_asset", one, &tab, &p, &cf, &g, &out);
    if (entry < 2) {
      smmc_portfolio_cashflow_outputs none;
      std::memset(&none, 0, sizeof none);
      none.struct_size = sizeof none;
      run("valid_no_outputs", e, &tab, &pt, &cf, &gl, &none);
      s = gau, s.n_paths = 0;
      smmc_portfolio_cashflow_outputs o = out;
      o.d_depleted_at = nullptr;  // the stubs have no kernel that copies the counts out
      run("valid_no_paths", e, &s, &pg, &cf, &gl, &o);  // nothing to launch: SMMC_OK and an empty record
    }
  }

  // one asset: the request is checked here and launched by the parent unit
  {
    const uint32_t a1[1] = {1};
    const float r1[SMMC_MAX_ASSETS] = {1.0f, 0, 0, 0};
    const smmc_glide g = make_gl(1, a1, r1);
    smmc_portfolio p = make_pf(false, 12);
    p.n_assets = 1, p.weights[0] = 1.0f, p.weights[1] = 0.0f;
    const int glide_before = fake_glide_launches(), parent_before = fake_portfolio_cashflow_launches();
    const int rc = smmc_engine_simulate_glide(one, &tab, &p, &cf, &g, &out);
    std::printf("staged:one_asset_is_the_parents_launch %d\n",
                rc == SMMC_ERR_HIP && fake_glide_launches() == glide_before && fake_portfolio_cashflow_launches() == parent_before + 1 ? 1 : 0);
  }

  // staging: what the launch is given is what the request says
  {
    const smmc_portfolio p = make_pf(true, 5);
    const smmc_sim s = make_sim(SMMC_MODE_GAUSSIAN, 300, 32, 0);  // the third change (348) lies beyond the plan
    const smmc::GlideArgs &x = *static_cast<const smmc::GlideArgs *>(fake_glide_last_args());
    const smmc::KernelArgs &a = *static_cast<const smmc::KernelArgs *>(fake_glide_last_kernel_args());
    const smmc::GlideEntry *t = static_cast<const smmc::GlideEntry *>(fake_glide_last_table());
    auto zero_entry = [](const smmc::GlideEntry &en) {
      static const smmc::GlideEntry z = {};
      return std::memcmp(&en, &z, sizeof z) == 0;
    };
    const int rc = smmc_engine_simulate_glide(e, &s, &p, &cf, &gl, &out);
    std::printf("staged:rc %d\n", rc == SMMC_ERR_HIP ? 1 : 0);
    std::printf("staged:portfolio %d\n", x.p.n_assets == 2 && x.p.rebalance_every == 5 && x.p.weights[0] == 0.6f && x.p.weights[1] == 0.4f &&
                                             x.p.shift100[0] == 100.5f && x.p.factor[SMMC_MAX_ASSETS] == 0.9f
                                         ? 1 : 0);
    std::printf("staged:schedule %d\n", x.c.amount == 4.0f && x.c.fraction == 0.0f && x.c.floor == 0.01f && !x.c.schedule ? 1 : 0);
    std::printf("staged:sim %d\n", a.n_periods == 300 && a.n_paths == 1000 && a.n_bins == 32 && a.stream == 3 && a.initial_capital == 1000.0f ? 1 : 0);
    std::printf("staged:outputs %d\n", a.d_final == finals && x.p.d_holdings == holdings && x.c.d_paid == paid && x.c.d_ruin_period == ruin &&
                                           x.c.d_depleted && a.d_hist && x.c.d_depleted >= a.d_hist + SMMC_MAX_BINS && a.partials
                                       ? 1 : 0);
    // two changes inside the plan: 120 periods to the first, 120 more to the second, none behind it; then the zero entry
    std::printf("staged:table_changes_beyond_the_plan %d\n",
                x.first == 120 && x.table && reinterpret_cast<uintptr_t>(x.table) % 32 == 0 && t[0].next == 120 && t[0].weights[0] == 0.5f &&
                        t[0].weights[1] == 0.5f && t[0].weights[2] == 0.0f && t[0].pad[0] == 0 && t[1].next == 0 && t[1].weights[0] == 0.4f &&
                        t[1].weights[1] == 0.6f && zero_entry(t[2])
                    ? 1 : 0);
    // every change beyond the plan, and none at all: the countdown never starts and the table is the zero entry
    const smmc_sim brief = make_sim(SMMC_MODE_GAUSSIAN, 100, 32, 0);
    (void)smmc_engine_simulate_glide(e, &brief, &p, &cf, &gl, &out);
    const bool all_beyond = x.first == 0 && x.table && zero_entry(t[0]);
    const smmc_glide none = make_gl(0, nullptr, nullptr);
    (void)smmc_engine_simulate_glide(e, &brief, &p, &cf, &none, &out);
    std::printf("staged:table_without_a_change %d\n", all_beyond && x.first == 0 && x.table && zero_entry(t[0]) ? 1 : 0);
    // a change after period 1 and one after the last period
    const uint32_t ends[2] = {1, 100};
    const smmc_glide at_ends = make_gl(2, ends, rows);
    (void)smmc_engine_simulate_glide(e, &brief, &p, &cf, &at_ends, &out);
    std::printf("staged:table_change_at_1_and_at_the_last_period %d\n",
                x.first == 1 && t[0].next == 99 && t[0].weights[0] == 0.5f && t[1].next == 0 && t[1].weights[1] == 0.6f && zero_entry(t[2]) ? 1 : 0);
    // 512 changes after the periods 1 .. 512 of a plan of 9: nine entries and the zero entry; of a plan of 600: all of them
    const smmc_glide most = make_gl(SMMC_MAX_GLIDE_CHANGES, after_most.data(), rows_most.data());
    const smmc_sim nine = make_sim(SMMC_MODE_GAUSSIAN, 9, 32, 0);
    (void)smmc_engine_simulate_glide(e, &nine, &p, &cf, &most, &out);
    bool ok = x.first == 1 && zero_entry(t[9]);
    for (uint32_t c = 0; c < 9; ++c) ok = ok && t[c].next == (c < 8 ? 1u : 0u) && t[c].weights[0] == (c % 2 ? 0.25f : 0.75f) && t[c].weights[1] == (c % 2 ? 0.75f : 0.25f);
    std::printf("staged:table_most_changes_short_plan %d\n", ok ? 1 : 0);
    const smmc_sim long_plan = make_sim(SMMC_MODE_GAUSSIAN, 600, 32, 0);
    (void)smmc_engine_simulate_glide(e, &long_plan, &p, &cf, &most, &out);
    ok = x.first == 1 && zero_entry(t[SMMC_MAX_GLIDE_CHANGES]);
    for (uint32_t c = 0; c < SMMC_MAX_GLIDE_CHANGES; ++c) ok = ok && t[c].next == (c + 1 < SMMC_MAX_GLIDE_CHANGES ? 1u : 0u) && t[c].weights[0] == (c % 2 ? 0.25f : 0.75f);
    std::printf("staged:table_most_changes %d\n", ok ? 1 : 0);
    // a per-period schedule is staged beside the table
    std::vector<float> amounts(300, -1.0f);
    smmc_cashflow varying = make_cf(0.0f, 0.01f);
    varying.amounts = amounts.data();
    (void)smmc_engine_simulate_glide(e, &s, &p, &varying, &gl, &out);
    std::printf("staged:varying_schedule %d\n", x.c.schedule && x.c.stride == 304 && x.c.schedule[0] == -1.0f && x.c.schedule[299] == -1.0f &&
                                                    x.c.schedule[300] == 0.0f && x.first == 120 && t[0].next == 120
                                                ? 1 : 0);
    // without the record and the counts nothing of the accumulator is handed out, and n_bins is 0 for the kernel
    smmc_portfolio_cashflow_outputs few;
    std::memset(&few, 0, sizeof few);
    few.struct_size = sizeof few;
    few.d_final = finals;
    (void)smmc_engine_simulate_glide(e, &s, &p, &cf, &gl, &few);
    std::printf("staged:nothing_asked %d\n", !x.c.d_depleted && !a.d_hist && !a.partials && a.n_bins == 0 && !x.c.d_paid && a.d_final == finals ? 1 : 0);
  }

  // the divide rule's decisions (SMMC_DIV_FAST 0, SMMC_DIV_EXACT 1) and what the launch is told, on the tame table: three months
  // within +-2 %, so 360 periods move a holding by fewer than 11 bits and the parent's answer for 60 / 40 is FAST
  {
    auto kind = [&](const char *what, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c, const smmc_glide *g) {
      const int k = smmc_engine_glide_divide_kind(e, s, p, c, g);
      const int parent = smmc_engine_portfolio_cashflow_divide_kind(e, s, p, c);
      (void)smmc_engine_simulate_glide(e, s, p, c, g, &out);
      std::printf("divide:%s %d %d %d\n", what, k, parent, fake_glide_last_exact());
    };
    const smmc_glide none = make_gl(0, nullptr, nullptr);
    kind("no_changes", &tab, &pt, &cf, &none);                  // the parent's answer: FAST
    kind("positive_rows", &tab, &pt, &cf, &gl);                 // FAST
    smmc_sim s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_EXACT_DIV);
    kind("flag", &s, &pt, &cf, &gl);                            // EXACT
    const uint32_t a2[2] = {100, 200};
    const float to_zero[2 * SMMC_MAX_ASSETS] = {0.0f, 1.0f, 0, 0, 0.5f, 0.5f, 0, 0};
    const smmc_glide z = make_gl(2, a2, to_zero);
    kind("an_asset_to_zero_and_back", &tab, &pt, &cf, &z);      // EXACT: the positively weighted set changes
    const float beyond_zero[2 * SMMC_MAX_ASSETS] = {0.5f, 0.5f, 0, 0, 1.0f, 0.0f, 0, 0};
    const uint32_t a_far[2] = {100, 5000};
    const smmc_glide zb = make_gl(2, a_far, beyond_zero);
    kind("a_zero_beyond_the_plan", &tab, &pt, &cf, &zb);        // EXACT: every row counts
    smmc_portfolio p = make_pf(false, 12);
    p.weights[0] = 1.0f, p.weights[1] = 0.0f;
    const float stays[SMMC_MAX_ASSETS] = {1.0f, 0.0f, 0, 0};
    const smmc_glide same_set = make_gl(1, a2, stays);
    kind("the_same_asset_unweighted_throughout", &tab, &p, &cf, &same_set);  // FAST: the set is the same
    const float tiny_row[SMMC_MAX_ASSETS] = {1.0f - 1e-7f, 1e-30f, 0, 0};
    const smmc_glide tiny = make_gl(1, a2, tiny_row);
    kind("a_tiny_positive_weight", &tab, &pt, &cf, &tiny);      // EXACT: its share of the amount and of the floor is too small
    smmc_cashflow c = make_cf(4.0f, 0.0f);
    kind("rebalanced_without_a_floor", &tab, &pt, &c, &gl);     // EXACT, as the parent
    c = make_cf(0.0f, 0.01f), c.fraction = 0.01f;
    kind("a_fraction", &tab, &pt, &c, &gl);                     // EXACT, as the parent
    c = make_cf(-4.0f, 0.0f);
    kind("contributions", &tab, &pt, &c, &gl);                  // FAST
    kind("contributions_with_a_tiny_weight", &tab, &pt, &c, &tiny);  // EXACT: 1000 * 1e-30 is below 2^-89 before it shrinks
  }

  // the accumulator lease: a call whose launch fails has taken the engine's accumulator and not given it back clean; the
  // next user (a plain simulate through tests/cpp/launch_fake.cpp) must still get its own buckets
  {
    smmc_engine *l = nullptr;
    const float table[3] = {1.0f, -2.0f, 0.5f};
    if (smmc_engine_create(0, nullptr, &l) != SMMC_OK || smmc_engine_set_table(l, table, 3) != SMMC_OK) return 1;
    smmc_sim s = make_sim(SMMC_MODE_TABLE, 36, 16, 0);
    s.n_paths = 5000;
    s.hist_lo = 400.0f;
    s.hist_hi = 2100.0f;
    std::vector<float> values(s.n_paths);
    std::vector<uint64_t> hist(16), again(16), want(16, 0);
    smmc_stats st;
    for (uint64_t i = 0; i < s.n_paths; ++i) {
      const float v = fake_path_value(i, 7, 0, 36, 1000.0f);
      if (v >= s.hist_lo && v < s.hist_hi) want[std::min<int>(15, static_cast<int>((static_cast<double>(v) - 400.0) * (16.0 / 1700.0)))] += 1;
    }
    const int first = smmc_engine_simulate_to_host(l, &s, values.data(), nullptr, nullptr, nullptr, &st, hist.data());
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_stats = stats;
    o.d_depleted_at = depleted;
    const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 36, 16, 0);
    const int failed = smmc_engine_simulate_glide(l, &g, &pg, &cf, &gl, &o);
    const int second = smmc_engine_simulate_to_host(l, &s, values.data(), nullptr, nullptr, nullptr, &st, again.data());
    std::printf("lease:after_failed_launch %d %d %d %d %d\n", first, failed, second, hist == want ? 1 : 0, again == want ? 1 : 0);
    smmc_engine_destroy(l);
  }

  std::printf("sizes %zu %zu %zu\n", sizeof(smmc_glide), sizeof(smmc::GlideEntry), sizeof(smmc_portfolio_cashflow_outputs));
  for (smmc_engine *p : {e, no_table, one, big}) smmc_engine_destroy(p);
  std::printf("glide_args: done\n");
  return 0;
}
