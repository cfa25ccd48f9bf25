// guardrails_args.cpp -- the argument checks and the staging of smmc_engine_simulate_guardrails and its _to_host form
// (include/smmc.h) without a GPU: csrc/smmc_guardrails.cpp and the library's other host units over tests/cpp/fake_hip.cpp,
// tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any device work, so each bad request must
// come back as SMMC_ERR_INVALID with a text in smmc_last_error() and without a launch; TEST INFRASTRUCTURE, driven by
// tests/test_guardrails_cpu.py (built with -fsanitize=address,undefined and run directly).  Prints one line per case:
// "<name> <return code> <length of the error text> <launches the call made>" and the text behind "#", then
// "staged:<what> <1: the launch got what the request says>", "lease:..." and "sizes ..." lines, then
// "guardrails_args: done".
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"
#include "smmc_internal.h"

extern "C" int fake_guardrails_launches(void);
extern "C" const void *fake_guardrails_last_kernel_args(void);
extern "C" const void *fake_guardrails_last_args(void);
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

// "4 a year of 1000, indexed by 2 %, cut by 10 % above 6 %, raised by 10 % below 3 %, between 2 and 8"
static smmc_guardrails make_gr() {
  smmc_guardrails g;
  std::memset(&g, 0, sizeof g);
  g.struct_size = sizeof g;
  g.review_every = 12;
  g.amount = 4.0f;
  g.index = 1.02f;
  g.upper = 0.006f;
  g.lower = 0.003f;
  g.cut = 0.9f;
  g.raise = 1.1f;
  g.amount_min = 2.0f;
  g.amount_max = 8.0f;
  g.floor = 0.01f;
  return g;
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
  const float rows2[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};                     // 3 rows x 2 assets
  const float rows3[9] = {1.0f, 0.2f, 0.3f, -2.0f, 0.4f, 0.2f, 0.5f, -0.3f, -0.1f};  // 3 rows x 3 assets
  if (smmc_engine_set_asset_table(e, rows2, 3, 2) != SMMC_OK) return 1;
  if (smmc_engine_set_asset_table(three, rows3, 3, 3) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);  // 8192 rows x 2 assets: 64 KiB of LDS
  if (smmc_engine_set_asset_table(big, largest.data(), SMMC_MAX_TABLE / 2, 2) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  alignas(8) static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2], cuts_at[SMMC_MAX_CASHFLOW_PERIODS + 2],
      raises_at[SMMC_MAX_CASHFLOW_PERIODS + 2];
  static float finals[1000], holdings[4000], paid[1000], last[1000], lowest[1000];
  static uint32_t ruin[1000], cuts[1000], raises[1000];

  smmc_guardrails_outputs out;
  std::memset(&out, 0, sizeof out);
  out.struct_size = sizeof out;
  out.d_final = finals;
  out.d_holdings = holdings;
  out.d_paid = paid;
  out.d_ruin_period = ruin;
  out.d_stats = stats;
  out.d_depleted_at = depleted;
  out.d_amount_last = last;
  out.d_amount_lowest = lowest;
  out.d_cuts = cuts;
  out.d_raises = raises;
  out.d_cuts_at = cuts_at;
  out.d_raises_at = raises_at;

  const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 100, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
  const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
  const smmc_guardrails gr = make_gr();

  for (int entry = 0; entry < 2; ++entry) {
    const char *tag = entry == 0 ? "device" : "to_host";
    char name[96];
    auto run = [&](const char *what, smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_guardrails *g,
                   const smmc_guardrails_outputs *o) {
      const int before = fake_guardrails_launches();
      const int rc = entry == 0 ? smmc_engine_simulate_guardrails(eng, s, p, g, o) : smmc_engine_simulate_guardrails_to_host(eng, s, p, g, o);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_guardrails_launches() - before);
    };
    smmc_portfolio p;
    smmc_guardrails g;
    smmc_sim s;
    // what the portfolio call refuses for sim and pf
    run("engine_null", nullptr, &gau, &pg, &gr, &out);
    run("sim_null", e, nullptr, &pg, &gr, &out);
    s = gau, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &pg, &gr, &out);
    run("portfolio_null", e, &gau, nullptr, &gr, &out);
    p = pg, p.struct_size = sizeof p + 4;
    run("portfolio_struct_size_wrong", e, &gau, &p, &gr, &out);
    p = pg, p.n_assets = 0;
    run("no_assets", e, &gau, &p, &gr, &out);
    p = pg, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &gau, &p, &gr, &out);
    p = pg, p.reserved = 1;
    run("reserved_not_zero", e, &gau, &p, &gr, &out);
    p = pg, p.weights[0] = -0.1f, p.weights[1] = 1.1f;
    run("weight_negative", e, &gau, &p, &gr, &out);
    p = pg, p.weights[0] = nan;
    run("weight_nan", e, &gau, &p, &gr, &out);
    p = pg, p.weights[0] = 0.5f, p.weights[1] = 0.3f, p.weights[2] = 0.2f;
    run("weight_beyond_the_assets", e, &gau, &p, &gr, &out);
    p = pg, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &gau, &p, &gr, &out);
    run("table_mode_without_asset_table", no_table, &tab, &pt, &gr, &out);
    run("asset_table_of_other_width", three, &tab, &pt, &gr, &out);
    run("gaussian_fields_in_table_mode", e, &tab, &pg, &gr, &out);
    p = pg, p.means[1] = nan;
    run("mean_nan", e, &gau, &p, &gr, &out);
    p = pg, p.factor[1] = 0.5f;
    run("factor_above_diagonal", e, &gau, &p, &gr, &out);
    p = pg, p.factor[SMMC_MAX_ASSETS + 1] = -1.2f;
    run("diagonal_negative", e, &gau, &p, &gr, &out);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pt, &gr, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pg, &gr, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &pg, &gr, &out);
    s = gau, s.mode = 7;
    run("unknown_mode", e, &s, &pg, &gr, &out);
    // the rule itself
    run("guardrails_null", e, &gau, &pg, nullptr, &out);
    g = gr, g.struct_size = sizeof g + 4;
    run("guardrails_struct_size_wrong", e, &gau, &pg, &g, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 0, 100, 0);
    run("no_periods", e, &s, &pg, &gr, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0);
    run("too_many_periods", e, &s, &pg, &gr, &out);
    g = gr, g.amount = 0.0f, g.amount_min = 0.0f;
    run("amount_zero", e, &gau, &pg, &g, &out);
    g = gr, g.amount = -4.0f;
    run("amount_negative", e, &gau, &pg, &g, &out);
    g = gr, g.amount = nan;
    run("amount_nan", e, &gau, &pg, &g, &out);
    g = gr, g.amount = inf, g.amount_max = inf;
    run("amount_infinite", e, &gau, &pg, &g, &out);
    g = gr, g.index = 0.0f;
    run("index_zero", e, &gau, &pg, &g, &out);
    g = gr, g.index = inf;
    run("index_infinite", e, &gau, &pg, &g, &out);
    g = gr, g.index = nan;
    run("index_nan", e, &gau, &pg, &g, &out);
    g = gr, g.lower = -0.001f;
    run("lower_negative", e, &gau, &pg, &g, &out);
    g = gr, g.lower = 0.007f;
    run("lower_above_upper", e, &gau, &pg, &g, &out);
    g = gr, g.upper = nan;
    run("upper_nan", e, &gau, &pg, &g, &out);
    g = gr, g.lower = nan;
    run("lower_nan", e, &gau, &pg, &g, &out);
    g = gr, g.cut = 0.0f;
    run("cut_zero", e, &gau, &pg, &g, &out);
    g = gr, g.cut = 1.01f;
    run("cut_above_one", e, &gau, &pg, &g, &out);
    g = gr, g.cut = nan;
    run("cut_nan", e, &gau, &pg, &g, &out);
    g = gr, g.raise = 0.99f;
    run("raise_below_one", e, &gau, &pg, &g, &out);
    g = gr, g.raise = inf;
    run("raise_infinite", e, &gau, &pg, &g, &out);
    g = gr, g.raise = nan;
    run("raise_nan", e, &gau, &pg, &g, &out);
    g = gr, g.amount_min = -1.0f;
    run("amount_min_negative", e, &gau, &pg, &g, &out);
    g = gr, g.amount_min = 4.5f;
    run("amount_min_above_amount", e, &gau, &pg, &g, &out);
    g = gr, g.amount_max = 3.5f;
    run("amount_max_below_amount", e, &gau, &pg, &g, &out);
    g = gr, g.amount_min = nan;
    run("amount_min_nan", e, &gau, &pg, &g, &out);
    g = gr, g.amount_max = nan;
    run("amount_max_nan", e, &gau, &pg, &g, &out);
    g = gr, g.floor = -1.0f;
    run("floor_negative", e, &gau, &pg, &g, &out);
    g = gr, g.floor = inf;
    run("floor_infinite", e, &gau, &pg, &g, &out);
    g = gr, g.floor = nan;
    run("floor_nan", e, &gau, &pg, &g, &out);
    // the outputs, the launch's size
    run("outputs_null", e, &gau, &pg, &gr, nullptr);
    smmc_guardrails_outputs o = out;
    o.struct_size = sizeof o - 8;
    run("outputs_struct_size_wrong", e, &gau, &pg, &gr, &o);
    o = out, o.reserved = 3;
    run("outputs_reserved_not_zero", e, &gau, &pg, &gr, &o);
    s = gau, s.n_paths = 1ull << 50;
    run("paths_per_workgroup", e, &s, &pg, &gr, &out);
    // 8192 rows x 2 words are 64 KiB, three arrays of 4097 counters 48 KiB and 4096 buckets 16 KiB: beyond the 128 KiB
    // an engine assumes at the least, less the 2 KiB the runtime may keep
    s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, SMMC_MAX_BINS, 0);
    run("lds_too_large", big, &s, &pt, &gr, &out);
    if (entry == 0) {
      o = out, o.d_amount_last = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(last) + 2);
      run("amount_last_misaligned", e, &gau, &pg, &gr, &o);
      o = out, o.d_cuts = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(cuts) + 1);
      run("cuts_misaligned", e, &gau, &pg, &gr, &o);
      o = out, o.d_paid = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(paid) + 2);
      run("paid_misaligned", e, &gau, &pg, &gr, &o);
      o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
      run("depleted_at_misaligned", e, &gau, &pg, &gr, &o);
      o = out, o.d_raises_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(raises_at) + 4);
      run("raises_at_misaligned", e, &gau, &pg, &gr, &o);
    }
    // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
    run("valid_table", e, &tab, &pt, &gr, &out);
    run("valid_gaussian", e, &gau, &pg, &gr, &out);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_EXACT_DIV);
    run("valid_exact_div_flag", e, &s, &pg, &gr, &out);
    g = gr, g.review_every = 0;
    run("valid_never_reviewed", e, &gau, &pg, &g, &out);
    g = gr, g.upper = inf, g.lower = 0.0f, g.amount_min = 0.0f, g.amount_max = inf, g.cut = 1.0f, g.raise = 1.0f, g.index = 1.0f, g.floor = 0.0f;
    run("valid_open_bounds", e, &gau, &pg, &g, &out);
    g = gr, g.amount_min = g.amount_max = g.amount, g.lower = g.upper;
    run("valid_shut_bounds", e, &gau, &pg, &g, &out);
    s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, 100, 0);
    run("valid_most_periods", e, &s, &pt, &gr, &out);
    smmc_guardrails_outputs none;
    std::memset(&none, 0, sizeof none);
    none.struct_size = sizeof none;
    run("valid_no_outputs", e, &tab, &pt, &gr, &none);
    s = gau, s.n_paths = 0;
    o = out, o.d_depleted_at = o.d_cuts_at = o.d_raises_at = nullptr;  // the stubs have no kernel that copies the counts out
    run("valid_no_paths", e, &s, &pg, &gr, &o);  // nothing to launch: SMMC_OK and an empty record
  }

  // staging: what the launch is given is what the request says
  {
    smmc_guardrails g = gr;
    g.review_every = 7;
    smmc_portfolio p = make_pf(true, 5);
    const smmc_sim s = make_sim(SMMC_MODE_GAUSSIAN, 77, 32, 0);
    const int rc = smmc_engine_simulate_guardrails(e, &s, &p, &g, &out);
    const smmc::GuardrailsArgs &x = *static_cast<const smmc::GuardrailsArgs *>(fake_guardrails_last_args());
    const smmc::KernelArgs &a = *static_cast<const smmc::KernelArgs *>(fake_guardrails_last_kernel_args());
    std::printf("staged:rc %d\n", rc == SMMC_ERR_HIP ? 1 : 0);
    std::printf("staged:rule %d\n", x.review_every == 7 && x.amount == g.amount && x.index == g.index && x.upper == g.upper && x.lower == g.lower &&
                                        x.cut == g.cut && x.raise == g.raise && x.amount_min == g.amount_min && x.amount_max == g.amount_max &&
                                        x.floor == g.floor
                                    ? 1 : 0);
    std::printf("staged:portfolio %d\n", x.p.n_assets == 2 && x.p.rebalance_every == 5 && x.p.weights[0] == 0.6f && x.p.weights[1] == 0.4f &&
                                             x.p.shift100[0] == 100.5f && x.p.factor[SMMC_MAX_ASSETS] == 0.9f
                                         ? 1 : 0);
    std::printf("staged:sim %d\n", a.n_periods == 77 && a.n_paths == 1000 && a.n_bins == 32 && a.stream == 3 && a.initial_capital == 1000.0f ? 1 : 0);
    std::printf("staged:per_path %d\n", a.d_final == finals && x.p.d_holdings == holdings && x.d_paid == paid && x.d_ruin_period == ruin &&
                                            x.d_amount_last == last && x.d_amount_lowest == lowest && x.d_cuts == cuts && x.d_raises == raises
                                        ? 1 : 0);
    // the three count arrays lie apart in the engine's accumulator, behind the buckets, each with room for the most periods
    const unsigned long long *dep = x.d_depleted, *cu = x.d_cuts_at, *ra = x.d_raises_at;
    std::printf("staged:counts %d\n", dep && cu && ra && a.d_hist && dep >= a.d_hist + SMMC_MAX_BINS && cu >= dep + SMMC_MAX_CASHFLOW_PERIODS + 1 &&
                                          ra >= cu + SMMC_MAX_CASHFLOW_PERIODS + 1 && a.partials
                                      ? 1 : 0);
    // without the record and the counts nothing of the accumulator is handed out, and n_bins is 0 for the kernel
    smmc_guardrails_outputs few;
    std::memset(&few, 0, sizeof few);
    few.struct_size = sizeof few;
    few.d_final = finals;
    (void)smmc_engine_simulate_guardrails(e, &s, &p, &g, &few);
    std::printf("staged:nothing_asked %d\n", !x.d_depleted && !x.d_cuts_at && !x.d_raises_at && !a.d_hist && !a.partials && a.n_bins == 0 &&
                                                 !x.d_paid && !x.d_cuts && a.d_final == finals
                                             ? 1 : 0);
    few.d_cuts_at = cuts_at;
    (void)smmc_engine_simulate_guardrails(e, &s, &p, &g, &few);
    std::printf("staged:one_count_array %d\n", !x.d_depleted && x.d_cuts_at && !x.d_raises_at && !a.d_hist ? 1 : 0);
  }

  // the accumulator lease: a call whose launch fails has taken the engine's accumulator (buckets and the three count
  // arrays) and not given it back clean; the next user (a plain simulate through tests/cpp/launch_fake.cpp) must still
  // get its own buckets
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
    smmc_guardrails_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_stats = stats;
    o.d_depleted_at = depleted;
    o.d_cuts_at = cuts_at;
    o.d_raises_at = raises_at;
    const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 36, 16, 0);
    const int failed = smmc_engine_simulate_guardrails(l, &g, &pg, &gr, &o);
    const int second = smmc_engine_simulate_to_host(l, &s, values.data(), nullptr, nullptr, nullptr, &st, again.data());
    std::printf("lease:after_failed_launch %d %d %d %d %d\n", first, failed, second, hist == want ? 1 : 0, again == want ? 1 : 0);
    smmc_engine_destroy(l);
  }

  std::printf("sizes %zu %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_guardrails), sizeof(smmc_guardrails_outputs));
  for (smmc_engine *p : {e, no_table, three, big}) smmc_engine_destroy(p);
  std::printf("guardrails_args: done\n");
  return 0;
}
