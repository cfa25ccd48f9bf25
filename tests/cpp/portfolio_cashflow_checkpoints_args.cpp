// portfolio_cashflow_checkpoints_args.cpp -- the argument checks, budgets and host protocol of
// smmc_engine_simulate_portfolio_cashflow_checkpoints and its _to_host form (include/smmc.h) without a GPU:
// csrc/smmc_portfolio_cashflow_checkpoints.cpp and the library's other host units over tests/cpp/fake_hip.cpp,
// tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any device work, so each bad request must come
// back as SMMC_ERR_INVALID with a text in smmc_last_error() and without a launch; TEST INFRASTRUCTURE, driven by
// tests/test_portfolio_cashflow_checkpoints_cpu.py (built with -fsanitize=address,undefined and run directly).  Prints
// one line per case: "<name> <return code> <length of the error text> <launches the call made>" and the text behind "#",
// then "ran:...", "empty:...", "lease:...", "grow:..." and "sizes ..." lines, then
// "portfolio_cashflow_checkpoints_args: done".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "smmc.h"

extern "C" int fake_pfcf_checkpoints_launches(void);
extern "C" int fake_pfcf_checkpoints_last_exact(void);
extern "C" int fake_pfcf_checkpoints_folds(void);
extern "C" uint32_t fake_pfcf_checkpoints_last_n(void);
extern "C" uint32_t fake_pfcf_checkpoints_last_first_period(void);
extern "C" uint32_t fake_pfcf_checkpoints_last_padding(void);
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

static void report(const char *name, int rc, int launches) {
  std::printf("%s %d %zu %d\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0), launches);
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr, *no_table = nullptr, *big = nullptr;
  for (smmc_engine **p : {&e, &no_table, &big})
    if (smmc_engine_create(0, nullptr, p) != SMMC_OK) {
      std::printf("engine_create failed: %s\n", smmc_last_error());
      return 1;
    }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float rows2[6] = {1.0f, 0.2f, -2.0f, 0.4f, 0.5f, -0.3f};  // 3 rows x 2 assets
  if (smmc_engine_set_asset_table(e, rows2, 3, 2) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);  // 4096 rows x 4 assets: 64 KiB of LDS
  if (smmc_engine_set_asset_table(big, largest.data(), SMMC_MAX_TABLE / 4, 4) != SMMC_OK) return 1;
  const size_t record_max = 64 + 8 * 4096;
  alignas(8) static unsigned char stats[64 + 8 * 4096];
  alignas(8) static unsigned char records[SMMC_MAX_CHECKPOINTS * (64 + 8 * 128) + 2 * (64 + 8 * 4096)];
  alignas(8) static uint64_t depleted[SMMC_MAX_CASHFLOW_PERIODS + 2];
  static float finals[1000], holdings[4000], paid[1000];
  static uint32_t ruin[1000];
  static_assert(sizeof records >= 2 * record_max, "two records of the largest kind fit");
  std::vector<float> steady(SMMC_MAX_CASHFLOW_PERIODS, 3.0f), bad_amounts(360, 3.0f);
  bad_amounts[200] = nan;
  uint32_t yearly[30], all64[SMMC_MAX_CHECKPOINTS + 1];
  for (uint32_t k = 0; k < 30; ++k) yearly[k] = 12 * (k + 1);
  for (uint32_t k = 0; k <= SMMC_MAX_CHECKPOINTS; ++k) all64[k] = k + 1;

  for (int entry = 0; entry < 2; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim *s, const smmc_portfolio *p, const smmc_cashflow *c, const uint32_t *per,
                    uint32_t n, const smmc_portfolio_cashflow_outputs *o, void *rec) {
      return entry == 0 ? smmc_engine_simulate_portfolio_cashflow_checkpoints(eng, s, p, c, per, n, o, rec)
                        : smmc_engine_simulate_portfolio_cashflow_checkpoints_to_host(eng, s, p, c, per, n, o, rec);
    };
    const char *tag = entry == 0 ? "device" : "to_host";
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
                   const uint32_t *per, uint32_t n, const smmc_portfolio_cashflow_outputs *o, void *rec) {
      const int before = fake_pfcf_checkpoints_launches();
      const int rc = call(eng, s, p, c, per, n, o, rec);
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc, fake_pfcf_checkpoints_launches() - before);
    };
    const smmc_sim tab = make_sim(SMMC_MODE_TABLE, 360, 100, 0), gau = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
    const smmc_cashflow cf = make_cf(3.0f, 0.001f, 0.01f);
    smmc_portfolio p;
    smmc_cashflow c;
    smmc_sim s;
    // what the parent call refuses: the portfolio's checks, the schedule's, the outputs structure's, the grid's
    run("engine_null", nullptr, &gau, &pg, &cf, yearly, 30, &out, records);
    run("sim_null", e, nullptr, &pg, &cf, yearly, 30, &out, records);
    s = gau, s.struct_size = sizeof s - 4;
    run("sim_struct_size_wrong", e, &s, &pg, &cf, yearly, 30, &out, records);
    run("portfolio_null", e, &gau, nullptr, &cf, yearly, 30, &out, records);
    p = pg, p.n_assets = SMMC_MAX_ASSETS + 1;
    run("five_assets", e, &gau, &p, &cf, yearly, 30, &out, records);
    p = pg, p.weights[1] = 0.4001f;
    run("weights_do_not_sum_to_one", e, &gau, &p, &cf, yearly, 30, &out, records);
    run("table_mode_without_asset_table", no_table, &tab, &pt, &cf, yearly, 30, &out, records);
    run("gaussian_fields_in_table_mode", e, &tab, &pg, &cf, yearly, 30, &out, records);
    p = pg, p.factor[1] = 0.5f;
    run("factor_above_diagonal", e, &gau, &p, &cf, yearly, 30, &out, records);
    s = make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF);
    run("stream_ref", e, &s, &pt, &cf, yearly, 30, &out, records);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2);
    run("stream_v2", e, &s, &pg, &cf, yearly, 30, &out, records);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0);
    run("n_bins_above_max", e, &s, &pg, &cf, yearly, 1, &out, records);
    run("cashflow_null", e, &gau, &pg, nullptr, yearly, 30, &out, records);
    c = cf, c.struct_size = sizeof c + 8;
    run("cashflow_struct_size_wrong", e, &gau, &pg, &c, yearly, 30, &out, records);
    s = make_sim(SMMC_MODE_GAUSSIAN, 0, 100, 0);
    run("no_periods", e, &s, &pg, &cf, yearly, 30, &out, records);
    s = make_sim(SMMC_MODE_GAUSSIAN, SMMC_MAX_CASHFLOW_PERIODS + 1, 100, 0);
    run("too_many_periods", e, &s, &pg, &cf, yearly, 30, &out, records);
    c = cf, c.floor = -1.0f;
    run("floor_negative", e, &gau, &pg, &c, yearly, 30, &out, records);
    c = cf, c.amount = inf;
    run("amount_infinite", e, &gau, &pg, &c, yearly, 30, &out, records);
    c = cf, c.amounts = bad_amounts.data();
    run("amounts_entry_nan", e, &gau, &pg, &c, yearly, 30, &out, records);
    run("outputs_null", e, &gau, &pg, &cf, yearly, 30, nullptr, records);
    smmc_portfolio_cashflow_outputs o = out;
    o.struct_size = sizeof o - 8;
    run("outputs_struct_size_wrong", e, &gau, &pg, &cf, yearly, 30, &o, records);
    o = out, o.reserved = 3;
    run("outputs_reserved_not_zero", e, &gau, &pg, &cf, yearly, 30, &o, records);
    s = gau, s.n_paths = 1ull << 50;
    run("paths_per_workgroup", e, &s, &pg, &cf, yearly, 30, &out, records);
    // what smmc_engine_simulate_checkpoints refuses about the checkpoint arguments
    run("periods_null", e, &gau, &pg, &cf, nullptr, 30, &out, records);
    run("records_null", e, &gau, &pg, &cf, yearly, 30, &out, nullptr);
    run("no_checkpoints", e, &gau, &pg, &cf, yearly, 0, &out, records);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
    run("too_many_checkpoints", e, &s, &pg, &cf, all64, SMMC_MAX_CHECKPOINTS + 1, &out, records);
    uint32_t per[4] = {12, 0, 36, 48};
    run("period_zero", e, &gau, &pg, &cf, per, 4, &out, records);
    per[1] = 361;
    run("period_above_n_periods", e, &gau, &pg, &cf, per, 2, &out, records);
    per[1] = 12;
    run("periods_not_increasing", e, &gau, &pg, &cf, per, 4, &out, records);
    per[1] = 40;
    run("periods_decreasing", e, &gau, &pg, &cf, per, 4, &out, records);
    // the two budgets, on both sides of each edge
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 129, 0);
    run("bucket_budget_over", e, &s, &pg, &cf, all64, SMMC_MAX_CHECKPOINTS, &out, records);
    s = make_sim(SMMC_MODE_GAUSSIAN, 360, 128, 0);
    run("bucket_budget_at", e, &s, &pg, &cf, all64, SMMC_MAX_CHECKPOINTS, &out, records);
    // LDS: 4096 rows x 4 words (65536 bytes), 4097 depletion counters, 3 n_bins buckets, four partials of 56 bytes:
    // n_bins = 3906 needs 129024 bytes (padded to 8) = 128 KiB less the reserve of 2048, n_bins = 3907 needs 129032
    p = pt, p.n_assets = 4, p.weights[0] = p.weights[1] = p.weights[2] = p.weights[3] = 0.25f;
    c = cf, c.amounts = steady.data();
    s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, 3907, 0);
    run("lds_budget_over", big, &s, &p, &c, yearly, 2, &out, records);
    s = make_sim(SMMC_MODE_TABLE, SMMC_MAX_CASHFLOW_PERIODS, 3906, 0);
    run("lds_budget_at", big, &s, &p, &c, yearly, 2, &out, records);
    if (entry == 0) {
      o = out, o.d_paid = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(paid) + 2);
      run("paid_misaligned", e, &gau, &pg, &cf, yearly, 30, &o, records);
      o = out, o.d_depleted_at = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(depleted) + 4);
      run("depleted_at_misaligned", e, &gau, &pg, &cf, yearly, 30, &o, records);
      run("records_misaligned", e, &gau, &pg, &cf, yearly, 30, &out, records + 4);
    }
    // a valid request passes every argument check; what stops it here is that this build has no kernel: ONE launch
    run("valid_table", e, &tab, &pt, &cf, yearly, 30, &out, records);
    run("valid_gaussian", e, &gau, &pg, &cf, yearly, 30, &out, records);
    c = cf, c.amounts = steady.data(), c.fractions = steady.data();
    run("valid_varying", e, &tab, &pt, &c, yearly, 30, &out, records);
    s = make_sim(SMMC_MODE_TABLE, 360, 0, 0);
    run("valid_no_buckets", e, &s, &pt, &cf, yearly, 30, &out, records);
    smmc_portfolio_cashflow_outputs none;
    std::memset(&none, 0, sizeof none);
    none.struct_size = sizeof none;
    run("valid_no_parent_outputs", e, &tab, &pt, &cf, yearly, 30, &none, records);
    // no paths: nothing to launch, SMMC_OK, empty records and an empty final record
    s = gau, s.n_paths = 0;
    o = out, o.d_depleted_at = nullptr;  // tests/cpp/cashflow_launch_stub.cpp has no kernel that copies the counts out
    std::memset(records, 0xff, sizeof records);
    std::memset(stats, 0xff, sizeof stats);
    run("valid_no_paths", e, &s, &pg, &cf, yearly, 30, &o, records);
    int empty = 1;
    const size_t rb = static_cast<size_t>(smmc_stats_bytes(100));
    for (uint32_t k = 0; k < 30; ++k) {
      smmc_stats st;
      std::memcpy(&st, records + k * rb, sizeof st);
      empty = empty && st.count == 0 && st.below == 0 && st.underflow == 0 && st.overflow == 0 && st.sum == 0.0 && st.n_bins == 100;
      for (size_t b = 0; b < 100; ++b) {
        uint64_t v;
        std::memcpy(&v, records + k * rb + sizeof st + 8 * b, 8);
        empty = empty && v == 0;
      }
    }
    smmc_stats fin;
    std::memcpy(&fin, stats, sizeof fin);
    std::printf("empty:%s %d %d\n", tag, empty, fin.count == 0 && fin.n_bins == 100 ? 1 : 0);
  }

  const smmc_portfolio pt = make_pf(false, 12), pg = make_pf(true, 12);
  const smmc_sim t360 = make_sim(SMMC_MODE_TABLE, 360, 0, 0);
  smmc_cashflow c;
  // the form a launch is given is the form the PARENT's rule names, and the kernel's arguments are the request's
  {
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_final = finals;
    int rc = smmc_engine_simulate_portfolio_cashflow_checkpoints(e, &t360, &pt, &(c = make_cf(4.0f, 0.0f, 0.01f)), yearly, 30, &o, records);
    std::printf("ran:fast %d %d %d\n", rc, fake_pfcf_checkpoints_last_exact(),
                smmc_engine_portfolio_cashflow_divide_kind(e, &t360, &pt, &c));
    rc = smmc_engine_simulate_portfolio_cashflow_checkpoints(e, &t360, &pt, &(c = make_cf(4.0f, 0.004f, 0.01f)), yearly, 30, &o, records);
    std::printf("ran:exact %d %d %d\n", rc, fake_pfcf_checkpoints_last_exact(),
                smmc_engine_portfolio_cashflow_divide_kind(e, &t360, &pt, &c));
    std::printf("ran:arguments %u %u %u\n", fake_pfcf_checkpoints_last_n(), fake_pfcf_checkpoints_last_first_period(),
                fake_pfcf_checkpoints_last_padding() == 0xffffffffu ? 1u : 0u);
  }

  // the partial array grows with n_checkpoints x grid: the stub writes every entry of the array a launch is given, under
  // AddressSanitizer; one checkpoint on few paths first, then 64 on many
  {
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    smmc_sim s = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
    s.n_paths = 300;
    const int small = smmc_engine_simulate_portfolio_cashflow_checkpoints(e, &s, &pg, &(c = make_cf(4.0f, 0.0f, 0.01f)), yearly, 1, &o, records);
    const uint32_t n_small = fake_pfcf_checkpoints_last_n();
    s.n_paths = 100000000;
    uint32_t all[SMMC_MAX_CHECKPOINTS];
    for (uint32_t k = 0; k < SMMC_MAX_CHECKPOINTS; ++k) all[k] = k + 1;
    const int large = smmc_engine_simulate_portfolio_cashflow_checkpoints(e, &s, &pg, &c, all, SMMC_MAX_CHECKPOINTS, &o, records);
    s.n_paths = 300;
    const int again = smmc_engine_simulate_portfolio_cashflow_checkpoints(e, &s, &pg, &c, yearly, 3, &o, records);
    std::printf("grow:partials %d %d %d %u %u %u\n", small, large, again, n_small, SMMC_MAX_CHECKPOINTS + 0u, fake_pfcf_checkpoints_last_n());
  }

  // the accumulator lease: a call whose launch fails has taken the engine's accumulator -- final buckets, depletion counters
  // and checkpoint buckets, a count left in each -- and not given it back clean; the next user (a plain simulate through
  // tests/cpp/launch_fake.cpp with 4096 buckets, whose sixteen copies span the whole accumulator) must still get its own
  {
    smmc_engine *l = nullptr;
    const float table[3] = {1.0f, -2.0f, 0.5f};
    if (smmc_engine_create(0, nullptr, &l) != SMMC_OK || smmc_engine_set_table(l, table, 3) != SMMC_OK) return 1;
    smmc_sim s = make_sim(SMMC_MODE_TABLE, 36, SMMC_MAX_BINS, 0);
    s.n_paths = 5000;
    s.hist_lo = 400.0f;
    s.hist_hi = 2100.0f;
    std::vector<float> out(s.n_paths);
    std::vector<uint64_t> hist(SMMC_MAX_BINS), again(SMMC_MAX_BINS), want(SMMC_MAX_BINS, 0);
    smmc_stats st;
    for (uint64_t i = 0; i < s.n_paths; ++i) {
      const float v = fake_path_value(i, 7, 0, 36, 1000.0f);
      if (v >= s.hist_lo && v < s.hist_hi)
        want[std::min<int>(SMMC_MAX_BINS - 1, static_cast<int>((static_cast<double>(v) - 400.0) * (static_cast<double>(SMMC_MAX_BINS) / 1700.0)))] += 1;
    }
    const int first = smmc_engine_simulate_to_host(l, &s, out.data(), nullptr, nullptr, nullptr, &st, hist.data());
    smmc_portfolio_cashflow_outputs o;
    std::memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.d_stats = stats;
    o.d_depleted_at = depleted;
    const smmc_sim g = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_cashflow cf = make_cf(4.0f, 0.0f, 0.01f);
    const int folds = fake_pfcf_checkpoints_folds();
    const int failed = smmc_engine_simulate_portfolio_cashflow_checkpoints(l, &g, &pg, &cf, yearly, 30, &o, records);
    const int folded = fake_pfcf_checkpoints_folds() - folds;  // an error between kernel and folds: none is queued
    const int second = smmc_engine_simulate_to_host(l, &s, out.data(), nullptr, nullptr, nullptr, &st, again.data());
    std::printf("lease:after_failed_launch %d %d %d %d %d %d\n", first, failed, second, hist == want ? 1 : 0, again == want ? 1 : 0, folded);
    smmc_engine_destroy(l);
  }

  std::printf("sizes %zu %zu %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_portfolio), sizeof(smmc_cashflow), sizeof(smmc_portfolio_cashflow_outputs));
  for (smmc_engine *p : {e, no_table, big}) smmc_engine_destroy(p);
  std::printf("portfolio_cashflow_checkpoints_args: done\n");
  return 0;
}
