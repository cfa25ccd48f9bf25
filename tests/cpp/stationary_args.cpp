// stationary_args.cpp -- the argument checks of smmc_engine_simulate_stationary, its _to_host form and
// smmc_engine_stationary_divide_kind (include/smmc.h) without a GPU: csrc/smmc_stationary.cpp and the library's other host
// units over tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any device
// work, so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error(); TEST INFRASTRUCTURE,
// driven by tests/test_stationary_cpu.py, which builds it with AddressSanitizer and UBSan.  Prints one line per case:
// "<name> <return code> <length of the error text>", then "kind:<case> <SMMC_DIV_*> <smmc_engine_divide_kind's>" lines,
// then "sizes ...", then "stationary_args: done".
#include <cstdio>
#include <cstring>
#include <vector>

#include "smmc.h"

namespace smmc {
extern size_t stationary_stub_extra_lds;  // tests/cpp/stationary_launch_stub.cpp
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

static smmc_stationary make_stationary(uint32_t q) {
  smmc_stationary st;
  std::memset(&st, 0, sizeof st);
  st.struct_size = sizeof st;
  st.renew_q16 = q;
  return st;
}

static void report(const char *name, int rc) {
  std::printf("%s %d %zu\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0));
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr, *no_table = nullptr, *big_table = nullptr, *redo = nullptr, *calm = nullptr;
  for (smmc_engine **p : {&e, &no_table, &big_table, &redo, &calm})
    if (smmc_engine_create(0, nullptr, p) != SMMC_OK) {
      std::printf("engine_create failed: %s\n", smmc_last_error());
      return 1;
    }
  const float table[3] = {1.0f, -2.0f, 0.5f};
  if (smmc_engine_set_table(e, table, 3) != SMMC_OK) return 1;
  const std::vector<float> largest(SMMC_MAX_TABLE, 0.5f);
  if (smmc_engine_set_table(big_table, largest.data(), SMMC_MAX_TABLE) != SMMC_OK) return 1;
  const float redo_table[8] = {100.0f, 100.0f, 100.0f, 100.0f, 100.0f, -50.0f, -50.0f, -50.0f};
  if (smmc_engine_set_table(redo, redo_table, 8) != SMMC_OK) return 1;
  const float calm_table[2] = {1.0f, -1.0f};
  if (smmc_engine_set_table(calm, calm_table, 2) != SMMC_OK) return 1;
  alignas(8) static unsigned char stats_raw[64 + 8 * 4096];
  static uint64_t hist[4096];
  smmc_stats rec;

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim &s, const smmc_stationary *st) {
      if (entry == 0) return smmc_engine_simulate_stationary(eng, &s, st, nullptr, nullptr, nullptr, stats_raw);
      if (entry == 1) return smmc_engine_simulate_stationary_to_host(eng, &s, st, nullptr, nullptr, nullptr, nullptr, &rec, hist);
      return smmc_engine_stationary_divide_kind(eng, &s, st);
    };
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    char name[96];
    auto run = [&](const char *what, int rc) {
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc);
    };
    const smmc_sim ok = make_sim(SMMC_MODE_TABLE, 360, 100, 0);
    const smmc_stationary q12 = make_stationary(5461);
    run("stationary_null", call(e, ok, nullptr));
    smmc_stationary bad = q12;
    bad.struct_size = sizeof bad - 4;
    run("struct_size_wrong", call(e, ok, &bad));
    bad = make_stationary(SMMC_RENEW_Q16_ONE + 1u);
    run("renew_above_one", call(e, ok, &bad));
    bad = make_stationary(0xFFFFFFFFu);
    run("renew_all_ones", call(e, ok, &bad));
    bad = q12;
    bad.reserved[0] = 1;
    run("reserved0_not_zero", call(e, ok, &bad));
    bad = q12;
    bad.reserved[1] = 7;
    run("reserved1_not_zero", call(e, ok, &bad));
    run("mode_gaussian", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0), &q12));
    run("stream_v2", call(e, make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_V2), &q12));
    run("stream_ref", call(e, make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF), &q12));
    run("no_table", call(no_table, ok, &q12));
    run("engine_null", call(nullptr, ok, &q12));
    run("n_bins_above_max", call(e, make_sim(SMMC_MODE_TABLE, 360, SMMC_MAX_BINS + 1, 0), &q12));
    // the largest table and histogram fit any device: the stub's LDS need is raised beyond it for this one case
    smmc::stationary_stub_extra_lds = size_t(1) << 20;
    run("lds_too_small", call(big_table, make_sim(SMMC_MODE_TABLE, 360, SMMC_MAX_BINS, 0), &q12));
    smmc::stationary_stub_extra_lds = 0;
    if (entry < 2) {
      // a valid request passes every argument check; what stops it here is that this build has no kernel
      run("valid", call(e, ok, &q12));
      const smmc_stationary never = make_stationary(0), always = make_stationary(SMMC_RENEW_Q16_ONE);
      run("valid_never", call(e, ok, &never));
      run("valid_always", call(e, ok, &always));
      run("valid_largest_table", call(big_table, make_sim(SMMC_MODE_TABLE, 360, 0, 0), &q12));
      smmc_sim none = ok;
      none.n_paths = 0;  // nothing is launched and nothing refused
      run("valid_no_paths", call(big_table, none, &q12));
    }
  }
  // which divide a launch uses: the rule of smmc_engine_divide_kind(e, sim, 0), whatever the renewal probability
  const smmc_stationary q4 = make_stationary(16384), q1 = make_stationary(SMMC_RENEW_Q16_ONE);
  const smmc_sim s360 = make_sim(SMMC_MODE_TABLE, 360, 0, 0);
  std::printf("kind:redo_table %d %d\n", smmc_engine_stationary_divide_kind(redo, &s360, &q4), smmc_engine_divide_kind(redo, &s360, 0));
  std::printf("kind:calm_table %d %d\n", smmc_engine_stationary_divide_kind(calm, &s360, &q4), smmc_engine_divide_kind(calm, &s360, 0));
  std::printf("kind:calm_table_always %d %d\n", smmc_engine_stationary_divide_kind(calm, &s360, &q1), smmc_engine_divide_kind(calm, &s360, 0));
  // bounds come from the extremes alone: the S&P 500's best and worst month (+42.2 %, -29.7 %) over 360 periods
  smmc_engine *sp = nullptr;
  const float sp_table[3] = {42.2f, -29.7f, 0.6f};
  if (smmc_engine_create(0, nullptr, &sp) != SMMC_OK || smmc_engine_set_table(sp, sp_table, 3) != SMMC_OK) return 1;
  const smmc_stationary q12k = make_stationary(5461);
  std::printf("kind:best_and_worst_month %d %d\n", smmc_engine_stationary_divide_kind(sp, &s360, &q12k), smmc_engine_divide_kind(sp, &s360, 0));
  smmc_engine_destroy(sp);
  const smmc_sim exact = make_sim(SMMC_MODE_TABLE, 360, 0, SMMC_FLAG_EXACT_DIV);
  std::printf("kind:exact_flag %d %d\n", smmc_engine_stationary_divide_kind(calm, &exact, &q4), smmc_engine_divide_kind(calm, &exact, 0));
  std::printf("sizes %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_stationary));
  for (smmc_engine *p : {e, no_table, big_table, redo, calm}) smmc_engine_destroy(p);
  std::printf("stationary_args: done\n");
  return 0;
}
