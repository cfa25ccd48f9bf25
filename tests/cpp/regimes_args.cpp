// regimes_args.cpp -- the argument checks of smmc_engine_simulate_regimes, its _to_host form and
// smmc_engine_regimes_divide_kind (include/smmc.h) without a GPU: csrc/smmc_regimes.cpp and the library's other host units
// over tests/cpp/fake_hip.cpp, tests/cpp/launch_fake.cpp and the launch stubs.  Every check runs before any device work,
// so each bad request must come back as SMMC_ERR_INVALID with a text in smmc_last_error(); TEST INFRASTRUCTURE, driven by
// tests/test_regimes_cpu.py, which builds it with AddressSanitizer and UBSan.  Prints one line per case:
// "<name> <return code> <length of the error text>", then "kind:<case> <SMMC_DIV_*>" lines, then "sizes ...", then
// "regimes_args: done".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "smmc.h"

namespace smmc {
extern size_t regimes_stub_extra_lds;  // tests/cpp/regimes_launch_stub.cpp
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
  s.gauss_std = -1.0f;                                      // not read
  s.n_bins = n_bins;
  s.hist_lo = 0.0f;
  s.hist_hi = 5000.0f;
  s.below_threshold = 1000.0f;
  s.flags = flags;
  return s;
}

static smmc_regimes make_regimes(float m0, float s0, float m1, float s1, uint32_t l0, uint32_t l1, uint32_t start1) {
  smmc_regimes rg;
  std::memset(&rg, 0, sizeof rg);
  rg.struct_size = sizeof rg;
  rg.mean[0] = m0;
  rg.mean[1] = m1;
  rg.std[0] = s0;
  rg.std[1] = s1;
  rg.leave_q16[0] = l0;
  rg.leave_q16[1] = l1;
  rg.start1_q16 = start1;
  return rg;
}

static void report(const char *name, int rc) {
  std::printf("%s %d %zu\n", name, rc, rc < 0 ? std::strlen(smmc_last_error()) : static_cast<size_t>(0));
  if (rc < 0) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr;
  if (smmc_engine_create(0, nullptr, &e) != SMMC_OK) {
    std::printf("engine_create failed: %s\n", smmc_last_error());
    return 1;
  }
  alignas(8) static unsigned char stats_raw[64 + 8 * 4096];
  static uint64_t hist[4096];
  smmc_stats rec;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

  for (int entry = 0; entry < 3; ++entry) {
    auto call = [&](smmc_engine *eng, const smmc_sim &s, const smmc_regimes *rg) {
      if (entry == 0) return smmc_engine_simulate_regimes(eng, &s, rg, nullptr, nullptr, nullptr, stats_raw);
      if (entry == 1) return smmc_engine_simulate_regimes_to_host(eng, &s, rg, nullptr, nullptr, nullptr, nullptr, &rec, hist);
      return smmc_engine_regimes_divide_kind(eng, &s, rg);
    };
    const char *tag = entry == 0 ? "device" : entry == 1 ? "to_host" : "divide_kind";
    char name[96];
    auto run = [&](const char *what, int rc) {
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc);
    };
    const smmc_sim ok = make_sim(SMMC_MODE_GAUSSIAN, 360, 100, 0);
    const smmc_regimes good = make_regimes(0.9f, 3.5f, -1.5f, 7.0f, 1638, 8192, 10920);
    run("regimes_null", call(e, ok, nullptr));
    smmc_regimes bad = good;
    bad.struct_size = sizeof bad - 4;
    run("struct_size_wrong", call(e, ok, &bad));
    run("mode_table", call(e, make_sim(SMMC_MODE_TABLE, 360, 100, 0), &good));
    run("stream_v2", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2), &good));
    run("stream_ref", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_REF), &good));
    bad = good;
    bad.leave_q16[0] = SMMC_REGIME_Q16_ONE + 1u;
    run("leave0_above_one", call(e, ok, &bad));
    bad = good;
    bad.leave_q16[1] = 0xFFFFFFFFu;
    run("leave1_all_ones", call(e, ok, &bad));
    bad = good;
    bad.start1_q16 = SMMC_REGIME_Q16_ONE + 1u;
    run("start1_above_one", call(e, ok, &bad));
    bad = good;
    bad.mean[0] = nan;
    run("mean0_nan", call(e, ok, &bad));
    bad = good;
    bad.mean[1] = inf;
    run("mean1_inf", call(e, ok, &bad));
    bad = good;
    bad.std[0] = inf;
    run("std0_inf", call(e, ok, &bad));
    bad = good;
    bad.std[1] = nan;
    run("std1_nan", call(e, ok, &bad));
    bad = good;
    bad.std[1] = -0.5f;
    run("std1_negative", call(e, ok, &bad));
    bad = good;
    bad.reserved[0] = 1;
    run("reserved0_not_zero", call(e, ok, &bad));
    bad = good;
    bad.reserved[1] = 7;
    run("reserved1_not_zero", call(e, ok, &bad));
    run("engine_null", call(nullptr, ok, &good));
    run("n_bins_above_max", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS + 1, 0), &good));
    // the draw tables and the largest histogram fit any device: the stub's LDS need is raised beyond it for this one case
    smmc::regimes_stub_extra_lds = size_t(1) << 20;
    run("lds_too_small", call(e, make_sim(SMMC_MODE_GAUSSIAN, 360, SMMC_MAX_BINS, 0), &good));
    smmc::regimes_stub_extra_lds = 0;
    if (entry < 2) {
      // a valid request passes every argument check; what stops it here is that this build has no kernel
      run("valid", call(e, ok, &good));
      const smmc_regimes edges = make_regimes(0.0f, 0.0f, 0.0f, 0.0f, 0, SMMC_REGIME_Q16_ONE, SMMC_REGIME_Q16_ONE);
      run("valid_edges", call(e, ok, &edges));
      run("valid_no_periods", call(e, make_sim(SMMC_MODE_GAUSSIAN, 0, 0, 0), &good));
      smmc_sim none = ok;
      none.n_paths = 0;  // nothing is launched and nothing refused
      run("valid_no_paths", call(e, none, &good));
    }
  }
  // which divide a launch uses: smmc_engine_divide_kind's rule on the union of the two regimes' bounds
  const smmc_sim s360 = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, 0);
  const smmc_regimes calm = make_regimes(0.5f, 0.8f, -0.5f, 1.5f, 1638, 8192, 10920);       // [88.999, 106.101]: proven
  const smmc_regimes crash = make_regimes(0.5f, 1.0f, -40.0f, 8.0f, 328, 656, 21845);       // [3.999, 116.001]: the window
  const smmc_regimes unbounded = make_regimes(0.9f, 3.5f, -1.5f, 15.0f, 1638, 8192, 10920);  // 98.5 - 105 < 0: no bounds
  std::printf("kind:calm %d\n", smmc_engine_regimes_divide_kind(e, &s360, &calm));
  std::printf("kind:crash %d\n", smmc_engine_regimes_divide_kind(e, &s360, &crash));
  std::printf("kind:unbounded %d\n", smmc_engine_regimes_divide_kind(e, &s360, &unbounded));
  // the calm regime alone is proven; the union with the other is not: each regime's bounds count
  const smmc_regimes crash_never = make_regimes(0.5f, 1.0f, -40.0f, 8.0f, 0, 656, 0);
  std::printf("kind:crash_never_entered %d\n", smmc_engine_regimes_divide_kind(e, &s360, &crash_never));
  const smmc_sim exact = make_sim(SMMC_MODE_GAUSSIAN, 360, 0, SMMC_FLAG_EXACT_DIV);
  std::printf("kind:exact_flag %d\n", smmc_engine_regimes_divide_kind(e, &exact, &calm));
  std::printf("sizes %zu %zu\n", sizeof(smmc_sim), sizeof(smmc_regimes));
  smmc_engine_destroy(e);
  std::printf("regimes_args: done\n");
  return 0;
}
