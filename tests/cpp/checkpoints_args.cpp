// checkpoints_args.cpp -- the argument checks of smmc_engine_simulate_checkpoints (include/smmc.h) without a GPU:
// csrc/smmc_capi.cpp over tests/cpp/fake_hip.cpp (host memory behind the HIP entry points) and
// tests/cpp/launch_fake.cpp.  Every check runs before any device work, so each bad request must come back as
// SMMC_ERR_INVALID with a text in smmc_last_error(); TEST INFRASTRUCTURE, driven by tests/test_checkpoints_cpu.py.
// Prints one line per case: "<name> <return code> <length of the error text>", then "checkpoints_args: done".
#include <cstdio>
#include <cstring>
#include <vector>

#include "smmc.h"

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

static void report(const char *name, int rc) {
  std::printf("%s %d %zu\n", name, rc, rc ? std::strlen(smmc_last_error()) : static_cast<size_t>(0));
  if (rc) std::printf("#   %s\n", smmc_last_error());
}

int main() {
  smmc_engine *e = nullptr;
  if (smmc_engine_create(0, nullptr, &e) != SMMC_OK) {
    std::printf("engine_create failed: %s\n", smmc_last_error());
    return 1;
  }
  const float table[3] = {1.0f, -2.0f, 0.5f};
  if (smmc_engine_set_table(e, table, 3) != SMMC_OK) return 1;
  alignas(8) static unsigned char records[64 * (64 + 8 * 256)];
  std::vector<uint32_t> up(SMMC_MAX_CHECKPOINTS + 1);
  for (size_t i = 0; i < up.size(); ++i) up[i] = static_cast<uint32_t>(i + 1);
  const uint32_t zero[2] = {0, 5}, above[2] = {5, 361}, equal[3] = {5, 9, 9}, down[3] = {5, 9, 8};

  for (int to_host = 0; to_host < 2; ++to_host) {
    auto call = [&](const smmc_sim &s, const uint32_t *periods, uint32_t n, void *rec) {
      return to_host ? smmc_engine_simulate_checkpoints_to_host(e, &s, periods, n, nullptr, rec)
                     : smmc_engine_simulate_checkpoints(e, &s, periods, n, nullptr, rec);
    };
    const char *tag = to_host ? "to_host" : "device";
    char name[96];
    auto run = [&](const char *what, int rc) {
      std::snprintf(name, sizeof name, "%s:%s", tag, what);
      report(name, rc);
    };
    const smmc_sim ok = make_sim(SMMC_MODE_TABLE, 360, 100, 0);
    run("n_checkpoints_zero", call(ok, up.data(), 0, records));
    run("n_checkpoints_above_max", call(ok, up.data(), SMMC_MAX_CHECKPOINTS + 1, records));
    run("period_zero", call(ok, zero, 2, records));
    run("period_above_n_periods", call(ok, above, 2, records));
    run("period_repeated", call(ok, equal, 3, records));
    run("period_decreasing", call(ok, down, 3, records));
    run("periods_null", call(ok, nullptr, 2, records));
    run("records_null", call(ok, up.data(), 2, nullptr));
    run("stream_ref", call(make_sim(SMMC_MODE_TABLE, 360, 100, SMMC_FLAG_STREAM_REF), up.data(), 2, records));
    run("stream_v2", call(make_sim(SMMC_MODE_GAUSSIAN, 360, 100, SMMC_FLAG_STREAM_V2), up.data(), 2, records));
    run("histogram_budget_64x129", call(make_sim(SMMC_MODE_GAUSSIAN, 360, 129, 0), up.data(), 64, records));
    run("histogram_budget_32x257", call(make_sim(SMMC_MODE_TABLE, 360, 257, 0), up.data(), 32, records));
    run("engine_null", to_host ? smmc_engine_simulate_checkpoints_to_host(nullptr, &ok, up.data(), 2, nullptr, records)
                               : smmc_engine_simulate_checkpoints(nullptr, &ok, up.data(), 2, nullptr, records));
  }
  // the budget itself admits what the header promises (the constant, not a launch: there is no kernel here)
  std::printf("budget %d %d\n", SMMC_MAX_CHECKPOINT_BINS >= 64 * 128, SMMC_MAX_CHECKPOINT_BINS >= 31 * 256);
  // a valid request passes every argument check; what stops it here is that this build has no kernel
  const smmc_sim ok = make_sim(SMMC_MODE_GAUSSIAN, 360, 128, 0);
  report("valid_request_without_kernel", smmc_engine_simulate_checkpoints(e, &ok, up.data(), 64, nullptr, records));
  smmc_engine_destroy(e);
  std::printf("checkpoints_args: done\n");
  return 0;
}
