// glide_launch_stub.cpp -- beside tests/cpp/launch_fake.cpp and portfolio_cashflow_launch_stub.cpp: the launch symbol of
// the glide kernel (smmc_internal.h).  TEST INFRASTRUCTURE; it simulates nothing: a launch is COUNTED
// (fake_glide_launches), its divide form, its arguments and the change table it was handed are KEPT
// (fake_glide_last_exact, fake_glide_last_kernel_args, fake_glide_last_args, fake_glide_last_table: over the fake HIP
// runtime a device pointer is host memory and the upload has happened by the time of the launch), and it reports "no
// device", so a request that passes every argument check of csrc/smmc_glide.cpp ends as SMMC_ERR_HIP and a refused one
// must leave the count where it was.  Before it fails, a launch leaves a count in every bucket and depletion counter of
// the accumulator it was given: what the next user of the engine must not see.
#include <cstring>

#include "smmc_internal.h"

static int g_launches = 0, g_last_exact = -1;
static smmc::KernelArgs g_kernel_args;
static smmc::GlideArgs g_args;
static smmc::GlideEntry g_table[SMMC_MAX_GLIDE_CHANGES + 1];
extern "C" int fake_glide_launches(void) { return g_launches; }
extern "C" int fake_glide_last_exact(void) { return g_last_exact; }
extern "C" const void *fake_glide_last_kernel_args(void) { return &g_kernel_args; }
extern "C" const void *fake_glide_last_args(void) { return &g_args; }
extern "C" const void *fake_glide_last_table(void) { return g_table; }

namespace smmc {
hipError_t launch_glide(const KernelArgs &a, const GlideArgs &x, bool exact_div, uint32_t, hipStream_t) {
  ++g_launches;
  g_last_exact = exact_div ? 1 : 0;
  g_kernel_args = a;
  g_args = x;
  // the entries the kernel could read: it follows `next` from entry 0 and stops behind an entry whose next is 0
  std::memset(g_table, 0xff, sizeof g_table);
  uint32_t n = 0;
  if (x.table && x.first) {
    do {
      g_table[n] = x.table[n];
    } while (x.table[n++].next != 0 && n < SMMC_MAX_GLIDE_CHANGES);
  }
  if (x.table) g_table[n] = x.table[n];  // and the entry behind them
  for (uint32_t b = 0; a.d_hist && b < a.n_bins; ++b) a.d_hist[b] += 1;  // as a kernel whose fold is never queued would
  for (uint32_t t = 0; x.c.d_depleted && t <= a.n_periods; ++t) x.c.d_depleted[t] += 1;
  return hipErrorNoDevice;
}
}  // namespace smmc
