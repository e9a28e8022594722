// What the batch planner (bialign_amd/csrc/bialign_plan.hpp) decides about BIALIGN_BATCH_LOCAL, on the CPU.  Stand-alone
// program, host code only, no HIP call (tests/test_local_host.py compiles and runs it).  Every case is one creation as
// create_batch() orders it (bialign_capi.hip) without the device, then the team shape of a launch of all its pairs on a
// device that would hold cross-CU teams, and prints one line:
//     <name> rc=<code> local=<0/1> storage=<mode> flags=<the flags the planner saw> pack=<0/1> tw=<waves per workgroup>
//     gw=<workgroups per pair> slim=<0/1> msg=<message>
#include "bialign_plan.hpp"

#include <cstdarg>
#include <cstdio>

using namespace bialign;

static char g_msg[512] = "";
namespace bialign {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace bialign

struct Case {
  const char* name;
  uint32_t flags;
  int s, beta;
  int64_t budget;    // bytes
  int replicas;      // > 0: a null batch
  bool dense;        // mu1 and mu2 as dense tables
  const char* team;  // BIALIGN_TEAM, BIALIGN_PACK and BIALIGN_SLIM as a test would force them (nullptr: unset)
  const char* pack;
};

static void run(const Case& c) {
  const int n = 300, m = 400;
  if (c.team) setenv("BIALIGN_TEAM", c.team, 1); else unsetenv("BIALIGN_TEAM");
  if (c.pack) setenv("BIALIGN_PACK", c.pack, 1); else unsetenv("BIALIGN_PACK");
  bialign_params prm{};
  prm.max_shift = c.s, prm.flags = c.flags, prm.recurrence = BIALIGN_REC_AUTO;
  prm.gap_opening_cost = c.beta, prm.gap_cost = -50, prm.shift_cost = -150;
  std::vector<int32_t> s1(20 * 20, 0), s2(3 * 3, 0);
  s1[0] = 1100, s2[0] = 800;
  bialign_scoring sc{20, s1.data(), 3, s2.data()};
  const int32_t len_a[2] = {n, n}, len_b[2] = {m, m};
  const int64_t off_a[2] = {0, n}, off_b[2] = {0, m}, tab_off[2] = {0, (int64_t)n * m};
  std::vector<uint8_t> codes(2 * m, 0);
  std::vector<int32_t> tab(c.dense ? 2 * (size_t)n * m : 0, 100);
  bialign_pairs pr{};
  pr.npairs = 2;
  pr.len_a = len_a, pr.len_b = len_b, pr.off_a = off_a, pr.off_b = off_b;
  pr.seq_a = pr.seq_b = pr.cls_a = pr.cls_b = codes.data();
  if (c.dense) pr.mu1_dense = pr.mu2_dense = tab.data(), pr.mu1_off = pr.mu2_off = tab_off;

  g_msg[0] = 0;
  BatchPlan b;
  NullPlan nul{};
  const bialign_params* uprm = &prm;
  const bialign_pairs* upr = &pr;
  int rc = BIALIGN_OK;
  if (c.replicas) {
    rc = expand_null_pairs(&prm, &pr, nullptr, c.replicas, 7u, c.dense, nul);
    uprm = &nul.vprm, upr = &nul.vp;
  }
  const NullPlan* unul = c.replicas ? &nul : nullptr;
  int64_t colmax = 0;
  if (rc == BIALIGN_OK) rc = check_inputs(uprm, &sc, upr, nullptr, unul, b);
  if (rc == BIALIGN_OK) rc = score_bound(uprm, &sc, upr, nullptr, unul, b, &colmax);
  if (rc == BIALIGN_OK) rc = plan_pairs(upr, unul, colmax, b);
  if (rc == BIALIGN_OK) {
    decide_pack(b, colmax);
    rc = plan_storage(b, budget_dwords(c.budget, (size_t)1 << 40));
  }
  TeamShape ts;
  if (rc == BIALIGN_OK) ts = team_shape(b, 0, b.npairs, 256, 4096, 512);  // (a device that holds 4096 one-wave workgroups of the cross-CU kernel)
  const int storage = b.level_trace ? BIALIGN_BATCH_LEVEL_TRACE : (b.lean_trace ? BIALIGN_BATCH_LEAN_TRACE : (b.lean ? BIALIGN_BATCH_SCORE_ONLY : 0));
  std::printf("%s rc=%d local=%d storage=%d flags=%u pack=%d tw=%d gw=%d slim=%d msg=%s\n", c.name, rc, (int)b.local, storage,
              (unsigned)b.prm.flags, (int)b.pack_now(), ts.tw, ts.gw, (int)ts.slim, g_msg);
}

int main() {
  const uint32_t LOCAL = BIALIGN_BATCH_LOCAL, SO = BIALIGN_BATCH_SCORE_ONLY;
  const int64_t roomy = (int64_t)1 << 36, tight = 16 << 20;  // a 300 x 400 pair's full layers at max_shift 1: ~42 MB; its LEAN form: ~2 MB
  const Case cases[] = {
      {"plain-full", 0, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"local-full-affine", LOCAL, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"local-full-linear", LOCAL, 2, 0, roomy, 0, false, nullptr, nullptr},
      {"local-full-s0", LOCAL, 0, -150, roomy, 0, false, nullptr, nullptr},
      {"local-full-s5", LOCAL, 5, -150, roomy, 0, false, nullptr, nullptr},
      {"local-full-dense", LOCAL, 1, -150, roomy, 0, true, nullptr, nullptr},
      {"local-score-only", LOCAL | SO, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"local-fit", LOCAL | BIALIGN_BATCH_FIT, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"local-lean-trace", LOCAL | BIALIGN_BATCH_LEAN_TRACE, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"local-level-trace", LOCAL | BIALIGN_BATCH_LEVEL_TRACE, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"local-level-trace-wide", LOCAL | BIALIGN_BATCH_LEVEL_TRACE, 7, -150, roomy, 0, false, nullptr, nullptr},
      {"local-wide", LOCAL, 6, -150, roomy, 0, false, nullptr, nullptr},
      {"local-wide-score-only", LOCAL | SO, 6, -150, roomy, 0, false, nullptr, nullptr},
      {"local-beta-positive", LOCAL, 1, 100, roomy, 0, false, nullptr, nullptr},
      {"plain-tight", 0, 1, -150, tight, 0, false, nullptr, nullptr},
      {"local-tight", LOCAL, 1, -150, tight, 0, false, nullptr, nullptr},
      {"local-tight-score-only", LOCAL | SO, 1, -150, tight, 0, false, nullptr, nullptr},
      {"null-plain", 0, 1, -150, roomy, 4, false, nullptr, nullptr},
      {"null-local", LOCAL, 1, -150, roomy, 4, false, nullptr, nullptr},
      {"null-local-dense", LOCAL, 1, -150, roomy, 4, true, nullptr, nullptr},
      {"unknown-bit-16", 16u, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"unknown-bit-32", 32u, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"unknown-bit-local", LOCAL | 0x100u, 1, -150, roomy, 0, false, nullptr, nullptr},
      {"null-unknown-bit", 32u, 1, -150, roomy, 4, false, nullptr, nullptr},
      // what a test can force: without the flag it takes, with the flag it does not
      {"plain-forced-pack-x4", 0, 1, -150, roomy, 0, false, "x4", "1"},
      {"local-forced-pack-x4", LOCAL, 1, -150, roomy, 0, false, "x4", "1"},
      {"plain-forced-3", 0, 1, -150, roomy, 0, false, "3", "1"},
      {"local-forced-3", LOCAL, 1, -150, roomy, 0, false, "3", "1"},
      {"local-forced-h2", LOCAL, 2, -150, roomy, 0, false, "h2", "1"},
      {"local-score-only-forced-3", LOCAL | SO, 1, -150, roomy, 0, false, "3", nullptr},
  };
  for (const Case& c : cases) run(c);
  return 0;
}
