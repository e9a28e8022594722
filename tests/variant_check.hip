// The instantiation plan of the sweeps and walks (bialign_amd/csrc/bialign_host.hpp), printed on the CPU.  Stand-alone
// program, host code only, no HIP call (tests/test_variant_cases_host.py compiles and runs it through plan_host.build).
// It calls the predicates that decide what is built -- fill_affine_exists, fill_linear_exists, fill_slim_exists,
// traceback_exists, traceback_fast_exists, TraceWindow<S>::EXISTS -- at run time over their whole domain and prints one
// line per existing variant, with `ladder=1` where a launcher of bialign_host.hpp / bialign_wide.hip instantiates it:
//
//   fill_affine S=<max_shift> TW=<waves per workgroup> F=<FillFlags by name, joined by +, or 0> ladder=<0|1>
//   fill_linear S=.. TW=.. F=.. ladder=..
//   fill_slim   S=.. TW=<team of 2, 3, 6, 12> F=<LEAN | PACK> ladder=1
//   trace_affine S=.. F=<TraceFlags by name> ladder=..      (S=0 with T_WIDE / T_LEVEL: the wide-band path, any max_shift)
//   trace_linear S=.. F=.. ladder=..
//   trace_fast  S=.. window=<0|1> ladder=1
//
// The ladders are stated here as bialign_host.hpp states them: per launcher the flag mask its with_flags() walks, the
// flags it adds, the condition on the base form, and its rungs.  No predicate is restated.
#include "bialign_host.hpp"

#include <cstdio>
#include <string>

using namespace bialign;

namespace bialign {
int fail(int code, const char*, ...) { return code; }
}  // namespace bialign

static constexpr int TEAMS[] = {1, 2, 4, 8};
static constexpr unsigned FILL_ALL = F_XCU | F_DENSE | F_LEAN | F_RESW | F_PACK | F_DENSE1 | F_BETA_ANY | F_LOCAL;
static constexpr unsigned TRACE_ALL = T_TRACE | T_STRIP | T_WIDE | T_PACK | T_DENSE1 | T_LEVEL;

// a flag word by the names of its bits (the enums' names without their prefix)
static std::string names(unsigned f, const char* const* bit_names) {
  std::string out;
  for (int b = 0; bit_names[b]; ++b)
    if (f & (1u << b)) out += (out.empty() ? "" : "+") + std::string(bit_names[b]);
  return out.empty() ? "0" : out;
}
static const char* const FILL_NAMES[] = {"XCU", "DENSE", "LEAN", "RESW", "PACK", "DENSE1", "BETA_ANY", "LOCAL", nullptr};
static const char* const TRACE_NAMES[] = {"TRACE", "STRIP", "WIDE", "PACK", "DENSE1", "LEVEL", nullptr};
static_assert(F_XCU == 1 && F_DENSE == 2 && F_LEAN == 4 && F_RESW == 8 && F_PACK == 16 && F_DENSE1 == 32 && F_BETA_ANY == 64 && F_LOCAL == 128,
              "FILL_NAMES is in bit order");
static_assert(T_TRACE == 1 && T_STRIP == 2 && T_WIDE == 4 && T_PACK == 8 && T_DENSE1 == 16 && T_LEVEL == 32, "TRACE_NAMES is in bit order");

static bool within(unsigned f, unsigned mask) { return (f & ~mask) == 0; }

// launch_fill_affine: mask, base form (S, 1, F) must exist, rungs "x8, x1, 8, 4, 2, 1"
// launch_fill_affine_local: mask | F_LOCAL, rungs "4, 1";  launch_resweep_affine: mask | F_RESW, one wave
static bool affine_ladder(int S, int TW, unsigned F) {
  if (F & F_LOCAL) return within(F & ~F_LOCAL, F_DENSE | F_LEAN | F_DENSE1) && (TW == 4 || TW == 1);
  if (F & F_RESW) return within(F & ~F_RESW, F_DENSE | F_DENSE1 | F_BETA_ANY) && TW == 1;
  const unsigned base = F & ~F_XCU;
  if (!within(base, F_DENSE | F_LEAN | F_PACK | F_DENSE1 | F_BETA_ANY) || !fill_affine_exists(S, 1, base)) return false;
  return (F & F_XCU) ? (TW == 8 || TW == 1) : true;
}
// launch_fill_linear: mask, rungs "x1, 8, 4, 2, 1";  _local: "4, 1";  launch_resweep_linear: one wave
static bool linear_ladder(int TW, unsigned F) {
  if (F & F_LOCAL) return within(F & ~F_LOCAL, F_DENSE | F_LEAN | F_DENSE1) && (TW == 4 || TW == 1);
  if (F & F_RESW) return within(F & ~F_RESW, F_DENSE | F_DENSE1) && TW == 1;
  if (!within(F & ~F_XCU, F_DENSE | F_LEAN | F_DENSE1)) return false;
  return (F & F_XCU) ? TW == 1 : true;
}
// launch_traceback_{affine,linear}: T_TRACE | T_PACK | T_DENSE1 (one layer: no T_PACK) at every max_shift; _strip:
// T_TRACE | T_STRIP with and without T_DENSE1; bialign_wide.hip, at S = 0 for both recurrences: T_WIDE with T_TRACE |
// T_DENSE1 where the AFFINE form exists, T_TRACE | T_LEVEL with and without T_DENSE1
static bool trace_ladder(bool affine, int S, unsigned F) {
  if (F & T_LEVEL) return S == 0 && (F & ~T_DENSE1) == (T_TRACE | T_LEVEL);
  if (F & T_WIDE) return S == 0 && within(F & ~T_WIDE, T_TRACE | T_DENSE1) && traceback_exists(true, 0, F);
  if (F & T_STRIP) return (F & ~T_DENSE1) == (T_TRACE | T_STRIP);
  return within(F, T_TRACE | T_DENSE1 | (affine ? T_PACK : 0u));
}

template <int S>
static void print_fast() {
  if (!traceback_fast_exists(S, T_TRACE | T_PACK)) return;
  std::printf("trace_fast S=%d window=0 ladder=1\n", S);
  if (TraceWindow<S>::EXISTS) std::printf("trace_fast S=%d window=1 ladder=1\n", S);
}

int main() {
  for (int S = 0; S <= 5; ++S)
    for (int TW : TEAMS)
      for (unsigned F = 0; F <= FILL_ALL; ++F)
        if (fill_affine_exists(S, TW, F)) std::printf("fill_affine S=%d TW=%d F=%s ladder=%d\n", S, TW, names(F, FILL_NAMES).c_str(), (int)affine_ladder(S, TW, F));
  for (int S = 0; S <= 5; ++S)
    for (int TW : TEAMS)
      for (unsigned F = 0; F <= FILL_ALL; ++F)
        if (fill_linear_exists(TW, F)) std::printf("fill_linear S=%d TW=%d F=%s ladder=%d\n", S, TW, names(F, FILL_NAMES).c_str(), (int)linear_ladder(TW, F));
  for (int S = 0; S <= 5; ++S)
    for (int TW : {2, 3, 6, 12})
      for (unsigned F : {(unsigned)F_LEAN, (unsigned)F_PACK})
        if (fill_slim_exists(S, F)) std::printf("fill_slim S=%d TW=%d F=%s ladder=1\n", S, TW, names(F, FILL_NAMES).c_str());
  for (int affine = 1; affine >= 0; --affine)
    for (int S = 0; S <= 5; ++S)
      for (unsigned F = 0; F <= TRACE_ALL; ++F)
        if (traceback_exists(affine, S, F))
          std::printf("trace_%s S=%d F=%s ladder=%d\n", affine ? "affine" : "linear", S, names(F, TRACE_NAMES).c_str(), (int)trace_ladder(affine, S, F));
#define VARIANT_FAST(S, X) print_fast<S>();
  BIALIGN_FOR_EACH_S(VARIANT_FAST, )
#undef VARIANT_FAST
  return 0;
}
