// Host-side proof that the ghost feed's steady-block fast path addresses exactly what the general path addresses.
// Stand-alone program (tests/test_feed_fastpath_host.py compiles and runs it, host code only): for every block a sweep
// prefetches -- every wave of a team, every strip -- where GhostFeed::steady() holds,
//     steady_base_dword + lane_offset(round, lane) / 4  ==  packed_src(round * 64 + lane)     for all 64 lanes of every round
// (the clipped surplus lanes of the last round included), every entry of the block is a packed record by the unpack's
// own test, and the block does not wrap.  Where steady() fails nothing is claimed.
// Output, one line per case:  S BLK T n m blocks steady steady_hi unsteady_hi   (_hi: blocks in lattice strips >= 2).
#include "bialign_kernels.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace bialign;

static int g_bad = 0;
static void bad(const char* what, int S, int T, int w, int n, int m, int h0, int r, int lane, long long a, long long b) {
  if (++g_bad <= 20)
    std::fprintf(stderr, "MISMATCH %s: S=%d T=%d w=%d n=%d m=%d h0=%d round=%d lane=%d: %lld vs %lld\n", what, S, T, w, n, m,
                 h0, r, lane, a, b);
}

template <int S, int BLKO>
static void run_case(int T, int n, int m) {
  using GF = GhostFeed<S, 9, false, BLKO>;
  using G = Geo<S>;
  using PK = Pack<S>;
  // the host's sweep geometry (sweep_geometry in bialign_plan.hpp)
  const int NS = (n + 1 + G::RR - 1) / G::RR;
  const int P = std::max(m + 2, 2 * (G::R - 1) + GF::MIN_GOFF);
  const int Gsteps = (NS - 1) * P + m + G::MAXOFF + 1;
  const int rec_last = Gsteps - 1;
  const int64_t bnd_off = (int64_t)Gsteps * PK::RECDW;
  long blocks = 0, steady = 0, steady_hi = 0, unsteady_hi = 0;
  for (int w = 0; w < T; ++w) {
    const int NSw = (NS - w + T - 1) / T;  // the wave's strips and steps, as the sweeps count them
    const int H = NSw > 0 ? (NSw - 1) * P + m + G::MAXOFF + 1 : 0;
    if (H == 0) continue;
    // the sweep prefetches block 0 up front and block g + BLK at every step g < H that is a multiple of BLK
    int blk_q = 0, blk_rem = 0;
    for (int h0 = 0; h0 <= (H - 1) / GF::BLK * GF::BLK + GF::BLK; h0 += GF::BLK) {
      if (blk_q != h0 / P || blk_rem != h0 % P) bad("block counters", S, T, w, n, m, h0, 0, 0, blk_q, blk_rem);
      const bool hi = blk_q * T + w >= 2;
      ++blocks;
      if (GF::steady(blk_q, blk_rem, P, T, w, m, rec_last)) {
        ++steady;
        steady_hi += hi;
        const int64_t base = GF::steady_base_dword(blk_q, blk_rem, P, T, w);
        for (int r = 0; r < GF::ROUNDS; ++r)
          for (int lane = 0; lane < 64; ++lane) {
            const int q = std::min(r * 64 + lane, GF::NPIECE - 1);
            const int64_t general = GF::packed_src((int64_t)0, q, bnd_off, blk_q, blk_rem, P, T, w, m, rec_last);
            const uint32_t off = GF::lane_offset(r, lane);
            if (off % 4 != 0) bad("offset alignment", S, T, w, n, m, h0, r, lane, off, 0);
            if (base + off / 4 != general) bad("source dword", S, T, w, n, m, h0, r, lane, base + off / 4, general);
            if (general < 0 || general >= bnd_off) bad("outside the packed region", S, T, w, n, m, h0, r, lane, general, bnd_off);
          }
        // the unpack of this block (fill_affine_slim_kernel; fill_affine_kernel, PK_COOP) takes every entry as packed:
        // its per-entry test must agree
        for (int t = 0; t < GF::BLK; ++t) {
          int ph = blk_rem + t, qst = blk_q * T + w;
          if (ph >= P) { ph -= P; qst += T; }
          const int ts = ph + 2 * (G::R - 1), over = ts >= P ? 1 : 0;
          if (!PK::interior(qst - 1 + over, ts - over * P, m)) bad("entry not packed", S, T, w, n, m, h0, 0, t, ts, 0);
        }
        if (blk_rem + GF::BLK >= P) bad("steady block wraps", S, T, w, n, m, h0, 0, 0, blk_rem, P);
      } else {
        unsteady_hi += hi;
      }
      blk_rem += GF::BLK;
      if (blk_rem >= P) { blk_rem -= P; ++blk_q; }
    }
  }
  std::printf("%d %d %d %d %d %ld %ld %ld %ld\n", S, GF::BLK, T, n, m, blocks, steady, steady_hi, unsteady_hi);
}

int main() {
  static const int shapes[][2] = {{110, 280}, {61, 256}, {221, 500}, {1024, 1024}, {105, 280}, {61, 46}, {333, 97}, {40, 700}};
  static const int teams[] = {1, 2, 3, 6};
  for (const auto& sh : shapes)
    for (int T : teams) {
      run_case<1, 0>(T, sh[0], sh[1]);
      run_case<2, 0>(T, sh[0], sh[1]);
      run_case<2, 2>(T, sh[0], sh[1]);  // the DIET ring of the s=2 kernel: half-length blocks
      run_case<3, 0>(T, sh[0], sh[1]);
    }
  if (g_bad) std::fprintf(stderr, "%d mismatches\n", g_bad);
  return g_bad ? 1 : 0;
}
