// Host-side proof that the scalar addressing of fill_affine_slim_kernel's interior steps addresses
// exactly what the per-lane bookkeeping addresses.  Stand-alone program (tests/test_step_addr_host.py compiles and runs
// it, host code only).  It walks every wave of a team through its sweep the way the kernel does -- per-lane column, strip
// and record base beside the scalar mirrors, the scalar record base, the ring address and the frozen column of an
// interior run, each updated where the kernel updates it -- and checks at every step:
//   * the mirrors equal lane 0's column and strip (boundary steps included), so the interior test is the parent's;
//   * in an interior step, for all 64 lanes: every lane is in lane 0's strip; scalar base + lane offset + immediate equals
//     lay + rec * RECDW + c * CH + slot * 4 for every chunk, and the tail piece likewise, in the packed form (Pack<1>)
//     and in the LEAN form (Rec<1,9,true>); the 32-bit lane offset never carries; the store stays inside the pair's
//     records; jj + s_adv is the lane's column and the unclamped code fetch stays within [1, m + 1];
//   * in an interior step, for all 64 lanes: factor * ring address + lane constant equals the (step, a) entry of the ring
//     for live lanes and the sentinel block for the others.
// Output, one line per case:  LEAN T n m layer_off steps interior_steps interior_runs
#include "bialign_kernels.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace bialign;

static long g_bad = 0;
static void bad(const char* what, int lean, int T, int w, int n, int m, int g, int lane, long long a, long long b) {
  if (++g_bad <= 20)
    std::fprintf(stderr, "MISMATCH %s: LEAN=%d T=%d w=%d n=%d m=%d step=%d lane=%d: %lld vs %lld\n", what, lean, T, w, n, m, g,
                 lane, a, b);
}

template <bool LEAN>
static void run_case(int T, int n, int m, int64_t layer_off) {
  constexpr int S = 1;
  using G = Geo<S>;
  using PK = Pack<S>;
  using R_ = Rec<S, 9, LEAN>;
  using GF = GhostFeed<S, 9, LEAN, 0>;
  using SA = StepAddr<S, LEAN>;
  using GS = GhostSrc<S, LEAN>;
  constexpr int W = G::W, R = G::R;
  // the host's sweep geometry (sweep_geometry in bialign_plan.hpp)
  const int NS = (n + 1 + G::RR - 1) / G::RR;
  const int P = std::max(m + 2, 2 * (G::R - 1) + GF::MIN_GOFF);
  const int Gsteps = (NS - 1) * P + m + G::MAXOFF + 1;
  const int rec_last = Gsteps - 1;
  const uint64_t layers = 0x00007f3400000000ull;            // the chunk buffer (any 4 GiB-aligned address)
  const uint64_t lay = layers + (uint64_t)layer_off * 4;    // the pair's storage, bytes
  const int64_t region = LEAN ? (int64_t)Gsteps * R_::RECDW : (int64_t)Gsteps * PK::RECDW;  // dwords interior steps may write
  const uint32_t ring_lds = 0x1200, sent_lds = 0x9000;     // LDS addresses of the wave's ring and the sentinel block
  long steps = 0, interior_steps = 0, runs = 0;
  for (int w = 0; w < T; ++w) {
    const int NSw = (NS - w + T - 1) / T;
    const int H = NSw > 0 ? (NSw - 1) * P + m + G::MAXOFF + 1 : 0;
    // per-lane state, as the kernel keeps it
    int jj[64], col[64], strip[64], rec_base[64];
    for (int L = 0; L < 64; ++L) {
      const int il = L / W, aa = L - il * W;
      jj[L] = col[L] = -(2 * il + aa);  // col: the lane's true column (the parent's jj)
      strip[L] = 0;
      rec_base[L] = w * P;
    }
    int s_ph = 0, s_q = 0, s_adv = 0;
    uint32_t ring_u = 0;
    uint64_t sbase = 0;
    bool was_interior = false;
    for (int g = 0; g < H; ++g, ++steps) {
      // the interior test: the parent reads lane 0, the change its mirrors
      if (s_ph != col[0]) bad("phase mirror", LEAN, T, w, n, m, g, 0, s_ph, col[0]);
      if (s_q != strip[0]) bad("strip mirror", LEAN, T, w, n, m, g, 0, s_q, strip[0]);
      const bool interior = PK::interior(s_q * T + w, s_ph, m);
      if (interior != PK::interior(strip[0] * T + w, col[0], m)) bad("interior test", LEAN, T, w, n, m, g, 0, interior, !interior);
      if (!interior) {
        for (int L = 0; L < 64; ++L) jj[L] += s_adv;
        s_adv = 0;
      }
      for (int L = 0; L < 64; ++L)
        if (jj[L] + s_adv != col[L]) bad("column", LEAN, T, w, n, m, g, L, jj[L] + s_adv, col[L]);
      const int gt = g & (GF::BLK - 1), ghalf = (g / GF::BLK) & 1;
      if (gt == 0) ring_u = ring_lds + ghalf * GS::HALFB;
      if (interior) {
        ++interior_steps;
        runs += !was_interior;
        if (sbase != lay + (uint64_t)SA::record_byte(g, s_q, T, w, P)) bad("record base", LEAN, T, w, n, m, g, 0, (long long)sbase, 0);
        if (ring_u != ring_lds + GS::ring_step_byte(g)) bad("ring address", LEAN, T, w, n, m, g, 0, ring_u, GS::ring_step_byte(g));
        for (int L = 0; L < 64; ++L) {
          const int il = L / W, aa = L - il * W;
          const bool live = L < R * W, ghost = il == 0;
          if (strip[L] != strip[0]) bad("lane in another strip", LEAN, T, w, n, m, g, L, strip[L], strip[0]);
          // the ghost source
          const uint32_t want_g = live ? ring_lds + (uint32_t)(ghalf * GF::SLOTS + (gt * W + aa) * GF::NP) * 16u : sent_lds;
          const uint32_t got_g = GS::factor(L) * ring_u + GS::lane_byte(L, sent_lds);
          if (got_g != want_g) bad("ghost source", LEAN, T, w, n, m, g, L, got_g, want_g);
          // the stores, by the parent's expressions
          const int rec = g + rec_base[L];
          const int pad_idx = L < W ? L : (L >= R * W ? W + (L - R * W) : 64);
          const bool pad_lane = pad_idx < R_::SLP - R_::SL;
          const bool storing = (live && (LEAN ? il == R - 1 : !ghost)) || (!LEAN && pad_lane);
          const int slot = LEAN ? aa : (pad_lane ? R_::SL + pad_idx : L - W);
          if (storing != SA::stores(L)) bad("who stores", LEAN, T, w, n, m, g, L, storing, SA::stores(L));
          if (!storing) continue;
          if (rec < 0 || rec > rec_last) bad("record outside the sweep", LEAN, T, w, n, m, g, L, rec, rec_last);
          const int recdw = LEAN ? R_::RECDW : PK::RECDW;
          for (int c = 0; c < SA::NCHUNK; ++c) {
            const int64_t dw = (int64_t)rec * recdw + c * R_::CH + slot * 4;
            const uint64_t got = sbase + (uint64_t)SA::chunk_off(L) + (uint64_t)SA::chunk_imm(c);
            if (got != lay + (uint64_t)dw * 4) bad("chunk store", LEAN, T, w, n, m, g, L, (long long)got, (long long)(lay + dw * 4));
            if (dw < 0 || dw + 4 > region) bad("chunk outside the pair", LEAN, T, w, n, m, g, L, dw, region);
          }
          const bool tail = LEAN ? R_::TAIL != 0 : (PK::TAILDW != 0 && slot < PK::TSLOTS);
          if (tail != SA::stores_tail(L)) bad("who stores the tail", LEAN, T, w, n, m, g, L, tail, SA::stores_tail(L));
          if (tail) {
            const int taildw = LEAN ? R_::TAIL : PK::TAILDW;
            const int64_t dw = (int64_t)rec * recdw + (LEAN ? R_::NCH4 : PK::NCH) * R_::CH + slot * taildw;
            const uint64_t got = sbase + (uint64_t)SA::tail_off(L) + (uint64_t)SA::TAIL_IMM;
            if (got != lay + (uint64_t)dw * 4) bad("tail store", LEAN, T, w, n, m, g, L, (long long)got, (long long)(lay + dw * 4));
            if (dw < 0 || dw + taildw > region) bad("tail outside the pair", LEAN, T, w, n, m, g, L, dw, region);
            if (SA::TAILB != taildw * 4) bad("tail bytes", LEAN, T, w, n, m, g, L, SA::TAILB, taildw * 4);
          }
        }
      }
      // ---- advance, as the kernel does
      for (int L = 0; L < 64; ++L) {
        if (interior) {
          // the unclamped code fetch of an interior step reads column jj + s_adv + 1 (s_adv already advanced)
          const int jc1 = jj[L] + (s_adv + 1) + 1;
          if (jc1 != std::min(std::max(col[L] + 2, 0), m + 1)) bad("unclamped code column", LEAN, T, w, n, m, g, L, jc1, col[L] + 2);
        } else {
          ++jj[L];
          if (jj[L] == P) {
            jj[L] = 0;
            ++strip[L];
            rec_base[L] += (T - 1) * P;
          }
        }
        if (interior && col[L] + 1 >= P) bad("interior step ends a strip", LEAN, T, w, n, m, g, L, col[L], P);
        if (interior) ++col[L];
        else col[L] = jj[L];
      }
      if (interior) ++s_adv;
      ++s_ph;
      if (!interior && s_ph == P) {
        s_ph = 0;
        ++s_q;
      }
      ring_u += GS::STEPB;
      if (interior) sbase += SA::RECB;
      else sbase = lay + (uint64_t)SA::record_byte(g + 1, s_q, T, w, P);
      was_interior = interior;
    }
  }
  std::printf("%d %d %d %d %lld %ld %ld %ld\n", LEAN ? 1 : 0, T, n, m, (long long)layer_off, steps, interior_steps, runs);
}

int main() {
  static const int shapes[][2] = {{41, 46}, {64, 300}, {300, 64}, {1024, 1024}, {1025, 1023}};
  static const int teams[] = {1, 2, 3, 6, 12};
  // dword offsets of the pair's storage: the buffer's start, just below a 4 GiB boundary (the pair's records straddle it)
  // and just above one
  static const int64_t offs[] = {0, (int64_t{1} << 30) - 4096, (int64_t{1} << 30) + 16, (int64_t{5} << 30) - 64};
  constexpr int LAG = 2 * (Geo<1>::R - 1) + 2 * GhostFeed<1, 9>::BLK + 16;  // team_shape(): T * lag + 64 <= P
  for (const auto& sh : shapes)
    for (int T : teams) {
      const int P = std::max(sh[1] + 2, 2 * (Geo<1>::R - 1) + GhostFeed<1, 9>::MIN_GOFF);
      if (T > 1 && T * LAG + 64 > P) continue;
      for (int64_t off : offs) {
        run_case<false>(T, sh[0], sh[1], off);
        run_case<true>(T, sh[0], sh[1], off);
      }
    }
  if (g_bad) std::fprintf(stderr, "%ld mismatches\n", g_bad);
  return g_bad ? 1 : 0;
}
