// Host-side proof for the affine traceback's short-chain kernel (bialign_trace_fast.hpp), from the kernels' own headers.
// Stand-alone program (tests/test_trace_fast_host.py compiles and runs it, host code only).  Per shape it checks
//   1. every entry of the candidate table against the generic walk's own candidate rule (affine_candidate, the function
//      walk_affine calls per column): offset code, source state, score for arbitrary mu1 / mu2, look-ahead, band-column guard;
//   2. the carried row (strip, il, row offset) against a fresh division, down every row and along random walks, and, at
//      EVERY lattice point and every (state, candidate) the kernel would load for, the guard mask against the generic
//      kernel's guard and base + 32-bit offset against
//      packed_addr(): same dwords, same half / corner / anchor, inside the pair's packed region, no 32-bit wrap; where
//      Col::fast fails nothing is claimed (the kernel calls packed_addr itself there);
//   3. packed_load(packed_addr()), the address function with its decode, against packed_cell (which the generic kernel
//      and the dump keep) for every in-band cell, on storage filled with patterns that make the 0xffff corner offsets
//      frequent.
// Output, one line per case:  S n m points loads fast_loads codes_by_il_seen walk_steps cells
#include "bialign_kernels.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace bialign;

static int g_bad = 0;
static void bad(const char* what, int S, int n, int m, long long a, long long b, long long c = 0, long long d = 0) {
  if (++g_bad <= 20) std::fprintf(stderr, "MISMATCH %s: S=%d n=%d m=%d: %lld %lld %lld %lld\n", what, S, n, m, a, b, c, d);
}
static uint32_t mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (uint32_t)x;
}

template <int S>
static void check_table() {
  using TF = TraceFast<S>;
  const int prm[][3] = {{-5, -3, -2}, {0, -7, 0}, {-1100, -350, -250}, {3, 11, -13}};  // beta, gamma, delta
  for (const auto& p : prm)
    for (int st = 0; st < 9; ++st)
      for (int b0 = 0; b0 < TF::W; ++b0)
        for (int c = 0; c < 16; ++c) {
          const typename TF::Entry e = TF::entry(st, b0, c, p[0], p[1], p[2]);
          const int ss = (e.lo >> 4) & 15;
          if (c == 15) {
            if (!(e.lo & TF::NEVER)) bad("lane 15 is a candidate", S, 0, 0, st, b0, c);
            continue;
          }
          for (int t = 0; t < 3; ++t) {
            const int mu1 = (int)(mix(t * 7 + 1) % 2001) - 1000, mu2 = (int)(mix(t * 13 + 5) % 2001) - 1000;
            const AffineCandidate g = affine_candidate(st, c, p[0], p[1], p[2], mu1, mu2);
            const int code = g.o0 * 8 + g.o1 * 4 + g.o2 * 2 + g.o3;
            if ((int)(e.lo & 15) != code) bad("code", S, 0, 0, st, b0, c, e.lo & 15);
            const int b = b0 + g.o1 - g.o3;
            const bool inband = b >= 0 && b < TF::W;  // |pl - pj| <= S
            if (!(e.lo & TF::NEVER) != inband) bad("band-column guard", S, 0, 0, st, b0, c, ss);
            if (!inband) continue;
            if (ss != g.ss) bad("source state", S, 0, 0, st, b0, c, ss);
            const int sc = e.cst + (((e.lo >> 8) & 1) ? mu1 : 0) + (((e.lo >> 9) & 1) ? mu2 : 0);
            if (sc != g.sc) bad("score", S, 0, 0, st, c, sc, g.sc);
            if (((int)(e.lo << 19) >> 29) != g.inc0 || ((int)(e.lo << 16) >> 29) != g.inc1) bad("look-ahead", S, 0, 0, st, b0, c);
          }
        }
}

template <int S>
static void run_case(int n, int m, bool cells) {
  using TF = TraceFast<S>;
  using G = Geo<S>;
  using PK = Pack<S>;
  using GF = GhostFeed<S, 9, false>;
  constexpr int W = TF::W, RR = TF::RR;
  PairDesc pd{};
  pd.n = n, pd.m = m;
  pd.NS = (n + 1 + G::RR - 1) / G::RR;  // the host's sweep geometry (sweep_geometry in bialign_plan.hpp)
  pd.P = std::max(m + 2, 2 * (G::R - 1) + GF::MIN_GOFF);
  pd.G = (pd.NS - 1) * pd.P + m + G::MAXOFF + 1;
  pd.layer_off = 0;
  const int P = pd.P;
  const int64_t packed_bytes = (int64_t)pd.G * PK::RECDW * 4, total_dw = PK::pair_dwords(pd.G, P, m);
  long points = 0, loads = 0, fast = 0, walk_steps = 0, ncells = 0;
  std::vector<char> seen((RR + 1) * 16, 0);  // (il, offset code) taken on the fast path

  // one point of the walk: every (state, candidate) the kernel would load for
  auto check_point = [&](const typename TF::Pos& pos, int i, int j, int k, int l) {
    ++points;
    const int a0 = k - i + S;
    const uint32_t deny = TF::deny(i, j, k, l);
    const typename TF::Col col = TF::column(pos.strip, pos.il, j, a0, P, m);
    const bool interior = col.fast;
    for (int st = 0; st < 9; ++st)
      for (int c = 0; c < 16; ++c) {
        const typename TF::Entry e = TF::entry(st, l - j + S, c, -5, -3, -2);
        const uint32_t lo = e.lo;
        const bool ok = (lo & deny) == 0;
        // the generic kernel's guard (pyx:133-141)
        const AffineCandidate g = affine_candidate(st, std::min(c, 14), 0, 0, 0, 0, 0);
        const int pi = i - g.o0, pj = j - g.o1, pk = k - g.o2, pl = l - g.o3;
        const bool gok = c < 15 && pi >= 0 && pj >= 0 && pk >= 0 && pl >= 0 && std::abs(pk - pi) <= S && std::abs(pl - pj) <= S;
        if (ok != gok) bad("guard", S, n, m, i, j, st, c);
        if (!ok) continue;
        ++loads;
        const PackedAddr ad = packed_addr<S>(pd, pi, pj, pk - pi + S, pl - pj + S, g.ss);
        if (ad.dw < 0 || ad.dw >= total_dw || ad.hdw < 0 || ad.hdw >= total_dw) bad("address function leaves the pair", S, n, m, ad.dw, ad.hdw);
        if (!interior) continue;
        ++fast;
        seen[pos.il * 16 + (lo & 15)] = 1;
        if (!ad.packed) { bad("fast path at a full record", S, n, m, i, j, st, c); continue; }
        const typename TF::Off o = TF::offsets(e, col, pos.il == 1, P);  // 32-bit sums: a wrap would miss the dword below
        const int64_t bb = pos.row + o.base, wb = pos.row + o.word;
        if (bb != ad.dw * 4) bad("base dword", S, n, m, bb, ad.dw * 4, i, j);
        if (wb != ad.hdw * 4) bad("halfword dword", S, n, m, wb, ad.hdw * 4, st, c);
        if (bb < 0 || wb < 0 || bb + 4 > packed_bytes || wb + 4 > packed_bytes) bad("outside the packed region", S, n, m, bb, wb);
        const uint32_t half = (lo >> 17) & 3;
        if ((half == 2) != ad.anchor || (!ad.anchor && (int)half != ad.half) || (bool)((lo >> 19) & 1) != ad.corner)
          bad("half / corner / anchor", S, n, m, half, ad.half, st, c);
      }
  };

  // down every row: the carried position against a fresh division; every lattice point of the band
  typename TF::Pos pos = TF::Pos::at(n, P);
  for (int i = n; i >= 0; --i) {
    const typename TF::Pos f = TF::Pos::at(i, P);
    if (pos.strip != f.strip || pos.il != f.il || pos.row != f.row || pos.strip * RR + pos.il - 1 != i)
      bad("carried row", S, n, m, i, pos.strip, pos.il, pos.row);
    for (int j = 0; j <= m; ++j)
      for (int k = std::max(i - S, 0); k <= std::min(i + S, n); ++k)
        for (int l = std::max(j - S, 0); l <= std::min(j + S, m); ++l) check_point(pos, i, j, k, l);
    if (i > 0) pos.step_up(P);
  }
  // random walks, stepped the way the kernel steps (row carried, never recomputed)
  for (int wk = 0; wk < 8; ++wk) {
    int i = n, j = m, k = n, l = m;
    typename TF::Pos p = TF::Pos::at(n, P);
    uint64_t r = 1000 + wk;
    while (i || j || k || l) {
      int code = 0;
      for (int tries = 0;; ++tries) {
        code = (mix(++r) % 8 < 5) ? 15 : 1 + (int)(mix(++r) % 15);
        const int pi = i - ((code >> 3) & 1), pj = j - ((code >> 2) & 1), pk = k - ((code >> 1) & 1), pl = l - (code & 1);
        if (pi >= 0 && pj >= 0 && pk >= 0 && pl >= 0 && std::abs(pk - pi) <= S && std::abs(pl - pj) <= S) break;
      }
      if (code & 8) p.step_up(P);
      i -= (code >> 3) & 1, j -= (code >> 2) & 1, k -= (code >> 1) & 1, l -= code & 1;
      const typename TF::Pos f = TF::Pos::at(i, P);
      if (p.strip != f.strip || p.il != f.il || p.row != f.row) bad("walked row", S, n, m, i, p.strip, p.il);
      check_point(p, i, j, k, l);
      ++walk_steps;
    }
  }
  int codes_seen = 0;
  for (int il = 1; il <= RR; ++il)
    for (int code = 1; code < 16; ++code) codes_seen += seen[il * 16 + code];

  // the address function and its decode against packed_cell
  if (cells) {
    std::vector<int32_t> lay(total_dw);
    for (int fill = 0; fill < 2; ++fill) {
      for (int64_t x = 0; x < total_dw; ++x) {
        const uint32_t h = mix(x * 2 + fill);
        lay[x] = fill == 0 ? (int32_t)h : (int32_t)((h & 3) | ((h >> 8) & 3) << 16);  // fill 1: offsets 0xffff are frequent
      }
      for (int i = 0; i <= n; ++i)
        for (int j = 0; j <= m; ++j)
          for (int aa = 0; aa < W; ++aa)
            for (int bb = 0; bb < W; ++bb) {
              const int k = i + aa - S, l = j + bb - S;
              if (k < 0 || k > n || l < 0 || l > m) continue;
              for (int st = 0; st < 9; ++st) {
                ++ncells;
                const int was = packed_cell<S>(lay.data(), pd, i, j, aa, bb, st), is = packed_load<S>(lay.data(), packed_addr<S>(pd, i, j, aa, bb, st));
                if (was != is) bad("packed_cell", S, n, m, i, j, was, is);
              }
            }
    }
  }
  std::printf("%d %d %d %ld %ld %ld %d %ld %ld\n", S, n, m, points, loads, fast, codes_seen, walk_steps, ncells);
}

int main() {
  check_table<1>();
  check_table<2>();
  check_table<3>();
  run_case<1>(45, 45, true);
  run_case<1>(47, 61, true);
  run_case<1>(130, 97, true);
  run_case<1>(12, 40, true);     // n < RR: one strip, nothing interior
  run_case<1>(70, 140, false);
  run_case<2>(25, 30, true);
  run_case<2>(60, 41, true);
  run_case<2>(41, 120, false);
  run_case<3>(20, 26, true);
  run_case<3>(50, 37, true);
  run_case<3>(37, 90, false);
  if (g_bad) {
    std::fprintf(stderr, "%d mismatches\n", g_bad);
    return 1;
  }
  return 0;
}
