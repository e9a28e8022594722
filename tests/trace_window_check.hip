// Host-side proof for the LDS window of the affine traceback's short-chain kernel (TraceWindow<S>, bialign_trace_fast.hpp),
// from the kernels' own headers.  Stand-alone program (tests/test_trace_window_host.py compiles and runs it, host code only).
// Sim<S> steps the window the way traceback_affine_fast_kernel<S, true> does -- the same hit test, the same issue loop after
// a pick, the same invalidation at a strip change, all through TraceWindow's functions -- and keeps, per ring record, which
// record and slots were issued into it and the serial number of its DMA instructions; in the full form also, per ring dword,
// the byte of the pair's storage that the DMA's lane moved there.  Per shape and ring length (K and KMIN) it checks
//   1. along oracle-like walks (54 % diagonal columns) and adversarial ones (runs of one move, the drift extremes), at every
//      column the hit test admits and for every (state, candidate) the kernel would load: the ring dwords TraceWindow::addr
//      names hold the very bytes TraceFast::offsets names, moved by a DMA that the column's counted wait has retired;
//   2. from sampled points, with the window begun there as after a strip change, EVERY sequence of DEPTH legal moves: the
//      ring entries of records T - 3 .. T hold those records, their slots cover s - W .. s, and the wait retires them;
//   3. every DMA lane reads 16 aligned bytes inside its record, inside the pair's packed region.
// Output, one line per case:  S n m K columns fast hits records_issued dfs_nodes dfs_hits   (K = 0: no window at this max_shift)
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
struct Sim {
  using TF = TraceFast<S>;
  using TW = TraceWindow<S>;
  static constexpr int W = TF::W;
  struct Rec_ {
    int r = -1, slo = 0;
    long seq = 0;  // serial number of the record's first DMA instruction
  };
  int S_ = S, n, m, P, K;
  int64_t packed_bytes;
  int wnext = 0;
  bool wlive = false;
  long seq = 0, issued = 0;
  Rec_ ring[TW::K];
  std::vector<int64_t>* tag = nullptr;  // full form: per ring dword, the storage byte it holds (-1: nothing yet)
  std::vector<long>* tseq = nullptr;    // ... and the serial number of the DMA that moved it

  void issue(int r, int s, int64_t rec_byte) {
    const int slo = TW::slot_lo(s);
    if (slo < 0 || (slo & 1) || slo + TW::WS > Rec<S, 9>::SLP) bad("first slot", S, n, m, r, s, slo);
    ring[r & (K - 1)] = Rec_{r, slo, seq};
    for (int d = 0; d < TW::NDMA; ++d)
      for (int lane = 0; lane < 64; ++lane) {
        const uint32_t src = TW::src_off(TW::lane_src(d, lane), slo);
        if ((src & 15) || src + 16 > (uint32_t)TF::RECB) bad("DMA lane leaves its record", S, n, m, r, d, lane, src);
        if (rec_byte + src < 0 || rec_byte + src + 16 > packed_bytes) bad("DMA lane leaves the packed region", S, n, m, r, d, lane, rec_byte);
        if (tag)
          for (int w = 0; w < 4; ++w) {
            const size_t at = (TW::ring_byte(r, K) + d * 1024 + lane * 16) / 4 + w;
            (*tag)[at] = rec_byte + src + 4 * w;
            (*tseq)[at] = seq + d;
          }
      }
    seq += TW::NDMA;
    ++issued;
  }
  // the kernel's steps
  bool hit(const typename TF::Col& col, int il, int T) const { return col.fast && wlive && il >= 2 && T - TW::RECS_PER_COL >= wnext; }
  void strip_changed() { wlive = false; }
  void after_pick(const typename TF::Pos& pos, int i, int j, int k) {
    const int a1 = k - i + S, Tn = j + 2 * pos.il + a1;
    if (!wlive && pos.il >= 2) {
      wlive = true;
      wnext = Tn + 1;
    }
    if (wlive) {
      const int low = std::max(Tn - TW::RECS_PER_COL - TW::lead(K), 0);
      for (int r = wnext - 1; r >= low; --r) issue(r, (pos.il - 1) * W + a1, pos.row + ((int64_t)P + r) * TF::RECB);
      wnext = std::min(wnext, low);
    }
  }
  // DMA number q (and all before it) has landed after the column's wait
  bool retired(long q, int T) const { return seq - q > (long)pend(T); }
  int pend(int T) const {
    const int d = T - TW::RECS_PER_COL - wnext;
    if (d < 0 || d > TW::lead(K)) bad("lead out of the kernel's waits", S, n, m, T, wnext, d);
    return TW::may_pend(T, wnext);
  }
  // a hit column at (T, s): the ring entries of its records
  void check_records(int T, int s) {
    for (int r = T - TW::RECS_PER_COL; r <= T; ++r) {
      const Rec_& e = ring[r & (K - 1)];
      if (e.r != r) { bad("ring entry holds another record", S, n, m, T, r, e.r); continue; }
      if (e.slo > std::max(s - W, 0) || s > e.slo + TW::WS - 1) bad("slots not covered", S, n, m, T, s, r, e.slo);
      if (!retired(e.seq + TW::NDMA - 1, T)) bad("record not waited for", S, n, m, T, r, e.seq, seq);
    }
  }
};

static bool legal(int S, int i, int j, int k, int l, int code) {
  const int pi = i - ((code >> 3) & 1), pj = j - ((code >> 2) & 1), pk = k - ((code >> 1) & 1), pl = l - (code & 1);
  return code > 0 && pi >= 0 && pj >= 0 && pk >= 0 && pl >= 0 && std::abs(pk - pi) <= S && std::abs(pl - pj) <= S;
}

template <int S>
struct Case {
  using TF = TraceFast<S>;
  using TW = TraceWindow<S>;
  using G = Geo<S>;
  using PK = Pack<S>;
  static constexpr int W = TF::W;
  static constexpr int DEPTH = 6;
  int n, m, P;
  long columns = 0, fast = 0, hits = 0, issued = 0, dfs_nodes = 0, dfs_hits = 0;

  // one column of a walk in the full form: every (state, candidate) the kernel would load for
  void check_column(Sim<S>& sim, const typename TF::Pos& pos, int i, int j, int k, int l) {
    ++columns;
    const int a0 = k - i + S, T = j + 2 * pos.il + a0, s = (pos.il - 1) * W + a0;
    const typename TF::Col col = TF::column(pos.strip, pos.il, j, a0, P, m);
    fast += col.fast;
    if (!sim.hit(col, pos.il, T)) return;
    ++hits;
    sim.check_records(T, s);
    const uint32_t deny = TF::deny(i, j, k, l);
    for (int st = 0; st < 9; ++st)
      for (int c = 0; c < 16; ++c) {
        const typename TF::Entry e = TF::entry(st, l - j + S, c, -5, -3, -2);
        if (e.lo & deny) continue;
        const bool tail = (e.lo >> 16) & 1;
        const typename TF::Off g = TF::offsets(e, col, false, P);
        const typename TF::Off a = TW::addr(TW::wentry(st, l - j + S, c), tail, T, s, sim.K);
        if (a.base + 4 > (uint32_t)(sim.K * TW::RB) || a.word + 4 > (uint32_t)(sim.K * TW::RB) || (a.base & 3) || (a.word & 3)) {
          bad("window address leaves the ring", S, n, m, a.base, a.word, st, c);
          continue;
        }
        if ((*sim.tag)[a.base / 4] != pos.row + g.base) bad("base dword", S, n, m, (*sim.tag)[a.base / 4], pos.row + g.base, st, c);
        if ((*sim.tag)[a.word / 4] != pos.row + g.word) bad("halfword dword", S, n, m, (*sim.tag)[a.word / 4], pos.row + g.word, st, c);
        if (!sim.retired((*sim.tseq)[a.base / 4], T) || !sim.retired((*sim.tseq)[a.word / 4], T)) bad("dword not waited for", S, n, m, T, st, c);
      }
  }
  void move(Sim<S>& sim, typename TF::Pos& pos, int& i, int& j, int& k, int& l, int code) {
    if (code & 8) {
      const int was = pos.strip;
      pos.step_up(P);
      if (pos.strip != was) sim.strip_changed();
    }
    i -= (code >> 3) & 1, j -= (code >> 2) & 1, k -= (code >> 1) & 1, l -= code & 1;
    sim.after_pick(pos, i, j, k);
  }
  Sim<S> fresh(int K) {
    Sim<S> sim;
    sim.n = n, sim.m = m, sim.P = P, sim.K = K;
    const int NS = (n + 1 + G::RR - 1) / G::RR, Gs = (NS - 1) * P + m + G::MAXOFF + 1;
    sim.packed_bytes = (int64_t)Gs * PK::RECDW * 4;
    return sim;
  }
  void walk(int K, int kind, uint64_t seed) {
    Sim<S> sim = fresh(K);
    std::vector<int64_t> tag((size_t)K * TW::RB / 4, -1);
    std::vector<long> tseq(tag.size(), 0);
    sim.tag = &tag, sim.tseq = &tseq;
    int i = n, j = m, k = n, l = m;
    typename TF::Pos pos = TF::Pos::at(n, P);
    uint64_t r = seed;
    static const int extreme[] = {8, 2, 10, 4, 1, 12, 9, 6, 14, 11, 15, 3};
    int run = 0, code = 15;
    while (i || j || k || l) {
      check_column(sim, pos, i, j, k, l);
      for (int tries = 0;; ++tries) {
        if (kind == 0) code = (mix(++r) % 8 < 5) ? 15 : 1 + (int)(mix(++r) % 15);
        else if (run > 0 && tries == 0) --run;
        else {
          code = tries > 40 ? 1 + (int)(mix(++r) % 15) : extreme[mix(++r) % 12];
          run = (int)(mix(++r) % 9);
        }
        if (legal(S, i, j, k, l, code)) break;
      }
      move(sim, pos, i, j, k, l, code);
    }
    issued += sim.issued;
  }
  // every sequence of legal moves, to depth DEPTH, in the light form.  Moves that differ only in l (q3) move neither T nor s:
  // one q3 per (q0, q1, q2) is taken, the one that keeps the walk in the band.
  void dfs(const Sim<S>& sim0, const typename TF::Pos& pos0, int i, int j, int k, int l, int depth) {
    ++dfs_nodes;
    const int a0 = k - i + S, T = j + 2 * pos0.il + a0, s = (pos0.il - 1) * W + a0;
    const typename TF::Col col = TF::column(pos0.strip, pos0.il, j, a0, P, m);
    Sim<S> here = sim0;
    if (here.hit(col, pos0.il, T)) {
      ++dfs_hits;
      here.check_records(T, s);
    }
    if (depth == DEPTH) return;
    for (int q = 1; q < 8; ++q) {
      int code = q << 1 | ((q >> 1) & 1);
      if (!legal(S, i, j, k, l, code)) code ^= 1;
      if (!legal(S, i, j, k, l, code)) continue;
      Sim<S> sim = here;
      typename TF::Pos pos = pos0;
      int ii = i, jj = j, kk = k, ll = l;
      move(sim, pos, ii, jj, kk, ll, code);
      dfs(sim, pos, ii, jj, kk, ll, depth + 1);
    }
  }
  void run(int n_, int m_) {
    n = n_, m = m_;
    P = std::max(m + 2, 2 * (G::R - 1) + GhostFeed<S, 9, false>::MIN_GOFF);
    if constexpr (!TW::EXISTS) {
      std::printf("%d %d %d 0 0 0 0 0 0 0\n", S, n, m);
    } else {
      for (int K : {TW::KMIN, TW::K}) {
        columns = fast = hits = issued = dfs_nodes = dfs_hits = 0;
        for (int wk = 0; wk < 8; ++wk) walk(K, wk & 1, 1000 + wk);
        // sampled points, the window begun there as after a strip change (the pick that led there starts it)
        for (int t = 0; t < 12; ++t) {
          const int i = G::RR + 2 + (int)(mix(7 * t + 1) % (uint32_t)(n - G::RR - 1)), j = 1 + (int)(mix(7 * t + 2) % (uint32_t)m);
          const int k = std::min(std::max(i - S + (int)(mix(7 * t + 3) % W), 0), n), l = std::min(std::max(j - S + (int)(mix(7 * t + 4) % W), 0), m);
          Sim<S> sim = fresh(K);
          typename TF::Pos pos = TF::Pos::at(i, P);
          sim.after_pick(pos, i, j, k);
          dfs(sim, pos, i, j, k, l, 0);
        }
        std::printf("%d %d %d %d %ld %ld %ld %ld %ld %ld\n", S, n, m, K, columns, fast, hits, issued, dfs_nodes, dfs_hits);
      }
    }
  }
};

int main() {
  static_assert(TraceWindow<1>::EXISTS && TraceWindow<2>::EXISTS && !TraceWindow<3>::EXISTS, "which max_shift has a window");
  static_assert(TraceWindow<1>::D + TraceWindow<1>::SPAN <= TraceWindow<1>::K && TraceWindow<2>::D + TraceWindow<2>::SPAN <= TraceWindow<2>::K, "lead");
  Case<1>().run(45, 70);
  Case<1>().run(64, 64);
  Case<1>().run(41, 130);
  Case<1>().run(130, 41);
  Case<1>().run(130, 97);   // (the four above are the GPU tests' shapes; these two have fast columns in every lane row)
  Case<1>().run(70, 140);
  Case<2>().run(100, 100);
  Case<3>().run(100, 100);
  if (g_bad) {
    std::fprintf(stderr, "%d mismatches\n", g_bad);
    return 1;
  }
  return 0;
}
