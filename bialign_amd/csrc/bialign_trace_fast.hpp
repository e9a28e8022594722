// bialign_trace_fast.hpp -- the affine traceback's short-chain column loop.  Part of bialign_kernels.hpp (include that, not this).
#pragma once

namespace bialign {

// ---------------------------------------------------------------------------
// traceback_affine_fast_kernel: the walk of traceback_affine_kernel<S, true, .., PACK> (tiled sweep, full storage, packed
// records, mu1 and mu2 by LOOKUP, S = 1..3) with a shorter per-column chain; every other form stays with the generic
// kernel, which is also this one's test partner (BIALIGN_TRACE_FAST=0).  Same results, bit for bit.
//   * Everything of a candidate that depends only on (state, band column of the point, candidate) -- offset code, source
//     state, constant part of the score, which of mu1 / mu2 enter, look-ahead increments, the guard as a bit mask, where the
//     value sits in its record -- is one 16-byte entry of a table built in LDS before the walk (TraceFast<S>::entry).
//   * The row of the point is carried as (strip, il); a step up wraps il to RR.  No division in the loop.
//   * A cell's address is a 32-bit byte offset from a scalar pointer to record 0 of the strip ABOVE the point's (both rows
//     a candidate can touch lie at offsets >= 0 from there).  The host admits only pairs whose offsets fit
//     (trace_fast_admits, bialign_host.hpp).
//   * Columns whose candidates may touch a non-interior step (strip changes, the first strips, the lattice border: a
//     scalar test on the point) take a side path through packed_addr(), the arithmetic of the generic kernel's packed_cell.
//   * The trace collects in LDS and goes to HBM reversed, by all 64 lanes: at once if it fits the buffer, else in
//     pieces laid from the END of the pair's trace bytes downwards and moved to the front when the length is known.
// ---------------------------------------------------------------------------
template <int S>
struct TraceFast {
  using PK = Pack<S>;
  static constexpr int W = 2 * S + 1, RR = Geo<S>::RR;
  static constexpr int RECB = PK::RECDW * 4;         // bytes of a packed record
  static constexpr int ENTRIES = 9 * W * 16;         // [state][band column l - j + S of the point][candidate]
  static constexpr int TAIL_SHIFT = PK::TAILDW == 2 ? 1 : 2;  // slot * 16 -> slot * TAILDW * 4
  static constexpr uint32_t NONE = 15;               // source-state field of "no candidate"
  // lo: bits 0-3 offset code o0 o1 o2 o3, 4-7 source state (NONE: lane 15, or the band column leaves the band),
  //     8 mu1 enters, 9 mu2 enters, 10-12 / 13-15 look-ahead increments (signed), 16 halfword in the record's tail,
  //     17-18 half (0 low, 1 high, 2: the anchor, no halfword), 19 can_be_empty position, 20-26 what the point must
  //     allow (NEED_*: the guard of pyx:133-141 as one mask test against the column's `deny`).
  // cst: the score's constant part.  da, db: byte offsets of the value's base dword and of its halfword's dword from the
  // column's uniform offsets (Col::u16; Col::u8 for a halfword in the tail).
  struct Entry {
    uint32_t lo;
    int32_t cst, da, db;
  };
  static constexpr int TAB_BYTES = ENTRIES * (int)sizeof(Entry);
  static constexpr uint32_t NEED_I = 1u << 20, NEED_J = 1u << 21, NEED_K = 1u << 22, NEED_L = 1u << 23;  // coordinate >= 1
  static constexpr uint32_t NEED_ALO = 1u << 24, NEED_AHI = 1u << 25;  // the point's band row k - i + S is > 0 / < W - 1
  static constexpr uint32_t NEVER = 1u << 26;
  __host__ __device__ static constexpr int shift_hd(int hU, int hV) { return hU == hV ? 0 : ((hU == 2 || hV == 2) ? 1 : 2); }
  // the generic kernel's per-column expressions (traceback_affine_kernel), for state st, candidate c, band column b0
  __host__ __device__ static inline Entry entry(int st, int b0, int c, int beta, int gamma, int delta) {
    if (c >= 15) return Entry{NEVER | NONE << 4, 0, 0, 0};
    const int hU = st / 3, hV = st - 3 * hU;
    const int u0 = hU >= 1, u1 = hU != 1, v0 = hV >= 1, v1 = hV != 1;
    const int grp = c < 9 ? 1 : (c < 12 ? 2 : 3);
    const int hfree = grp == 2 ? 2 - (c - 9) : 2 - (c - 12);
    const int o0 = grp == 2 ? 0 : u0, o1 = grp == 2 ? 0 : u1;
    const int o2 = grp == 3 ? 0 : v0, o3 = grp == 3 ? 0 : v1;
    const int ss = grp == 1 ? c : (grp == 2 ? 3 * hU + hfree : 3 * hfree + hV);
    const int ra = ss / 3, rb = ss - 3 * ra;
    const int openU = (hU != 2 && ra != hU) ? beta : 0, openV = (hV != 2 && rb != hV) ? beta : 0;
    const int gU = hU == 2 ? 0 : gamma, gV = hV == 2 ? 0 : gamma;  // valU, valV where they are not mu1, mu2
    const int cst = grp == 1   ? delta * shift_hd(hU, hV) + gU + gV + openU + openV
                    : grp == 2 ? delta * (v0 + v1) + gV + openV
                               : delta * (u0 + u1) + gU + openU;
    const uint32_t m1 = grp != 2 && hU == 2, m2 = grp != 3 && hV == 2;
    const int r0 = ra >= 1, r1 = ra != 1, r2 = rb >= 1, r3 = rb != 1;
    const int inc0 = (o0 - o2) + (r0 - r2), inc1 = (o1 - o3) + (r1 - r3);
    const uint32_t code = (uint32_t)(o0 * 8 + o1 * 4 + o2 * 2 + o3);
    const int b = b0 + o1 - o3;  // band column of the candidate's point
    if (b < 0 || b >= W) return Entry{NEVER | NONE << 4 | code, cst, 0, 0};
    const int v = b * 9 + ss, h = PK::hw(v), d = h >> 1;
    const bool anchor = v == PK::ANCHOR, tail = !anchor && d >= 4 * PK::NCH;
    const uint32_t half = anchor ? 2u : (uint32_t)(h & 1);
    const int hpos = anchor ? 0 : (tail ? PK::NCH * Rec<S, 9>::CH + (d - 4 * PK::NCH) : (d >> 2) * Rec<S, 9>::CH + (d & 3));
    const int da = o0 - o2;  // band row of the candidate's point - the point's
    const uint32_t need = (o0 ? NEED_I : 0) | (o1 ? NEED_J : 0) | (o2 ? NEED_K : 0) | (o3 ? NEED_L : 0) | (da < 0 ? NEED_ALO : 0) |
                          (da > 0 ? NEED_AHI : 0);
    const uint32_t lo = code | (uint32_t)ss << 4 | m1 << 8 | m2 << 9 | ((uint32_t)inc0 & 7u) << 10 | ((uint32_t)inc1 & 7u) << 13 |
                        (tail ? 1u : 0u) << 16 | half << 17 | (pack_corner(W, ss, b) ? 1u : 0u) << 19 | need;
    // record t = (j - o1) + 2 (il - o0) + a, slot (il - o0 - 1) W + a, with a = a0 + da: what is left beside the column's part
    const int drec = (da - o1 - 2 * o0) * RECB, dslot16 = (da - o0 * W) * 16;
    return Entry{lo, cst, drec + dslot16, tail ? drec + hpos * 4 + dslot16 / (1 << TAIL_SHIFT) : drec + dslot16 + hpos * 4};
  }
  // what the point forbids: the NEED_* bits no candidate may carry here (i, j, k, l; a0 = k - i + S)
  __host__ __device__ static inline uint32_t deny(int i, int j, int k, int l) {
    const int a0 = k - i + S;
    return NEVER | (i > 0 ? 0 : NEED_I) | (j > 0 ? 0 : NEED_J) | (k > 0 ? 0 : NEED_K) | (l > 0 ? 0 : NEED_L) | (a0 > 0 ? 0 : NEED_ALO) |
           (a0 < W - 1 ? 0 : NEED_AHI);
  }
  // The position the loop carries: row i as (strip, il), and `row`, the byte offset from the pair's storage of record 0 of
  // strip - 1 (negative in strip 0, where no candidate takes the fast path).
  struct Pos {
    int strip, il;
    int64_t row;
    __host__ __device__ static inline Pos at(int i, int P) {
      Pos p;
      p.strip = i / RR;
      p.il = i - p.strip * RR + 1;
      p.row = ((int64_t)p.strip - 1) * P * RECB;
      return p;
    }
    __host__ __device__ inline void step_up(int P) {  // i -> i - 1
      if (--il == 0) {
        il = RR;
        --strip;
        row -= (int64_t)P * RECB;
      }
    }
  };
  // The uniform part of a column at point (i = strip*RR + il - 1, j), band row a0.  fast: every point a candidate can
  // touch lies in an interior step -- rows il and il - 1 (il = 1: row RR of the strip above), columns j - 1 and j, every
  // band row (a bound, a little tighter than needed at il = 1).  u16, u8: byte offsets from `row` that the entries' da / db
  // count from; a candidate with o0 at il = 1 reads row RR of the strip above: up16 / up8 on top.
  struct Col {
    bool fast;
    uint32_t u16, u8;
  };
  __host__ __device__ static inline Col column(int strip, int il, int j, int a0, int P, int m) {
    const bool up = il == 1;
    const int tl = j + 2 * il;
    Col c;
    c.fast = strip - (up ? 1 : 0) >= PK::Q0 && tl >= PK::LO + 3 && tl <= m - S - W + 1 - (up ? 2 * RR - 2 : 0);
    const uint32_t rec = (uint32_t)P * RECB + (uint32_t)(tl + a0) * RECB, slot16 = (uint32_t)(il * W + a0) * 16;
    c.u16 = rec + slot16 - W * 16;
    c.u8 = rec + (slot16 >> TAIL_SHIFT) - ((W * 16) >> TAIL_SHIFT);
    return c;
  }
  __host__ __device__ static inline uint32_t up16(int P) { return (uint32_t)(2 * RR * RECB + RR * W * 16) - (uint32_t)P * RECB; }
  __host__ __device__ static inline uint32_t up8(int P) { return (uint32_t)(2 * RR * RECB + ((RR * W * 16) >> TAIL_SHIFT)) - (uint32_t)P * RECB; }
  // byte offsets, from `row`, of the base dword and of the halfword's dword of a candidate's value on the fast path
  struct Off {
    uint32_t base, word;
  };
  __host__ __device__ static inline Off offsets(const Entry& e, const Col& c, bool up, int P) {
    const bool tail = (e.lo >> 16) & 1;
    Off o{c.u16 + (uint32_t)e.da, (tail ? c.u8 : c.u16) + (uint32_t)e.db};
    if (up && (e.lo & 8)) {
      o.base += up16(P);
      o.word += tail ? up8(P) : up16(P);
    }
    return o;
  }
};

// ---------------------------------------------------------------------------
// The walk's LDS window (traceback_affine_fast_kernel<S, true>).  Seen from a point of lane row il >= 2 at record
// T = j + 2 il + a, slot s = (il - 1) W + a, a column's candidates lie in records T - 3 .. T, slots s - W .. s (Entry:
// record -(o0 + o1 + o2), slot -(W - 1) o0 - o2), and the pick moves the point by just such a candidate step.  So the
// records the next columns read are known before any pick: a ring of the last K records of the strip is filled by LDS-DMA
// D records ahead of T - 3, each record with the WS slots below the walk's slot at the time of issue.  A column all of
// whose records have landed reads base and halfword dword from the ring instead of HBM; every other column (not
// Col::fast, lane row 1, the columns after a strip change) takes the global loads: the window never changes a value,
// only where it is read from.  tests/trace_window_check.hip proves coverage, addresses and the counted waits.
// ---------------------------------------------------------------------------
template <int S>
struct TraceWindow {
  using TF = TraceFast<S>;
  using PK = Pack<S>;
  using R_ = Rec<S, 9>;
  static constexpr int W = TF::W, RECB = TF::RECB;
  static constexpr int RECS_PER_COL = 3;        // a column lowers T by o0 + o1 + o2 <= 3 ...
  static constexpr int SPAN = RECS_PER_COL + 1; // ... and its candidates lie in that many records, T - 3 .. T
  static constexpr int WS = S == 1 ? 16 : 32;   // slots of a window record: slot sl sits at position sl mod WS (s=1: one DMA instruction per record)
  // How far the slot can fall while T falls by x records: x = x1 + 2 x0 - da and slot change = -W x0 + da for x0 rows up,
  // x1 columns left and a band-row change da <= W - 1, so the slot falls by at most W x / 2 + (W - 1)(W - 2) / 2; it never rises.
  __host__ __device__ static constexpr int drift(int x) { return (W * x + 1) / 2 + (W - 1) * (W - 2) / 2; }
  // A record issued at (T, s) is at most D + 3 records below T and is read until T has fallen to it: the slots
  // s - drift(D + 3) - W .. s must fit into WS, less one for the even start (the tail piece is 16 bytes = two slots).
  __host__ __device__ static constexpr int lead_max() {
    int d = -1;
    while (drift(d + 1 + RECS_PER_COL) + W + 2 <= WS) ++d;
    return d;
  }
  static constexpr int D = lead_max() < 4 ? lead_max() : 4;  // records of lead below T - 3 (s=1: 3, s=2: 4, s=3: none)
  static constexpr bool EXISTS = D >= 0 && (PK::TAILDW == 0 || PK::TAILDW == 2);
  static constexpr int K = 8, KMIN = SPAN;      // ring records (a power of two >= lead + SPAN); KMIN: no lead (tests)
  static_assert(!EXISTS || (K >= D + SPAN && (K & (K - 1)) == 0 && (KMIN & (KMIN - 1)) == 0), "ring too short for the lead");
  static_assert(!EXISTS || WS <= R_::SLP, "a window record is wider than a record");
  // 16-byte pieces of a window record: NCH chunks of WS slots, then the tails of WS slots; whole DMA instructions
  static constexpr int NPIECE16 = PK::NCH * WS + WS * PK::TAILDW / 4;
  static constexpr int NDMA = (NPIECE16 + 63) / 64;
  static constexpr int RB = NDMA * 1024;        // bytes of a window record
  static constexpr int TAIL_AT = PK::NCH * WS * 16;
  static constexpr int WTAB_BYTES = TF::ENTRIES * 4;
  __host__ __device__ static constexpr int lds_bytes(int k) { return WTAB_BYTES + k * RB; }
  __host__ __device__ static constexpr int lead(int k) { return k - SPAN < D ? k - SPAN : D; }  // ... of a ring of k records
  // first slot of the record issued while the walk stands at slot s (even, >= 0; s <= SL - 1 keeps it <= SLP - WS)
  __host__ __device__ static inline int slot_lo(int s) {
    const int lo = (s + 2 - WS) & ~1;
    return lo > 0 ? lo : 0;
  }
  // Source of lane `lane` of DMA instruction d: byte offset from the record's start = base + (slot << sh), with
  // slot = slo + ((u - slo) mod WS), the slot of slo .. slo + WS - 1 that sits at position u.  The tail's lanes move two
  // slots (u even, sh = 3); the surplus lanes of the last instruction repeat its last useful lane.
  struct LaneSrc {
    uint32_t base, u, sh;
  };
  __host__ __device__ static inline LaneSrc lane_src(int d, int lane) {
    const int q = d * 64 + lane < NPIECE16 ? d * 64 + lane : NPIECE16 - 1;
    const int p = q / WS, u = q - p * WS;
    if (p < PK::NCH) return LaneSrc{(uint32_t)(p * R_::CH * 4), (uint32_t)u, 4u};
    return LaneSrc{(uint32_t)(PK::NCH * R_::CH * 4), (uint32_t)(2 * u), 3u};
  }
  __host__ __device__ static inline uint32_t src_off(const LaneSrc& c, int slo) {
    return c.base + (((uint32_t)slo + ((c.u - (uint32_t)slo) & (WS - 1))) << c.sh);
  }
  __host__ __device__ static inline uint32_t ring_byte(int r, int k) { return (uint32_t)(r & (k - 1)) * RB; }
  // What a candidate adds to the column's (T, s): bits 0-11 byte offset of its halfword's dword in a window record at
  // position 0, 16-17 records below T, 20-23 slots below s.  (Tail or not: Entry::lo bit 16.)
  __host__ __device__ static inline uint32_t wentry(int st, int b0, int c) {
    if (c >= 15) return 0;
    const typename TF::Entry e = TF::entry(st, b0, c, 0, 0, 0);
    if (((e.lo >> 4) & 15) == TF::NONE) return 0;
    const int o0 = (e.lo >> 3) & 1, o1 = (e.lo >> 2) & 1, o2 = (e.lo >> 1) & 1, o3 = e.lo & 1;
    const int v = (b0 + o1 - o3) * 9 + (int)((e.lo >> 4) & 15);
    uint32_t woff = 0;
    if (v != PK::ANCHOR) {
      const int d = PK::hw(v) >> 1;
      woff = d >= 4 * PK::NCH ? TAIL_AT + (d - 4 * PK::NCH) * 4 : (d >> 2) * WS * 16 + (d & 3) * 4;
    }
    return woff | (uint32_t)(o0 + o1 + o2) << 16 | (uint32_t)((W - 1) * o0 + o2) << 20;
  }
  // byte offsets, in the ring, of a candidate's base dword and of its halfword's dword for a column at (T, s)
  __host__ __device__ static inline typename TF::Off addr(uint32_t we, bool tail, int T, int s, int k) {
    const uint32_t ring = ring_byte(T - (int)((we >> 16) & 3), k), u = (uint32_t)(s - (int)((we >> 20) & 15)) & (WS - 1);
    return typename TF::Off{ring + u * 16, ring + (we & 0xfffu) + (tail ? u * 8 : u * 16)};
  }
  // The records a column at T reads have landed when at most this many of the wave's DMA instructions are outstanding:
  // those of the records below T - 3, issued later (vector memory operations retire in order).  The kernel has two waits:
  // the full lead's, which is every column's but for the last ones above record 0 and for a short ring (tests), and 0.
  __host__ __device__ static inline bool full_lead(int T, int next) { return T - RECS_PER_COL - next == D; }
  __host__ __device__ static inline int may_pend(int T, int next) { return full_lead(T, next) ? D * NDMA : 0; }
};

template <int N>
__device__ __forceinline__ void trace_window_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int S, bool WIN = false>
__global__ void __launch_bounds__(64) traceback_affine_fast_kernel(const DeviceBatch A, int npairs, int tbuf_bytes, int wk) {
  using TF = TraceFast<S>;
  using TW = TraceWindow<S>;
  static_assert(!WIN || TW::EXISTS, "no window at this max_shift");
  typedef typename TF::Entry Entry;
  const int pid = A.order[blockIdx.x];
  const PairDesc pd = A.pairs[pid];
  const int n = pd.n, m = pd.m, P = pd.P, cap = pd.trace_cap;
  const int c = threadIdx.x;
  constexpr int BIG = 0x7fffffff;
  constexpr int W = TF::W, RR = TF::RR;
  extern __shared__ __align__(16) int32_t smem[];
  const int32_t* const pbase = A.layers + pd.layer_off;

  // pyx:573-582: best end layer, first one with the least shift
  const int endv = c < 9 ? packed_cell<S>(A.layers, pd, n, m, S, S, c) : -BIG;
  const int best = __builtin_amdgcn_readfirstlane(-wave_min16(-endv));
  if (c == 0) A.scores[pid] = best;
  const int skey = (c < 9 && endv == best) ? (shift_of(c / 3, c % 3) << 4 | c) : BIG;
  int st = __builtin_amdgcn_readfirstlane(wave_min16(skey)) & 15;
  int cur = best;

  const TraceInputs in = stage_trace_inputs<false>(A, pd, smem);
  const int staged = ((A.k1 * A.k1 + A.k2 * A.k2) * 4 + 2 * (code_pad(n) + code_pad(m)) + 15) & ~15;
  Entry* const tab = reinterpret_cast<Entry*>(reinterpret_cast<char*>(smem) + staged);
  // WIN: the window's candidate table and its ring of wk records lie between the table and the trace buffer
  uint32_t* const wtab = reinterpret_cast<uint32_t*>(tab + TF::ENTRIES);
  const char* const wring = reinterpret_cast<const char*>(wtab + TF::ENTRIES);
  uint8_t* const tbuf = WIN ? reinterpret_cast<uint8_t*>(const_cast<char*>(wring) + wk * TW::RB) : reinterpret_cast<uint8_t*>(tab + TF::ENTRIES);
  for (int e = c; e < TF::ENTRIES; e += 64) tab[e] = TF::entry(e / (16 * W), (e >> 4) % W, e & 15, A.beta, A.gamma, A.delta);
  if constexpr (WIN)
    for (int e = c; e < TF::ENTRIES; e += 64) wtab[e] = TW::wentry(e / (16 * W), (e >> 4) % W, e & 15);
  __syncthreads();

  uint8_t* const out = A.trace + pd.trace_off;
  int i = n, j = m, k = n, l = m, d0 = 0, d1 = 0, len = 0, complete = 0, flushed = 0;
  typename TF::Pos pos = TF::Pos::at(n, P);
  const char* rowp = reinterpret_cast<const char*>(pbase) + pos.row;
  const uint32_t prb = (uint32_t)P * TF::RECB, up16 = TF::up16(P), up8 = TF::up8(P);
  const Entry* const tabc = tab + (c < 15 ? c : 15);  // lanes beyond the candidates read the "no candidate" entry
  const int k1 = A.k1, k2 = A.k2;
  // A zero the compiler cannot see through, added to the (uniform) LDS addresses of mu1 and mu2: they stay vector reads in
  // flight behind the global loads; as scalars their bytes would be waited for and read back ahead of the loads.
  int vz = 0;
  asm volatile("" : "+v"(vz));
  // columns until the buffer is full or the trace reaches trace_cap
  int room = min(tbuf_bytes, cap);
  // columns flushed .. flushed + cnt - 1 (walk order) from the LDS buffer to the end of the pair's trace bytes, downwards
  auto flush = [&](int cnt) {
    __syncthreads();
    for (int y = c; y < cnt; y += 64) out[cap - 1 - flushed - y] = tbuf[y];
    __syncthreads();
    flushed += cnt;
  };
  // WIN: records wnext .. (the record the strip's window began at) of the strip are in the ring or on their way, issued in
  // falling order; wlive is false from a strip change until the next pick that leaves the walk in a lane row >= 2.
#if defined(BIALIGN_EXP) && BIALIGN_EXP == 10
  int whits = 0;  // columns served from the window, reported in place of the pair's score (tools/trace_window_share.py)
#endif
  [[maybe_unused]] int wnext = 0;
  [[maybe_unused]] bool wlive = false;
  [[maybe_unused]] const int wlead = TW::lead(wk);
  [[maybe_unused]] const uint32_t wlds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int32_t*)smem + (uint32_t)(wring - reinterpret_cast<const char*>(smem));
  [[maybe_unused]] typename TW::LaneSrc wsrc[TW::NDMA];
  if constexpr (WIN) {
#pragma unroll
    for (int d = 0; d < TW::NDMA; ++d) wsrc[d] = TW::lane_src(d, c);
  }
  // the DMAs of record r of the walk's strip, for a walk at slot s (the ghost feed's form: scalar base, lane offsets, m0)
  [[maybe_unused]] auto wissue = [&](int r, int s) {
    const char* const base = rowp + prb + (uint32_t)r * (uint32_t)TF::RECB;
    const uint32_t dst0 = wlds + TW::ring_byte(r, wk);
    const int slo = TW::slot_lo(s);
#pragma unroll
    for (int d = 0; d < TW::NDMA; ++d) {
      const uint32_t off = TW::src_off(wsrc[d], slo), dst = dst0 + d * 1024;
      uint32_t keep;
      asm volatile(
          "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
          "global_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
          : "=&s"(keep)
          : "v"(off), "s"(dst), "s"(base)
          : "memory");
    }
  };
  while (true) {
    if ((i | j | k | l | (st ^ 8)) == 0) { complete = 1; break; }
    const Entry E = tabc[(st * W + (l - j + S)) * 16];
    [[maybe_unused]] uint32_t we = 0;
    if constexpr (WIN) we = (wtab + (c < 15 ? c : 15))[(st * W + (l - j + S)) * 16];
    // code bytes and table values of mu1, mu2 (uniform addresses): waited for where sc is formed
    int ca = in.sa[i - 1 + vz], cb = in.sb[j - 1 + vz], cc = in.ca[k - 1 + vz], cd = in.cb[l - 1 + vz];  // (index -1: inside the staged arrays' LDS, unused)
    const uint32_t lo = E.lo;
    const int a0 = k - i + S;
    uint32_t deny = TF::NEVER | (a0 > 0 ? 0 : TF::NEED_ALO) | (a0 < W - 1 ? 0 : TF::NEED_AHI);
    const bool edge = min(min(i, j), min(k, l)) == 0;  // a coordinate at 0: the last columns of a walk
    if (edge) deny = TF::deny(i, j, k, l);
    const bool ok = (lo & deny) == 0;  // pyx:133-141
    const typename TF::Col col = TF::column(pos.strip, pos.il, j, a0, P, m);
    int ld = 0;
    auto value = [&](int base, uint32_t word) {
      const uint32_t half = (lo >> 17) & 3;
      const uint32_t e = Pack<S>::offset_of(half == 1 ? word >> 16 : word & 0xffffu, base);
      int v = base + (int)e;
      if (((lo >> 19) & 1) && e == 0xffffu) v = NEG;
      if (half == 2) v = base + 0x8000;
      return v;
    };
    [[maybe_unused]] bool hit = false;
    [[maybe_unused]] const int wT = j + 2 * pos.il + a0;
    if constexpr (WIN) hit = col.fast && wlive && pos.il >= 2 && wT - TW::RECS_PER_COL >= wnext;
    if (WIN && hit) {  // every candidate's record is in the ring once the DMAs of the records below T - 3 alone are pending
      if constexpr (WIN) {
#if defined(BIALIGN_EXP) && BIALIGN_EXP == 10
        ++whits;
#endif
        if (TW::full_lead(wT, wnext)) trace_window_wait<TW::D * TW::NDMA>();
        else trace_window_wait<0>();
        if (ok) {
          const typename TF::Off o = TW::addr(we, (lo >> 16) & 1, wT, (pos.il - 1) * W + a0, wk);
          ld = value(*reinterpret_cast<const int32_t*>(wring + o.base), *reinterpret_cast<const uint32_t*>(wring + o.word));
        }
      }
    } else if (col.fast) {
      if (ok) {
        const bool tail = (lo >> 16) & 1;
        uint32_t ob = col.u16 + (uint32_t)E.da, ow = (tail ? col.u8 : col.u16) + (uint32_t)E.db;
        if (pos.il == 1 && (lo & 8)) {  // row RR of the strip above
          ob += up16;
          ow += tail ? up8 : up16;
        }
        ld = value(*reinterpret_cast<const int32_t*>(rowp + ob), *reinterpret_cast<const uint32_t*>(rowp + ow));
      }
    } else if (ok) {  // a candidate may lie in a full record: packed_cell's own arithmetic
      const int o0 = (lo >> 3) & 1, o1 = (lo >> 2) & 1, o2 = (lo >> 1) & 1, o3 = lo & 1;
      ld = packed_load<S>(pbase, packed_addr<S>(pd, i - o0, j - o1, a0 + o0 - o2, (l - j + S) + o1 - o3, (lo >> 4) & 15));
      // WIN: a use here, so that hipcc waits for these loads inside this path; left pending (in its model) where the path
      // joins the others, the next write of their register drew a vmcnt(0) into the window's path, and with it every DMA
      if constexpr (WIN) asm volatile("" ::"v"(ld));
    }
    bool z1 = false, z2 = false;
    if (edge) {
      z1 = i < 1 || j < 1;
      z2 = k < 1 || l < 1;
      if (z1) ca = cb = 0;
      if (z2) cc = cd = 0;
    }
    int mu1 = in.s1[__umul24(ca, k1) + cb], mu2 = in.s2[__umul24(cc, k2) + cd];
    if (z1) mu1 = 0;
    if (z2) mu2 = 0;
    const int sc = E.cst + (((lo >> 8) & 1) ? mu1 : 0) + (((lo >> 9) & 1) ? mu2 : 0);
    // pyx:554-565: cases reproducing the cell; look-ahead adds the offset AND the source state
    const int t0 = d0 + ((int)(lo << 19) >> 29), t1 = d1 + ((int)(lo << 16) >> 29);
    const int key = (ok && ld + sc == cur) ? ((abs(t0) + abs(t1)) << 16 | abs(t1) << 8 | c) : BIG;
    const int kmin = __builtin_amdgcn_readfirstlane(wave_min16(key));
    if (kmin == BIG) break;  // pyx:570-571 -> "incomplete traceback"
    const int pick = kmin & 63;
    const int cs = __builtin_amdgcn_readlane((int)lo, pick);  // code and source state in one register
    cur = __builtin_amdgcn_readlane(ld, pick);
    st = (cs >> 4) & 15;
    const int q0 = (cs >> 3) & 1, q1 = (cs >> 2) & 1, q2 = (cs >> 1) & 1, q3 = cs & 1;
    d0 += q0 - q2;  // pyx:566: only the offset moves the running shift
    d1 += q1 - q3;
    if (room > 0) {  // (0 for good once the trace has reached trace_cap)
      if (c == 0) tbuf[len - flushed] = (uint8_t)(cs & 15);
      if (--room == 0) {
        if (len + 1 - flushed == tbuf_bytes) flush(tbuf_bytes);
        room = min(tbuf_bytes, cap - (len + 1));
      }
    }
    ++len;
    i -= q0; j -= q1; k -= q2; l -= q3;
    if (q0) {
      const int strip_was = pos.strip;
      pos.step_up(P);
      if (pos.strip != strip_was) {
        rowp -= prb;
        if constexpr (WIN) wlive = false;  // the ring holds the strip below's records
      }
    }
    if constexpr (WIN) {  // the records that entered the lead range, at most three but for the strip's first fill
      const int a1 = k - i + S, Tn = j + 2 * pos.il + a1;
      if (!wlive && pos.il >= 2) {
        wlive = true;
        wnext = Tn + 1;
      }
      if (wlive) {
        const int low = max(Tn - TW::RECS_PER_COL - wlead, 0);
        for (int r = wnext - 1; r >= low; --r) wissue(r, (pos.il - 1) * W + a1);
        wnext = min(wnext, low);
      }
    }
  }
  if constexpr (WIN) trace_window_wait<0>();  // no DMA lands in LDS after the wave has ended
  if (len > cap) len = cap;
  if (flushed == 0) {  // the whole trace is in LDS: reversed (pyx:586) and coalesced
    __syncthreads();
    for (int x = c; x < len; x += 64) out[x] = tbuf[len - 1 - x];
  } else {
    flush(len - flushed);
    const int sh = cap - len;  // the trace sits in out[sh .. cap), already reversed: move it to the front
    if (sh > 0) {
      __builtin_amdgcn_s_waitcnt(0);  // the flushes' stores before the loads
      __syncthreads();
      for (int x0 = 0; x0 < len; x0 += 64) {  // a position is read (at x0 = its index - sh) before it is written
        const int x = x0 + c;
        const uint8_t t = x < len ? out[sh + x] : 0;
        if (x < len) out[x] = t;
      }
    }
  }
  if (c == 0) {
    A.trace_len[pid] = len;
    A.complete[pid] = complete;
#if defined(BIALIGN_EXP) && BIALIGN_EXP == 10
    if constexpr (WIN) A.scores[pid] = whits;
#endif
  }
}

}  // namespace bialign
