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

template <int S>
__global__ void __launch_bounds__(64) traceback_affine_fast_kernel(const DeviceBatch A, int npairs, int tbuf_bytes) {
  using TF = TraceFast<S>;
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
  uint8_t* const tbuf = reinterpret_cast<uint8_t*>(tab + TF::ENTRIES);
  for (int e = c; e < TF::ENTRIES; e += 64) tab[e] = TF::entry(e / (16 * W), (e >> 4) % W, e & 15, A.beta, A.gamma, A.delta);
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
  while (true) {
    if ((i | j | k | l | (st ^ 8)) == 0) { complete = 1; break; }
    const Entry E = tabc[(st * W + (l - j + S)) * 16];
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
    if (col.fast) {
      if (ok) {
        const bool tail = (lo >> 16) & 1;
        uint32_t ob = col.u16 + (uint32_t)E.da, ow = (tail ? col.u8 : col.u16) + (uint32_t)E.db;
        if (pos.il == 1 && (lo & 8)) {  // row RR of the strip above
          ob += up16;
          ow += tail ? up8 : up16;
        }
        const int base = *reinterpret_cast<const int32_t*>(rowp + ob);
        const uint32_t word = *reinterpret_cast<const uint32_t*>(rowp + ow);
        const uint32_t half = (lo >> 17) & 3;
        const uint32_t e = Pack<S>::offset_of(half == 1 ? word >> 16 : word & 0xffffu, base);
        ld = base + (int)e;
        if (((lo >> 19) & 1) && e == 0xffffu) ld = NEG;
        if (half == 2) ld = base + 0x8000;
      }
    } else if (ok) {  // a candidate may lie in a full record: packed_cell's own arithmetic
      const int o0 = (lo >> 3) & 1, o1 = (lo >> 2) & 1, o2 = (lo >> 1) & 1, o3 = lo & 1;
      ld = packed_load<S>(pbase, packed_addr<S>(pd, i - o0, j - o1, a0 + o0 - o2, (l - j + S) + o1 - o3, (lo >> 4) & 15));
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
      if (pos.strip != strip_was) rowp -= prb;
    }
  }
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
  }
}

}  // namespace bialign
