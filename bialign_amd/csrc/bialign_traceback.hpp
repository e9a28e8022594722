// bialign_traceback.hpp -- tracebacks of both recurrences.  Part of bialign_kernels.hpp (include that, not this).
#pragma once

namespace bialign {

// |U0-V0| + |U1-V1| of a column / state given its two halves (pyx:97, 541-545)
__host__ __device__ __forceinline__ int shift_of(int hU, int hV) {
  return hU == hV ? 0 : ((hU == 2 || hV == 2) ? 1 : 2);
}

// ---------------------------------------------------------------------------
// Affine traceback (pyx:535-586).  One wave per pair: lane c < 15 owns candidate
// c of the case generator's order (pyx:275-296) -- nine sources of the full
// offset, then three of the structure-only and three of the sequence-only offset
// -- so a column costs one HBM round trip and a handful of instructions.  The
// tie-break of pyx:554-565 ("first candidate minimising [|d0|+|d1|, |d1|]" with
// the source state added as a one-step look-ahead) is a wave-min over the packed
// key (|d0|+|d1|, |d1|, c).
// ---------------------------------------------------------------------------
// Score tables and the pair's sequence codes staged in LDS for the tracebacks (every
// column needs mu1, mu2: two dependent global loads otherwise).
struct TraceInputs {
  const int32_t *s1, *s2;
  const uint8_t *sa, *ca, *sb, *cb;
};
// D1 (dense mu1): the sequence codes are not staged (sa, sb are then unused).
template <bool D1 = false>
__device__ __forceinline__ TraceInputs stage_trace_inputs(const DeviceBatch& A, const PairDesc& pd,
                                                          int32_t* smem) {
  const int k1 = A.k1, k2 = A.k2, n = pd.n, m = pd.m;
  int32_t* s1 = smem;
  int32_t* s2 = s1 + k1 * k1;
  uint8_t* sa = reinterpret_cast<uint8_t*>(s2 + k2 * k2);
  uint8_t* ca = sa + (D1 ? 0 : code_pad(n));
  uint8_t* sb = ca + code_pad(n);
  uint8_t* cb = sb + (D1 ? 0 : code_pad(m));
  for (int t = threadIdx.x; t < k1 * k1; t += 64) s1[t] = A.s1[t];
  for (int t = threadIdx.x; t < k2 * k2; t += 64) s2[t] = A.s2[t];
  for (int t = threadIdx.x; t < n; t += 64) {
    if (!D1) sa[t] = A.seq_a[pd.seq_a + t];
    ca[t] = A.cls_a[pd.seq_a + t];
  }
  for (int t = threadIdx.x; t < m; t += 64) {
    if (!D1) sb[t] = A.seq_b[pd.seq_b + t];
    cb[t] = A.cls_b[pd.seq_b + t];
  }
  __syncthreads();
  return TraceInputs{s1, s2, sa, ca, sb, cb};
}

__device__ __forceinline__ int wave_min16(int v) {  // min over lanes 0..15, valid in every lane < 16
  // four DPP row rotations (a row = 16 lanes) instead of four trips through the LDS crossbar
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x128 /* row_ror:8 */, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x124 /* row_ror:4 */, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x122 /* row_ror:2 */, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x121 /* row_ror:1 */, 0xf, 0xf, false));
  return v;
}
__device__ __forceinline__ int wave_min64(int v) {  // min over the wave's 64 lanes (all active), wave-uniform
  v = wave_min16(v);  // every row of 16 lanes reduces by itself
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// Fit and overlap alignments (DeviceBatch::free_ends), end rule of the full-storage tracebacks.  The end cells in position
// order: x < n -> (x, m), else (n, x - n), for x = 0 .. n + m; that is the order by (i, j), and the order of end_key_of.
// An overlap batch takes all of them, a fit batch those of row n (x >= n).  The wave's lanes stride over the positions,
// read each cell's value through the kernel's own cell addressing (end_cell(i, j)), and reduce to the best one and the
// smallest position that attains it.  Column m and row n are scanned by a loop each, so that a fit batch runs the loop
// over row n it always ran (its row is loop-invariant); a lane meets its positions in rising order in both.
template <typename EndCell>
__device__ __forceinline__ void free_end_scan(int n, int m, bool a_ends, int lane, EndCell&& end_cell, int* end_a, int* end_b) {
  constexpr int BIG = 0x7fffffff;
  int bv = -BIG, bx = 0;
  if (a_ends) {
    for (int x = lane; x < n; x += 64) {
      const int e = end_cell(x, m);
      if (e > bv) bv = e, bx = x;
    }
  }
  for (int j = lane; j <= m; j += 64) {
    const int e = end_cell(n, j);
    if (e > bv) bv = e, bx = n + j;
  }
  const int best = -wave_min64(-bv);
  const int x = wave_min64(bv == best ? bx : BIG);
  *end_a = x < n ? x : n;
  *end_b = x < n ? m : x - n;
}

// ---------------------------------------------------------------------------
// The walk as device functions: start point in, (end point, len, how it ended) out.  A walk stands on lattice point
// (i, j, k, l) in state st (affine) with layer value cur, running shifts (d0, d1), len columns emitted.  The hit search
// (bialign_hits.hpp) walks several ends per pair through them, and the traceback kernels below walk one.  The rules of
// the walk -- the scores of a point, the affine candidates, tie-break and stop rules, free ends, the trace's reversal --
// are stated here once, and the kernels keep what is theirs (the TraceState of the continuing forms, their cell
// addressing, staging, publishing).  One copy is left: traceback_linear_kernel holds the text of walk_linear's column
// loop itself, because it ran slower with the call (DESIGN.md section 7f has the device code and the times).
// ---------------------------------------------------------------------------
struct WalkPoint {
  int i, j, k, l, st, cur, d0, d1, len;
};
enum : int { WALK_INCOMPLETE = 0, WALK_COMPLETE = 1, WALK_LEFT = 2 };  // LEFT: `leave` said so (STRIP, LEVEL: next round)

// mu1 at (i, j) and mu2 at (k, l), 0 on the lattice's edge: LOOKUP through the staged tables and codes, dense from the
// pair's tables (D1: dense mu1, and mu2 dense if dense_forms says so; else mu2 dense if the batch has a table).
struct PointScores {
  int mu1, mu2;
};
template <bool D1>
__device__ __forceinline__ PointScores point_scores(const DeviceBatch& A, const PairDesc& pd, const TraceInputs& in,
                                                    const int32_t* mu1tab, int i, int j, int k, int l) {
  const int m = pd.m;
  const int mu1 = (i >= 1 && j >= 1)
                      ? (D1 ? mu1tab[(int64_t)(i - 1) * m + (j - 1)] : in.s1[in.sa[i - 1] * A.k1 + in.sb[j - 1]])
                      : 0;
  const int mu2 = (k >= 1 && l >= 1)
                      ? ((D1 ? (A.dense_forms & 1) != 0 : A.dense_tab != nullptr)
                             ? A.dense_tab[pd.tab_off + (int64_t)(k - 1) * m + (l - 1)]
                             : in.s2[in.ca[k - 1] * A.k2 + in.cb[l - 1]])
                      : 0;
  return PointScores{mu1, mu2};
}

// Candidate c < 15 of a point in state st (pyx:84-131, the generator's order of pyx:275-296): its offset (o0..o3), source
// state ss, score sc given the point's mu1 / mu2, and what offset and source state add to the running shifts for the
// look-ahead of pyx:554-565.  Host code too: tests/trace_fast_check.hip holds the short-chain kernel's table against it.
struct AffineCandidate {
  int o0, o1, o2, o3, ss, sc, inc0, inc1;
};
__host__ __device__ __forceinline__ AffineCandidate affine_candidate(int st, int c, int beta, int gamma, int delta, int mu1, int mu2) {
  // lane-constant part of the candidate: its group (full, structure-only, sequence-only offset) and, for groups 2/3,
  // the free half h.  The groups are predicates of c, not a number: a number stays live in the kernels' column loop.
  const bool grp1 = c < 9, grp2 = c >= 9 && c < 12, grp3 = c >= 12;
  const int hfree = grp2 ? 2 - (c - 9) : 2 - (c - 12);  // h = M, X, Y in the generator's order
  const int hU = st / 3, hV = st - 3 * hU;
  const int u0 = hU >= 1, u1 = hU != 1, v0 = hV >= 1, v1 = hV != 1;
  const int valU = hU == 2 ? mu1 : gamma, valV = hV == 2 ? mu2 : gamma;
  AffineCandidate g;
  g.o0 = grp2 ? 0 : u0, g.o1 = grp2 ? 0 : u1;
  g.o2 = grp3 ? 0 : v0, g.o3 = grp3 ? 0 : v1;
  g.ss = grp1 ? c : (grp2 ? 3 * hU + hfree : 3 * hfree + hV);
  const int ra = g.ss / 3, rb = g.ss - 3 * ra;
  const int openU = (hU != 2 && ra != hU) ? beta : 0, openV = (hV != 2 && rb != hV) ? beta : 0;
  g.sc = grp1   ? delta * shift_of(hU, hV) + valU + valV + openU + openV
         : grp2 ? delta * (v0 + v1) + valV + openV
                : delta * (u0 + u1) + valU + openU;
  const int r0 = ra >= 1, r1 = ra != 1, r2 = rb >= 1, r3 = rb != 1;
  g.inc0 = (g.o0 - g.o2) + (r0 - r2), g.inc1 = (g.o1 - g.o3) + (r1 - r3);
  return g;
}

// Start of a walk in the free-end modes: the end that end_key_finish_kernel decoded (LOCAL), or the best end cell by
// free_end_scan over end_value(i, j), the kernel's best layer value at (i, j, i, j) (FIT, OVERLAP); the spans are set to
// (start -1, the end) in the mode's layout.  A global batch leaves (*end_a, *end_b) alone.
template <typename EndValue>
__device__ __forceinline__ void free_end_start(const DeviceBatch& A, int pid, int n, int m, bool fit, bool ovl, bool local, int c,
                                               EndValue&& end_value, int* end_a, int* end_b) {
  if (local) {
    *end_a = A.span[4 * (int64_t)pid + 1];
    *end_b = A.span[4 * (int64_t)pid + 3];
  }
  if (fit) {
    free_end_scan(n, m, ovl, c, end_value, end_a, end_b);
    if (c == 0 && !ovl) {
      A.span[2 * pid] = -1;
      A.span[2 * pid + 1] = *end_b;
    }
    if (c == 0 && ovl) {  // (start_a, end_a, start_b, end_b), as end_key_finish_kernel leaves them
      int32_t* span = A.span + 4 * (int64_t)pid;
      span[0] = -1, span[1] = *end_a, span[2] = -1, span[3] = *end_b;
    }
  }
}
// ... and its other end: a complete walk that stopped on the free start (i, j, i, j) publishes it (one lane calls this).
// One test per mode: `ovl || local` is a third flag that lives through the column loop, two SGPRs that take the packed
// affine kernels from 100 to 102 and so from eight waves to seven.
__device__ __forceinline__ void publish_free_starts(const DeviceBatch& A, int pid, bool fit, bool ovl, bool local, int i, int j) {
  if (fit && !ovl) A.span[2 * pid] = j;
  if (ovl) A.span[4 * (int64_t)pid] = i, A.span[4 * (int64_t)pid + 2] = j;
  if (local) A.span[4 * (int64_t)pid] = i, A.span[4 * (int64_t)pid + 2] = j;
}

// pyx:586 reversed: lane 0 stored the columns end -> start; the wave swaps them into start -> end order in place
__device__ __forceinline__ void reverse_trace(uint8_t* out, int len, int c) {
  __builtin_amdgcn_s_waitcnt(0);  // lane 0's byte stores before the wave-wide reversal
  __syncthreads();
  for (int x = c; x < len / 2; x += 64) {
    const uint8_t t = out[x];
    out[x] = out[len - 1 - x];
    out[len - 1 - x] = t;
  }
}

// pyx:573-582: the best end layer at (i, j, i, j), and the first state with the least shift that attains it
template <typename Cell>
__device__ __forceinline__ void affine_end_state(Cell&& cell, int i, int j, int SR, int c, int* best_out, int* st_out) {
  constexpr int BIG = 0x7fffffff;
  const int endv = c < 9 ? cell(i, j, SR, SR, c) : -BIG;
  const int best = __builtin_amdgcn_readfirstlane(-wave_min16(-endv));
  const int skey = (c < 9 && endv == best) ? (shift_of(c / 3, c % 3) << 4 | c) : BIG;
  *st_out = __builtin_amdgcn_readfirstlane(wave_min16(skey)) & 15;
  *best_out = best;
}

// Affine walk (pyx:535-586) from w to its end: lane c < 15 owns candidate c, lane 0 writes the columns end -> start into
// out[0 .. cap).  cell(pi, pj, a, b, ss) reads a layer value, leave(i, j, k, l) ends a round of the continuing forms.
template <bool D1, typename Cell, typename Leave>
__device__ __forceinline__ int walk_affine(const DeviceBatch& A, const PairDesc& pd, const TraceInputs& in, const int32_t* mu1tab,
                                           int SR, int c, bool fit, bool ovl, bool local, Cell&& cell, Leave&& leave,
                                           uint8_t* out, int cap, WalkPoint& w) {
  constexpr int BIG = 0x7fffffff;
  const int beta = A.beta, gamma = A.gamma, delta = A.delta;
  int i = w.i, j = w.j, k = w.k, l = w.l, st = w.st, cur = w.cur, d0 = w.d0, d1 = w.d1, len = w.len;
  int how = WALK_INCOMPLETE;
  while (true) {
    if (i == 0 && j == 0 && k == 0 && l == 0 && st == 8) { how = WALK_COMPLETE; break; }
    if (fit && i == 0 && k == 0 && j == l && st == 8 && cur == 0) { how = WALK_COMPLETE; break; }  // fit: a free start, start_b = j
    if (ovl && j == 0 && l == 0 && i == k && st == 8 && cur == 0) { how = WALK_COMPLETE; break; }  // overlap: and on column 0, start_a = i
    if (local && i == k && j == l && st == 8 && cur == 0) { how = WALK_COMPLETE; break; }  // local: a free start, (start_a, start_b) = (i, j)
    if (leave(i, j, k, l)) { how = WALK_LEFT; break; }
    const PointScores mu = point_scores<D1>(A, pd, in, mu1tab, i, j, k, l);
    const AffineCandidate g = affine_candidate(st, c, beta, gamma, delta, mu.mu1, mu.mu2);  // this lane's candidate
    const int pi = i - g.o0, pj = j - g.o1, pk = k - g.o2, pl = l - g.o3;
    const bool ok = c < 15 && pi >= 0 && pj >= 0 && pk >= 0 && pl >= 0 && abs(pk - pi) <= SR &&
                    abs(pl - pj) <= SR;  // pyx:133-141
    const int ld = ok ? cell(pi, pj, pk - pi + SR, pl - pj + SR, g.ss) : 0;
    // pyx:554-565: cases reproducing the cell; look-ahead adds the offset AND the source state
    const int t0 = d0 + g.inc0, t1 = d1 + g.inc1;
    const int key = (ok && ld + g.sc == cur) ? ((abs(t0) + abs(t1)) << 16 | abs(t1) << 8 | c) : BIG;
    const int kmin = __builtin_amdgcn_readfirstlane(wave_min16(key));
    if (kmin == BIG) break;  // pyx:570-571 -> "incomplete traceback"
    const int pick = kmin & 63;
    const int code = __builtin_amdgcn_readlane(g.o0 * 8 + g.o1 * 4 + g.o2 * 2 + g.o3, pick);
    st = __builtin_amdgcn_readlane(g.ss, pick);
    cur = __builtin_amdgcn_readlane(ld, pick);
    const int q0 = (code >> 3) & 1, q1 = (code >> 2) & 1, q2 = (code >> 1) & 1, q3 = code & 1;
    d0 += q0 - q2;  // pyx:566: only the offset moves the running shift
    d1 += q1 - q3;
    if (c == 0 && len < cap) out[len] = (uint8_t)code;
    ++len;
    i -= q0; j -= q1; k -= q2; l -= q3;
  }
  w = WalkPoint{i, j, k, l, st, cur, d0, d1, len};
  return how;
}

// Non-affine walk (pyx:513-531): lane c < 13 = case c; it ends, complete, when no case reproduces the cell (the origin)
// or on a free start.  w.st, w.d0 and w.d1 are unused.  The hit search calls it; traceback_linear_kernel states the same
// loop in its own body (see there), so a change to a rule here is made there too.
template <bool D1, typename Cell, typename Leave>
__device__ __forceinline__ int walk_linear(const DeviceBatch& A, const PairDesc& pd, const TraceInputs& in, const int32_t* mu1tab,
                                           int SR, int c, bool fit, bool ovl, bool local, Cell&& cell, Leave&& leave,
                                           uint8_t* out, int cap, WalkPoint& w) {
  constexpr int BIG = 0x7fffffff;
  const int gamma = A.gamma, delta = A.delta;
  // offsets of the thirteen cases as bit masks o0*8+o1*4+o2*2+o3 (pyx:233-248), per lane
  constexpr int OFF[16] = {15, 10, 5, 12, 3, 8, 4, 2, 1, 11, 7, 14, 13, 0, 0, 0};
  int code_c = 0;
#pragma unroll
  for (int t = 0; t < 13; ++t)
    if (c == t) code_c = OFF[t];
  const int o0 = (code_c >> 3) & 1, o1 = (code_c >> 2) & 1, o2 = (code_c >> 1) & 1, o3 = code_c & 1;
  // score of case c as a*mu1 + b*mu2 + const (pyx:233-248)
  const int use1 = (c == 0 || c == 3 || c == 11 || c == 12), use2 = (c == 0 || c == 4 || c == 9 || c == 10);
  const int gD = gamma + delta;
  const int kconst = c == 0 ? 0 : (c <= 2 ? 2 * gamma : (c <= 4 ? delta : gD));

  int i = w.i, j = w.j, k = w.k, l = w.l, cur = w.cur, len = w.len;
  int how = WALK_COMPLETE;
  while (true) {
    if (fit && i == 0 && k == 0 && j == l && cur == 0) break;  // fit: a free start, start_b = j
    if (ovl && j == 0 && l == 0 && i == k && cur == 0) break;  // overlap: and on column 0, start_a = i
    if (local && i == k && j == l && cur == 0) break;          // local: a free start, (start_a, start_b) = (i, j)
    if (leave(i, j, k, l)) { how = WALK_LEFT; break; }
    const PointScores mu = point_scores<D1>(A, pd, in, mu1tab, i, j, k, l);
    const int sc = kconst + (use1 ? mu.mu1 : 0) + (use2 ? mu.mu2 : 0);
    const int pi = i - o0, pj = j - o1, pk = k - o2, pl = l - o3;
    const bool ok = c < 13 && pi >= 0 && pj >= 0 && pk >= 0 && pl >= 0 && abs(pk - pi) <= SR && abs(pl - pj) <= SR;
    const int ld = ok ? cell(pi, pj, pk - pi + SR, pl - pj + SR) : 0;
    const int key = (ok && ld + sc == cur) ? c : BIG;
    const int pick = __builtin_amdgcn_readfirstlane(wave_min16(key));
    if (pick == BIG) break;
    const int code = __builtin_amdgcn_readlane(code_c, pick);
    cur = __builtin_amdgcn_readlane(ld, pick);
    if (c == 0 && len < cap) out[len] = (uint8_t)code;
    ++len;
    i -= (code >> 3) & 1; j -= (code >> 2) & 1; k -= (code >> 1) & 1; l -= code & 1;
  }
  w = WalkPoint{i, j, k, l, 0, cur, 0, 0, len};
  return how;
}

//   STRIP (lean traceback): the walk continues from the pair's
//   TraceState through ONE strip -- the one fill_affine_kernel<.., RESW> has just re-swept into
//   the scratch records -- and stops when it steps into the strip above (whose bottom row, the
//   only row of it a candidate can touch from here, is in the LEAN records) or ends.
//   WIDE (max_shift beyond the tiled kernels, bialign_wide.hpp): the band half-width is the runtime
//   value A.wide_s and the layers lie in the reference's own order; S is then a dummy (0).
//   PACK: the sweep stored packed records in interior steps (Pack<S>).
//   D1: mu1 from the pair's dense table (DeviceBatch::dense_forms bit 1), mu2 dense if bit 0 is set.
//   LEVEL (level-checkpointed traceback of the wide-band path, bialign_wide.hpp): the walk continues from the
//   pair's TraceState through ONE segment of levels -- the one fill_wide_*_kernel<.., WIDE_SEG> has just swept
//   into the pair's scratch, addressed by level -- while every candidate of its point (1..4 levels down) lies
//   there; the band half-width is A.wide_s and S a dummy (0), as for WIDE.
template <int S, bool DO_TRACE, bool STRIP = false, bool WIDE = false, bool PACK = false, bool D1 = false, bool LEVEL = false>
__global__ void __launch_bounds__(64) traceback_affine_kernel(const DeviceBatch A, int npairs) {
  static_assert(!WIDE || !STRIP, "no lean traceback on the wide-band path");
  static_assert(!PACK || (!WIDE && !STRIP), "packed records: full-storage tiled sweeps");
  static_assert(!LEVEL || (DO_TRACE && !WIDE && !STRIP && !PACK), "level traceback: a form of its own");
  const int SR = (WIDE || LEVEL) ? A.wide_s : S;  // band half-width
  const int pid = A.order[blockIdx.x];
  const PairDesc pd = A.pairs[pid];
  const int n = pd.n, m = pd.m;
  const int32_t* lay = A.layers;
  const int c = threadIdx.x;  // candidate lane
  constexpr int W = 2 * S + 1, RR = Geo<S>::RR;
  extern __shared__ __align__(16) int32_t smem[];

  TraceState ts{};
  if (STRIP || LEVEL) {
    ts = A.tstate[pid];
    if (ts.done) return;
  }
  const int Q = STRIP ? (ts.started ? ts.strip : pd.NS - 1) : 0;
  const int Qlo = STRIP ? max(Q - A.resw_k + 1, 0) : 0;  // strips Qlo..Q sit in the scratch slots Q-sp
  const int64_t sstride = (int64_t)(m + Geo<S>::MAXOFF + 1) * Rec<S, 9>::RECDW;
  // LEVEL: the segment in the scratch and its lowest level
  const int seg = LEVEL ? wide_segment_of(ts, n, m, A.resw_k) : 0, seg_base = LEVEL ? wide_seg_base(seg, A.resw_k) : 0;
  // layer value (state ss) of lattice point (pi, pj, a, b)
  auto cell = [&](int pi, int pj, int a, int b, int ss) -> int {
    if (LEVEL) {  // [level - base][i][a][b/2][12]
      const int WR = 2 * SR + 1, lev = 2 * (pi + pj) + a + b - 2 * SR;
      return A.scratch[pd.scratch_off + ((lev - seg_base) * wide_level_points(n, SR) + (int64_t)(pi * WR + a) * ((WR + 1) / 2) + (b >> 1)) * 12 + ss];
    }
    if (WIDE) return lay[pd.layer_off + wide_dword(m, 2 * SR + 1, 9, pi, pj, a, b, ss)];
    if (PACK) return packed_cell<S>(lay, pd, pi, pj, a, b, ss);
    if (!STRIP) return lay[cell_dword<S, 9>(pd, pi, pj, a, b, ss)];
    const int sp = pi / RR, ilp = pi - sp * RR + 1;
    if (sp >= Qlo)  // inside a re-swept strip: record = step within the strip
      return A.scratch[pd.scratch_off + (Q - sp) * sstride +
                       Rec<S, 9>::dword(pj + 2 * ilp + a, (ilp - 1) * W + a, b * 9 + ss)];
    // bottom row of the strip above (ilp == RR): LEAN record of its global step
    return lay[pd.layer_off + Rec<S, 9, true>::dword((int64_t)sp * pd.P + pj + 2 * ilp + a, a, b * 9 + ss)];
  };

  constexpr bool FIT_FORM = !STRIP && !WIDE && !LEVEL;  // fit alignments: the tiled full-storage forms
  const bool fit = FIT_FORM && A.free_ends;
  const bool ovl = fit && (A.free_ends & FREE_A_ENDS);  // overlap alignments: A's end gaps are free as well
  const bool local = FIT_FORM && A.local;  // local alignments: the same forms
  WalkPoint w{n, m, n, m, 0, 0, 0, 0, 0};
  if (!(STRIP || LEVEL) || !ts.started) {
    free_end_start(A, pid, n, m, fit, ovl, local, c, [&](int pi, int pj) {
      int e = cell(pi, pj, SR, SR, 0);
      for (int q = 1; q < 9; ++q) e = max(e, cell(pi, pj, SR, SR, q));
      return e;
    }, &w.i, &w.j);
    w.k = w.i, w.l = w.j;
    affine_end_state(cell, w.i, w.j, SR, c, &w.cur, &w.st);
    if (c == 0) A.scores[pid] = w.cur;
    if (!DO_TRACE) return;
  } else {
    w = WalkPoint{ts.i, ts.j, ts.k, ts.l, ts.st, ts.cur, ts.d0, ts.d1, ts.len};
  }
  const TraceInputs in = stage_trace_inputs<D1>(A, pd, smem);
  const int32_t* const mu1tab = D1 ? mu1_table(A, pd) : nullptr;

  uint8_t* out = A.trace + pd.trace_off;
  const int how = walk_affine<D1>(A, pd, in, mu1tab, SR, c, fit, ovl, local, cell, [&](int i, int j, int k, int l) {
    return (STRIP && i < Qlo * RR) ||  // above the re-swept strips: next round
           (LEVEL && seg > 0 && i + j + k + l < seg_base + WIDE_SEG_OVERLAP);  // a candidate may lie below the scratch
  }, out, pd.trace_cap, w);
  if (how == WALK_LEFT) {  // hand over to the next round
    if (c == 0) {
      TraceState nx;
      nx.i = w.i; nx.j = w.j; nx.k = w.k; nx.l = w.l; nx.st = w.st; nx.cur = w.cur; nx.d0 = w.d0; nx.d1 = w.d1;
      nx.len = w.len; nx.strip = LEVEL ? seg - 1 : Qlo - 1; nx.started = 1; nx.done = 0;
      A.tstate[pid] = nx;
    }
    return;
  }
  const int len = min(w.len, pd.trace_cap);
  reverse_trace(out, len, c);
  if (c == 0) {
    A.trace_len[pid] = len;
    A.complete[pid] = how == WALK_COMPLETE;
    if (how == WALK_COMPLETE) publish_free_starts(A, pid, fit, ovl, local, w.i, w.j);
    if (STRIP || LEVEL) {
      ts.done = 1;
      ts.started = 1;
      A.tstate[pid] = ts;
    }
  }
}

// Non-affine traceback (pyx:513-531): the first case, in generator order, that is
// guard-valid and reproduces the cell; stops when none does (the origin).  One wave
// per pair, lane c < 13 = case c; "first" = wave-min over the matching lane ids.
template <int S, bool DO_TRACE, bool STRIP = false, bool WIDE = false, bool D1 = false, bool LEVEL = false>  // STRIP, WIDE, D1, LEVEL: see traceback_affine_kernel
__global__ void __launch_bounds__(64) traceback_linear_kernel(const DeviceBatch A, int npairs) {
  static_assert(!WIDE || !STRIP, "no lean traceback on the wide-band path");
  static_assert(!LEVEL || (DO_TRACE && !WIDE && !STRIP), "level traceback: a form of its own");
  constexpr bool CONT = STRIP || LEVEL;  // the walk goes on from the pair's TraceState
  const int SR = (WIDE || LEVEL) ? A.wide_s : S;
  const int pid = A.order[blockIdx.x];
  const PairDesc pd = A.pairs[pid];
  const int n = pd.n, m = pd.m;
  const int32_t* lay = A.layers;
  const int c = threadIdx.x;
  constexpr int W = 2 * S + 1, RR = Geo<S>::RR;
  extern __shared__ __align__(16) int32_t smem[];
  TraceState ts{};
  if (CONT) {
    ts = A.tstate[pid];
    if (ts.done) return;
  }
  const int Q = STRIP ? (ts.started ? ts.strip : pd.NS - 1) : 0;
  const int Qlo = STRIP ? max(Q - A.resw_k + 1, 0) : 0;
  const int64_t sstride = (int64_t)(m + Geo<S>::MAXOFF + 1) * Rec<S, 1>::RECDW;
  const int seg = LEVEL ? wide_segment_of(ts, n, m, A.resw_k) : 0, seg_base = LEVEL ? wide_seg_base(seg, A.resw_k) : 0;
  auto cell = [&](int pi, int pj, int a, int b) -> int {
    if (LEVEL) {  // [level - base][i][a][b/2]
      const int WR = 2 * SR + 1, lev = 2 * (pi + pj) + a + b - 2 * SR;
      return A.scratch[pd.scratch_off + (lev - seg_base) * wide_level_points(n, SR) + (int64_t)(pi * WR + a) * ((WR + 1) / 2) + (b >> 1)];
    }
    if (WIDE) return lay[pd.layer_off + wide_dword(m, 2 * SR + 1, 1, pi, pj, a, b, 0)];
    if (!STRIP) return lay[cell_dword<S, 1>(pd, pi, pj, a, b, 0)];
    const int sp = pi / RR, ilp = pi - sp * RR + 1;
    if (sp >= Qlo)
      return A.scratch[pd.scratch_off + (Q - sp) * sstride + Rec<S, 1>::dword(pj + 2 * ilp + a, (ilp - 1) * W + a, b)];
    return lay[pd.layer_off + Rec<S, 1, true>::dword((int64_t)sp * pd.P + pj + 2 * ilp + a, a, b)];
  };
  constexpr bool FIT_FORM = !STRIP && !WIDE && !LEVEL;  // fit alignments: the tiled full-storage forms
  const bool fit = FIT_FORM && A.free_ends;
  const bool ovl = fit && (A.free_ends & FREE_A_ENDS);  // overlap alignments: A's end gaps are free as well
  const bool local = FIT_FORM && A.local;  // local alignments: the same forms
  WalkPoint w{n, m, n, m, 0, 0, 0, 0, 0};
  if (CONT && ts.started) {
    w.i = ts.i; w.j = ts.j; w.k = ts.k; w.l = ts.l; w.cur = ts.cur; w.len = ts.len;
  } else {
    free_end_start(A, pid, n, m, fit, ovl, local, c, [&](int pi, int pj) { return cell(pi, pj, SR, SR); }, &w.i, &w.j);
    w.k = w.i, w.l = w.j;
    w.cur = cell(w.i, w.j, SR, SR);
    if (c == 0) A.scores[pid] = w.cur;  // pyx:471
  }
  if (!DO_TRACE) return;
  const TraceInputs in = stage_trace_inputs<D1>(A, pd, smem);
  const int32_t* const mu1tab = D1 ? mu1_table(A, pd) : nullptr;

  uint8_t* out = A.trace + pd.trace_off;
  // The column loop is walk_linear's, stated here a second time: with the call in its place the 1024 x 1024 one-layer
  // batch walked 2 % slower than the parent's kernel on the device, with this text it does not.
  // A change to a rule of the one-layer walk is made in both.
  constexpr int BIG = 0x7fffffff;
  const int gamma = A.gamma, delta = A.delta;
  // offsets of the thirteen cases as bit masks o0*8+o1*4+o2*2+o3 (pyx:233-248), per lane
  constexpr int OFF[16] = {15, 10, 5, 12, 3, 8, 4, 2, 1, 11, 7, 14, 13, 0, 0, 0};
  int code_c = 0;
#pragma unroll
  for (int t = 0; t < 13; ++t)
    if (c == t) code_c = OFF[t];
  const int o0 = (code_c >> 3) & 1, o1 = (code_c >> 2) & 1, o2 = (code_c >> 1) & 1, o3 = code_c & 1;
  // score of case c as a*mu1 + b*mu2 + const (pyx:233-248)
  const int use1 = (c == 0 || c == 3 || c == 11 || c == 12), use2 = (c == 0 || c == 4 || c == 9 || c == 10);
  const int gD = gamma + delta;
  const int kconst = c == 0 ? 0 : (c <= 2 ? 2 * gamma : (c <= 4 ? delta : gD));
  int i = w.i, j = w.j, k = w.k, l = w.l, cur = w.cur, len = w.len;
  bool finished = true;
  while (true) {
    if (fit && i == 0 && k == 0 && j == l && cur == 0) break;  // fit: a free start, start_b = j
    if (ovl && j == 0 && l == 0 && i == k && cur == 0) break;  // overlap: and on column 0, start_a = i
    if (local && i == k && j == l && cur == 0) break;          // local: a free start, (start_a, start_b) = (i, j)
    if (STRIP && i < Qlo * RR) { finished = false; break; }  // above the re-swept strips: next round
    if (LEVEL && seg > 0 && i + j + k + l < seg_base + WIDE_SEG_OVERLAP) { finished = false; break; }
    const PointScores mu = point_scores<D1>(A, pd, in, mu1tab, i, j, k, l);
    const int sc = kconst + (use1 ? mu.mu1 : 0) + (use2 ? mu.mu2 : 0);
    const int pi = i - o0, pj = j - o1, pk = k - o2, pl = l - o3;
    const bool ok = c < 13 && pi >= 0 && pj >= 0 && pk >= 0 && pl >= 0 && abs(pk - pi) <= SR && abs(pl - pj) <= SR;
    const int ld = ok ? cell(pi, pj, pk - pi + SR, pl - pj + SR) : 0;
    const int key = (ok && ld + sc == cur) ? c : BIG;
    const int pick = __builtin_amdgcn_readfirstlane(wave_min16(key));
    if (pick == BIG) break;
    const int code = __builtin_amdgcn_readlane(code_c, pick);
    cur = __builtin_amdgcn_readlane(ld, pick);
    if (c == 0 && len < pd.trace_cap) out[len] = (uint8_t)code;
    ++len;
    i -= (code >> 3) & 1; j -= (code >> 2) & 1; k -= (code >> 1) & 1; l -= code & 1;
  }
  if (CONT && !finished) {  // hand over to the next round
    if (c == 0) {
      TraceState nx{};
      nx.i = i; nx.j = j; nx.k = k; nx.l = l; nx.cur = cur; nx.len = len;
      nx.strip = LEVEL ? seg - 1 : Qlo - 1; nx.started = 1; nx.done = 0;
      A.tstate[pid] = nx;
    }
    return;
  }
  if (len > pd.trace_cap) len = pd.trace_cap;
  reverse_trace(out, len, c);
  if (c == 0) {
    A.trace_len[pid] = len;
    A.complete[pid] = 1;
    publish_free_starts(A, pid, fit, ovl, local, i, j);
    if (CONT) {
      ts.done = 1;
      ts.started = 1;
      A.tstate[pid] = ts;
    }
  }
}

}  // namespace bialign
