// bialign_null.hpp -- shuffled-null significance: the replicas' B codes and the per-pair reduction of their scores.
//
// A null batch (bialign_batch_create_null) is a SCORE_ONLY batch of npairs * R *virtual* pairs, virtual pair
// v = p * R + r being real pair p against replica r of its B molecule.  The sweeps run on it exactly as on any batch:
// a virtual pair's PairDesc::seq_a is the real pair's, its seq_b points into the replica buffers, which
// shuffle_codes_kernel fills from the one uploaded copy of B.  null_stats_kernel then reduces every real pair's R
// scores to exact integers; no floating point on the device.  A FEATURE-form null batch
// (bialign_batch_create_null_features) has replica planes of doubles beside the replica codes, which
// shuffle_features_kernel fills (below); build_mu2_kernel reads them through the same seq_b.  A DENSE-form null batch
// (bialign_batch_create_null_dense) keeps every replica's finished permutation in an index array beside the replica
// codes (shuffle_index_kernel), through which permute_tables_kernel gathers the columns of the real pairs' tables into
// each chunk's table scratch (below).
//
// The permutation is the one include/bialign.h states (normative there; bialign_amd/significance.py mirrors it): THE
// PERMUTATION (BIALIGN_NULL_MONO, null_perm_to_lds and shuffle_codes_kernel) or, where bialign_batch_set_null_model asked
// for it, THE DINUCLEOTIDE PERMUTATION (null_dinuc_perm_to_lds, through the two wave-per-pair kernels in every form).
//
// Mapping of shuffle_codes_kernel: one thread per virtual pair.  It copies B into its own slice of the replica buffers and
// runs the Fisher-Yates swaps there in place (swapping the values is the same as gathering through the permuted
// index array: seq'[x] = seq_b[perm[x]]).  The chain of swaps is sequential per replica by definition, the replicas
// are independent: npairs * R threads, each O(m) dependent byte accesses that stay in L2 -- against O(m^2) lattice
// cells per replica in the sweep.  Vector loads and stores, 64-bit offsets, no atomics, no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bialign.h"
#include "bialign_types.hpp"

namespace bialign {

__host__ __device__ inline uint32_t null_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ inline uint32_t null_hash(uint32_t seed, uint32_t p, uint32_t r) {
  return null_mix(null_mix(null_mix(seed ^ 0x9E3779B9u) + p) + r);
}
// in [0, t]
__host__ __device__ inline uint32_t null_draw(uint32_t h, uint32_t t) {
  return (uint32_t)(((uint64_t)null_mix(h + t) * (uint64_t)(t + 1)) >> 32);
}

struct ShuffleArgs {
  const PairDesc* pairs;    // the VIRTUAL pairs: m, and seq_b = start of the replica's slice in dst_seq / dst_cls
  const int64_t* src_off;   // [real pairs] start of pair p's B in src_seq / src_cls
  const uint8_t *src_seq, *src_cls;  // the uploaded B codes
  uint8_t *dst_seq, *dst_cls;        // the replica buffers
  int32_t first, count;     // virtual pairs first .. first + count
  int32_t replicas;
  uint32_t seed;
};

constexpr int NULL_BLOCK = 256;

// (not moved onto the wave kernels below: their uint16 index array would refuse len_b > 65535, which this form takes)
__global__ __launch_bounds__(NULL_BLOCK) void shuffle_codes_kernel(ShuffleArgs A) {
  const int64_t t0 = (int64_t)blockIdx.x * NULL_BLOCK + threadIdx.x;
  if (t0 >= A.count) return;
  const int32_t v = A.first + (int32_t)t0;
  const int32_t p = v / A.replicas, r = v - p * A.replicas;
  const PairDesc& pd = A.pairs[v];
  const int32_t m = pd.m;
  const uint8_t* const ss = A.src_seq + A.src_off[p];
  const uint8_t* const sc = A.src_cls + A.src_off[p];
  uint8_t* const ds = A.dst_seq + pd.seq_b;
  uint8_t* const dc = A.dst_cls + pd.seq_b;
  for (int32_t x = 0; x < m; ++x) {
    ds[x] = ss[x];
    dc[x] = sc[x];
  }
  const uint32_t h = null_hash(A.seed, (uint32_t)p, (uint32_t)r);
  for (int32_t t = m - 1; t >= 1; --t) {
    const uint32_t j = null_draw(h, (uint32_t)t);  // <= t < m: inside the slice
    const uint8_t st = ds[t], ct = dc[t], sj = ds[j], cj = dc[j];
    ds[j] = st;
    dc[j] = ct;
    ds[t] = sj;
    dc[t] = cj;
  }
}

struct NullStatsArgs {
  const int32_t* scores;    // [npairs * replicas], pair-major
  const int32_t* observed;  // [npairs] or nullptr
  bialign_null_stats* out;  // [npairs]
  int32_t npairs, replicas;
};

// One wave per real pair: lanes stride over its R scores, then a butterfly over the wave.  |score| < 2^28 and
// R * bound^2 < 2^63 are the host's checks (bialign_batch_create_null), so neither sum can overflow.
__global__ __launch_bounds__(NULL_BLOCK) void null_stats_kernel(NullStatsArgs A) {
  const int lane = threadIdx.x & 63;
  const int32_t p = (int32_t)blockIdx.x * (NULL_BLOCK / 64) + (int32_t)(threadIdx.x >> 6);
  if (p >= A.npairs) return;  // (whole waves leave: p is wave-uniform)
  const int32_t R = A.replicas;
  const int32_t* const sc = A.scores + (int64_t)p * R;
  const bool have_obs = A.observed != nullptr;
  const int32_t obs = have_obs ? A.observed[p] : 0;
  int64_t sum = 0, sumsq = 0;
  int32_t mn = INT32_MAX, mx = INT32_MIN, nge = 0;
  for (int32_t r = lane; r < R; r += 64) {
    const int32_t x = sc[r];
    sum += x;
    sumsq += (int64_t)x * x;
    mn = x < mn ? x : mn;
    mx = x > mx ? x : mx;
    nge += (have_obs && x >= obs) ? 1 : 0;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    sum += __shfl_xor(sum, d, 64);
    sumsq += __shfl_xor(sumsq, d, 64);
    const int32_t omn = __shfl_xor(mn, d, 64), omx = __shfl_xor(mx, d, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    nge += __shfl_xor(nge, d, 64);
  }
  if (lane == 0) {
    bialign_null_stats s;
    s.sum = sum;
    s.sumsq = sumsq;
    s.min = mn;
    s.max = mx;
    s.n_ge = nge;
    s.replicas = R;
    A.out[p] = s;
  }
}

// ---- FEATURE-form null batches (bialign_batch_create_null_features): the replicas' sequence codes and their three
// planes of doubles (up, down, unp), a residue's letter and its three numbers moving together.
//
// Mapping: one wave per virtual pair, not shuffle_codes_kernel's thread per replica -- that one swaps in place in
// global memory, which with three doubles per residue would be four dependent 8-byte read-modify-writes per swap.
// Here the swaps run on an index array in LDS and the data moves once:
//   1. perm = identity, uint16 (m < 65536 is the host's check), 2 * m bytes of dynamic LDS;
//   2. draw(t) depends on (h, t) only, not on the array: per block of 64 values of t every lane computes one draw into
//      a register, and the chain of swaps -- sequential by definition -- takes them from there by readlane.  The loop
//      is wave-uniform; the two LDS reads of a step are broadcasts, lane 0 alone stores (so lane 0 only ever reads
//      what it wrote itself: no barrier inside the chain);
//   3. all lanes gather seq, up, down, unp through perm: random reads inside the one B molecule (24 * m bytes, cache
//      resident), coalesced stores of 512 bytes per plane and wave.  The doubles are moved, never recomputed.
// (Draws kept in LDS as well would double the array to 4 * m bytes, beyond a workgroup's 160 KiB for the longest
// molecules the engine takes; registers + readlane need none.)
// Vector loads and stores, 64-bit offsets, no atomics.  m = 1: the chain is empty, the identity.
// What the wave-per-pair kernels' arguments share with ShuffleArgs, field for field (the launchers fill them in one place,
// bialign_null.hip), and behind them the null model, which only these kernels have.  ShuffleArgs itself keeps its layout:
// extending it would move shuffle_codes_kernel's argument loads.
struct ShuffleBase {
  const PairDesc* pairs;    // the VIRTUAL pairs: m, and seq_b = start of the replica's slice in the dst_* buffers
  const int64_t* src_off;   // [real pairs] start of pair p's B in the src_* buffers
  int32_t first, count;     // virtual pairs first .. first + count
  int32_t replicas;
  uint32_t seed;
  int32_t model;            // BIALIGN_NULL_MONO: null_perm_to_lds; BIALIGN_NULL_DINUCLEOTIDE: null_dinuc_perm_to_lds
  int32_t tree_cap;         // ... and its CAP, 0..NULL_TREE_CAP
};

struct ShuffleFeatArgs : ShuffleBase {
  const uint8_t* src_seq;   // the uploaded B codes
  const double *src_up, *src_down, *src_unp;  // ... and features
  uint8_t* dst_seq;         // the replica buffers
  double *dst_up, *dst_down, *dst_unp;
};

// (the index array is uint16: m <= NULL_FEAT_MAX_M = 65535, bialign_host.hpp, checked where the batch is created)
constexpr int NULL_FEAT_MAX_GRID = 1 << 20;  // workgroups of a launch; more virtual pairs loop

// The permutation of replica hash h over 0..m-1, left in perm[0..m) for every lane of the one wave that calls it (steps
// 1 and 2 above; m is wave-uniform).  The only statement of the chain on the device: both wave-per-pair kernels call it.
__device__ __forceinline__ void null_perm_to_lds(uint32_t h, int32_t m, int32_t lane, uint16_t* perm) {
  for (int32_t x = lane; x < m; x += 64) perm[x] = (uint16_t)x;
  __syncthreads();
  for (int32_t tb = (m - 1) & ~63; tb >= 0; tb -= 64) {
    const uint32_t d = null_draw(h, (uint32_t)(tb + lane));  // lane k holds draw(tb + k) <= tb + k
    const int32_t khi = m - 1 - tb < 63 ? m - 1 - tb : 63, klo = tb == 0 ? 1 : 0;
    for (int32_t k = khi; k >= klo; --k) {
      const int32_t t = tb + k;                                    // m - 1 down to 1
      const int32_t j = __builtin_amdgcn_readlane((int32_t)d, k);  // <= t < m: inside the array
      const uint16_t pt = perm[t], pj = perm[j];
      if (lane == 0) {
        perm[t] = pj;
        perm[j] = pt;
      }
    }
  }
  __syncthreads();
}

// ---- THE DINUCLEOTIDE PERMUTATION (include/bialign.h, whose step numbers the comments below use): the sibling of
// null_perm_to_lds, one wave per virtual pair, perm left in the same LDS array.  The letters are B's sequence codes.
//
// LDS of a molecule of m residues, mp = m rounded up to even, behind one another:
//   perm uint16[mp] | L uint16[mp] | first uint32[256] | off, cnt, last, nxt uint16[256] each | map, intree uint8[256] each
//   | B uint8[m]
// = 4 * mp + NULL_DINUC_FIXED + m bytes (null_dinuc_lds): within a workgroup's 160 KiB up to m = NULL_DINUC_MAX_M.
//
// Where each step runs:
//   letters  all lanes stage the codes into B; an LDS atomicMin per residue leaves every code's first position; a ballot
//            and prefix popcount over blocks of 64 positions numbers the first occurrences in order (map), B is renamed
//            in place.  K letters.
//   1        per letter a ballot over blocks of 64 edges and a prefix popcount: a stable fill of L, and cnt / off fall out
//            of the running write position.  K * ceil((m - 1) / 64) wave steps.
//   2        a wave-uniform serial chain of LDS reads: every value read goes through readfirstlane (lane 0's view, which
//            wrote it), lane 0 stores.  At most tree_cap draws, the marking walks at most K steps each.
//   3        per letter the element at last[x] moves to the list's end, 64 elements shifting at a time, then the swaps of
//            the chain take their draws 64 at a time from registers by readlane, as null_perm_to_lds does.
//   4        the walk, serial like 2: three dependent LDS reads per position (nxt = off + ptr, L, B).
// Every loop is bounded by m, K <= 256 or tree_cap.  No global memory but the m code loads; no global atomics.
constexpr int NULL_LETTERS = 256;    // a sequence code is a uint8
constexpr int NULL_TREE_CAP = 4096;  // CAP
constexpr int NULL_DINUC_FIXED = NULL_LETTERS * (4 + 4 * 2 + 2 * 1);
constexpr int NULL_LDS_MAX = 160 * 1024;
__host__ __device__ constexpr int64_t null_dinuc_lds(int64_t m) { return 4 * ((m + 1) & ~int64_t(1)) + NULL_DINUC_FIXED + m; }
constexpr int NULL_DINUC_MAX_M = BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN;
static_assert(null_dinuc_lds(NULL_DINUC_MAX_M) <= NULL_LDS_MAX && null_dinuc_lds(NULL_DINUC_MAX_M + 1) > NULL_LDS_MAX,
              "NULL_DINUC_MAX_M is the longest molecule the layout admits");
static_assert(NULL_DINUC_MAX_M >= 30000 && NULL_DINUC_MAX_M <= 65535, "include/bialign.h promises 30000; L and perm are uint16");

// in [0, bound)
__host__ __device__ inline uint32_t null_uni(uint32_t h, uint32_t salt, uint32_t bound) {
  return (uint32_t)(((uint64_t)null_mix(h + salt) * (uint64_t)bound) >> 32);
}

// a[i] as lane 0 sees it, in every lane (wave-uniform control flow only)
template <class T>
__device__ __forceinline__ int32_t null_wave_ld(const T* a, int32_t i) {
  return __builtin_amdgcn_readfirstlane((int32_t)a[i]);
}

__device__ __forceinline__ void null_dinuc_perm_to_lds(uint32_t h, int32_t m, int32_t lane, const uint8_t* __restrict__ codes,
                                                       int32_t tree_cap, uint16_t* perm) {
  if (m <= 2) {  // (wave-uniform, as everything that steers a branch or a loop below)
    for (int32_t x = lane; x < m; x += 64) perm[x] = (uint16_t)x;
    __syncthreads();
    return;
  }
  const int32_t mp = (m + 1) & ~1;
  uint16_t* const L = perm + mp;
  uint32_t* const first = reinterpret_cast<uint32_t*>(L + mp);
  uint16_t* const off = reinterpret_cast<uint16_t*>(first + NULL_LETTERS);
  uint16_t* const cnt = off + NULL_LETTERS;
  uint16_t* const last = cnt + NULL_LETTERS;
  uint16_t* const nxt = last + NULL_LETTERS;
  uint8_t* const map = reinterpret_cast<uint8_t*>(nxt + NULL_LETTERS);
  uint8_t* const intree = map + NULL_LETTERS;
  uint8_t* const B = intree + NULL_LETTERS;
  const uint64_t below = ((uint64_t)1 << lane) - 1;  // the lanes ahead of this one

  // letters: renumbered 0, 1, 2, ... in order of first occurrence
  for (int32_t c = lane; c < NULL_LETTERS; c += 64) {
    first[c] = 0xFFFFFFFFu;
    intree[c] = 0;
  }
  for (int32_t x = lane; x < m; x += 64) B[x] = codes[x];
  __syncthreads();
  for (int32_t x = lane; x < m; x += 64) atomicMin(&first[B[x]], (uint32_t)x);
  __syncthreads();
  int32_t K = 0;
  for (int32_t xb = 0; xb < m; xb += 64) {
    const int32_t x = xb + lane;
    const bool opens = x < m && first[B[x]] == (uint32_t)x;
    const uint64_t mask = __ballot(opens);
    if (opens) map[B[x]] = (uint8_t)(K + __popcll(mask & below));
    K += __popcll(mask);
  }
  __syncthreads();
  for (int32_t x = lane; x < m; x += 64) B[x] = map[B[x]];
  __syncthreads();

  // 1. edges: L sorted by (tail, e); cnt, off; nxt = off + ptr of step 4
  int32_t w = 0;
  for (int32_t x = 0; x < K; ++x) {
    const int32_t o = w;
    for (int32_t eb = 0; eb < m - 1; eb += 64) {
      const int32_t e = eb + lane;
      const bool mine = e < m - 1 && B[e] == x;
      const uint64_t mask = __ballot(mine);
      if (mine) L[w + __popcll(mask & below)] = (uint16_t)e;  // w + ... < m - 1: every edge has one tail
      w += __popcll(mask);
    }
    if (lane == 0) {
      off[x] = (uint16_t)o;
      cnt[x] = (uint16_t)(w - o);
      nxt[x] = (uint16_t)o;
    }
  }
  __syncthreads();
  const int32_t z = null_wave_ld(B, m - 1);

  // 2. last exits
  if (lane == 0) intree[z] = 1;
  int32_t s = 0;
  bool gave_up = false;
  for (int32_t x = 0; x < K && !gave_up; ++x) {
    if (null_wave_ld(cnt, x) == 0 || null_wave_ld(intree, x)) continue;
    int32_t u = x;
    while (!null_wave_ld(intree, u)) {  // (u != z has an exit: cnt[u] >= 1)
      if (s >= tree_cap) {
        gave_up = true;
        break;
      }
      const int32_t l = (int32_t)null_uni(h, 0x80000000u + (uint32_t)s, (uint32_t)null_wave_ld(cnt, u));
      if (lane == 0) last[u] = (uint16_t)l;
      ++s;
      u = null_wave_ld(B, null_wave_ld(L, null_wave_ld(off, u) + l) + 1);
    }
    if (gave_up) break;
    u = x;
    for (int32_t g = 0; g < K && !null_wave_ld(intree, u); ++g) {  // (a path along last[] into the tree: no letter twice)
      if (lane == 0) intree[u] = 1;
      u = null_wave_ld(B, null_wave_ld(L, null_wave_ld(off, u) + null_wave_ld(last, u)) + 1);
    }
  }
  if (gave_up)  // the molecule's own last exits
    for (int32_t x = lane; x < K; x += 64)
      if (x != z && cnt[x] > 0) last[x] = (uint16_t)(cnt[x] - 1);
  __syncthreads();

  // 3. order of exits
  for (int32_t x = 0; x < K; ++x) {
    const int32_t c = null_wave_ld(cnt, x);
    if (c == 0) continue;
    const int32_t o = null_wave_ld(off, x);
    uint16_t* const Lx = L + o;  // letter x's list
    int32_t r = c;
    if (x != z) {  // the last exit to the list's end, the others keep their order
      const int32_t l = null_wave_ld(last, x);
      const int32_t keep = null_wave_ld(Lx, l);
      for (int32_t ib = l; ib < c - 1; ib += 64) {
        const int32_t i = ib + lane;
        const uint16_t v = i < c - 1 ? Lx[i + 1] : 0;
        __syncthreads();
        if (i < c - 1) Lx[i] = v;
        __syncthreads();
      }
      if (lane == 0) Lx[c - 1] = (uint16_t)keep;
      r = c - 1;
    }
    for (int32_t tb = (r - 1) & ~63; tb >= 0; tb -= 64) {  // (r = 0: tb = -64, no step)
      const uint32_t d = null_uni(h, (uint32_t)(o + tb + lane), (uint32_t)(tb + lane + 1));  // lane k: the draw of t = tb + k
      const int32_t khi = r - 1 - tb < 63 ? r - 1 - tb : 63, klo = tb == 0 ? 1 : 0;
      for (int32_t k = khi; k >= klo; --k) {
        const int32_t t = tb + k;                                    // r - 1 down to 1
        const int32_t j = __builtin_amdgcn_readlane((int32_t)d, k);  // <= t < r: inside the letter's list
        const uint16_t pt = Lx[t], pj = Lx[j];
        if (lane == 0) {
          Lx[t] = pj;
          Lx[j] = pt;
        }
      }
    }
  }
  __syncthreads();

  // 4. walk
  if (lane == 0) perm[0] = 0;
  int32_t cur = null_wave_ld(B, 0);
  for (int32_t pos = 1; pos < m; ++pos) {
    const int32_t q = null_wave_ld(nxt, cur);
    const int32_t e = null_wave_ld(L, q);
    const int32_t to = e + 1 < m ? e + 1 : m - 1;  // (e <= m - 2 by construction; the consumers index global memory with it)
    if (lane == 0) {
      nxt[cur] = (uint16_t)(q + 1);
      perm[pos] = (uint16_t)to;
    }
    cur = null_wave_ld(B, to);
  }
  __syncthreads();
}

// The permutation of virtual pair (p, r) under the launch's model, left in perm for every lane of the wave
__device__ __forceinline__ void null_model_perm_to_lds(const ShuffleBase& A, int32_t p, int32_t r, int32_t m, int32_t lane,
                                                       const uint8_t* codes, uint16_t* perm) {
  const uint32_t h = null_hash(A.seed, (uint32_t)p, (uint32_t)r);
  if (A.model == BIALIGN_NULL_DINUCLEOTIDE) null_dinuc_perm_to_lds(h, m, lane, codes, A.tree_cap, perm);
  else null_perm_to_lds(h, m, lane, perm);
}

__global__ __launch_bounds__(64) void shuffle_features_kernel(ShuffleFeatArgs A) {
  extern __shared__ uint16_t null_perm[];  // [longest m of the launch]
  const int32_t lane = (int32_t)threadIdx.x;
  for (int64_t w = blockIdx.x; w < A.count; w += gridDim.x) {
    const int32_t v = A.first + (int32_t)w;
    const int32_t p = v / A.replicas, r = v - p * A.replicas;
    const PairDesc& pd = A.pairs[v];
    const int32_t m = __builtin_amdgcn_readfirstlane(pd.m);
    const int64_t src = A.src_off[p], dst = pd.seq_b;
    null_model_perm_to_lds(A, p, r, m, lane, A.src_seq + src, null_perm);
    // (source and replica buffers are distinct allocations: the four loads of a residue go out together)
    const uint8_t* __restrict__ const ss = A.src_seq + src;
    const double* __restrict__ const su = A.src_up + src;
    const double* __restrict__ const sd = A.src_down + src;
    const double* __restrict__ const sp = A.src_unp + src;
    uint8_t* __restrict__ const ds = A.dst_seq + dst;
    double* __restrict__ const du = A.dst_up + dst;
    double* __restrict__ const dd = A.dst_down + dst;
    double* __restrict__ const dp = A.dst_unp + dst;
    for (int32_t x = lane; x < m; x += 64) {
      const int32_t s = null_perm[x];  // < m
      ds[x] = ss[s];
      du[x] = su[s];
      dd[x] = sd[s];
      dp[x] = sp[s];
    }
    __syncthreads();  // (the next virtual pair of this workgroup overwrites the array)
  }
}

// ---- DENSE-form null batches (bialign_batch_create_null_dense): a residue of B carries a COLUMN of the pair's n x m
// table(s), so replica r's tables are the real pair's with their columns gathered through perm.  Two stages:
//
// shuffle_index_kernel, once per run ahead of the first sweep: the chain of shuffle_features_kernel, one wave per
// virtual pair, and the finished perm stored to an HBM index array (uint16, laid out like the replica codes: the virtual
// pair's at its seq_b), together with the gathered codes of whichever of mu1 / mu2 is in LOOKUP form (a nullptr source:
// that form is dense, the replicas' codes of that kind stay zero).
//
// permute_tables_kernel, once per chunk in the table builder's slot: a pure gather, no chain.  The real pair's tables
// lie end to end (mu2's, then mu1's: the order the consumers expect them in), and so do the replica's in the chunk's
// scratch -- forms * n rows of m values, all gathered through the same perm.  Grid (virtual pairs of the chunk in
// launch order, tile groups).  A workgroup of PERM_WAVES waves takes a tile of T rows: it loads them coalesced into LDS
// (T * m dwords, contiguous in the source), then lanes run along x -- one coalesced 2-byte load of perm[x] per column
// tile of 64 --, the waves take every PERM_WAVES-th row of the tile, read LDS at perm[x] and store 256-byte row
// segments: HBM sees each source byte once and each destination byte once.  T = permute_tile_rows(m): PERM_ROWS rows,
// fewer where they exceed the 64 KiB tile; a row that alone exceeds it (m > PERM_LDS_DW) is gathered straight from
// global memory.  Vector loads and stores, 64-bit offsets, no atomics.  perm[x] < m: the index kernel ran first.
struct ShuffleIndexArgs : ShuffleBase {
  const uint8_t *src_seq, *src_cls;  // the uploaded B codes; nullptr: mu1 (seq) / mu2 (cls) is dense
  uint8_t *dst_seq, *dst_cls;        // the replica buffers
  uint16_t* dst_perm;                // the replicas' permutations; nullptr: a LOOKUP-form null batch under the
                                     // dinucleotide model, which wants the gathered codes only
};

__global__ __launch_bounds__(64) void shuffle_index_kernel(ShuffleIndexArgs A) {
  extern __shared__ uint16_t null_perm[];  // [longest m of the launch]
  const int32_t lane = (int32_t)threadIdx.x;
  for (int64_t w = blockIdx.x; w < A.count; w += gridDim.x) {
    const int32_t v = A.first + (int32_t)w;
    const int32_t p = v / A.replicas, r = v - p * A.replicas;
    const PairDesc& pd = A.pairs[v];
    const int32_t m = __builtin_amdgcn_readfirstlane(pd.m);
    const int64_t src = A.src_off[p], dst = pd.seq_b;
    null_model_perm_to_lds(A, p, r, m, lane, A.src_seq + src, null_perm);  // (the dinucleotide model has src_seq: the host's check)
    for (int32_t x = lane; x < m; x += 64) {
      const int32_t s = null_perm[x];  // < m
      if (A.dst_perm) A.dst_perm[dst + x] = (uint16_t)s;
      if (A.src_seq) A.dst_seq[dst + x] = A.src_seq[src + s];
      if (A.src_cls) A.dst_cls[dst + x] = A.src_cls[src + s];
    }
    __syncthreads();  // (the next virtual pair of this workgroup overwrites the array)
  }
}

constexpr int PERM_WAVES = 4;           // waves per workgroup
constexpr int PERM_ROWS = 16;           // rows per tile at most
constexpr int PERM_LDS_DW = 16384;      // dwords of the LDS tile: 64 KiB
constexpr int PERM_MAX_GRID_Y = 4096;   // tile groups per pair in the grid; taller tables loop

// rows of an LDS tile for tables of m columns; 0: one row exceeds the tile, gather from global memory
__host__ __device__ inline int32_t permute_tile_rows(int32_t m) {
  return m > PERM_LDS_DW ? 0 : (PERM_LDS_DW / m < PERM_ROWS ? PERM_LDS_DW / m : PERM_ROWS);
}

struct PermuteArgs {
  const PairDesc* pairs;    // the VIRTUAL pairs: n, m, tab_off (chunk-relative), seq_b = start of the replica's perm
  const int32_t* order;     // launch order of the pairs to permute (block x -> virtual pair id)
  const uint16_t* perm;     // what shuffle_index_kernel wrote
  const int32_t* src;       // the real pairs' resident tables
  const int64_t* src_off;   // [real pairs] start of pair p's tables in src
  int32_t* tab;             // the chunk's table buffer
  int32_t replicas;
  int32_t forms;            // dense forms of the batch, 1 or 2: tables per pair
};

__global__ __launch_bounds__(64 * PERM_WAVES) void permute_tables_kernel(PermuteArgs A) {
  extern __shared__ int32_t perm_tile[];  // [T * m of the launch's widest LDS tile]
  const int32_t pid = A.order[blockIdx.x];
  const PairDesc& pd = A.pairs[pid];
  const int32_t m = pd.m;
  const int64_t rows = (int64_t)pd.n * A.forms;
  const int32_t lane = (int32_t)(threadIdx.x & 63);
  const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
  const int32_t* __restrict__ const src = A.src + A.src_off[pid / A.replicas];
  int32_t* __restrict__ const dst = A.tab + pd.tab_off;
  const uint16_t* __restrict__ const perm = A.perm + pd.seq_b;
  const int32_t T = permute_tile_rows(m);
  const int32_t TR = T ? T : PERM_ROWS;
  const int64_t ntiles = (rows + TR - 1) / TR;
  for (int64_t t = blockIdx.y; t < ntiles; t += gridDim.y) {  // (uniform over the workgroup: the barriers are met by all)
    const int64_t r0 = t * TR;
    const int32_t nr = rows - r0 < TR ? (int32_t)(rows - r0) : TR;
    const int32_t* const srow = src + r0 * m;
    int32_t* const drow = dst + r0 * m;
    if (T) {
      const int32_t cnt = nr * m;  // <= PERM_LDS_DW
      for (int32_t i = (int32_t)threadIdx.x; i < cnt; i += 64 * PERM_WAVES) perm_tile[i] = srow[i];
      __syncthreads();
    }
    for (int32_t x = lane; x < m; x += 64) {
      const int32_t s = perm[x];  // < m
      for (int32_t r = wave; r < nr; r += PERM_WAVES)
        drow[(int64_t)r * m + x] = T ? perm_tile[r * m + s] : srow[(int64_t)r * m + s];
    }
    if (T) __syncthreads();  // (the next tile overwrites the array)
  }
}

}  // namespace bialign
