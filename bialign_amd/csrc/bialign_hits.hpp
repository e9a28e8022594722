// bialign_hits.hpp -- the hit search of a full-storage FIT batch (include/bialign.h, bialign_batch_set_hits): every
// placement of A in B, found and walked while the chunk's layers are resident.  One wave per pair, behind the chunk's
// traceback; the kernel is instantiated in bialign_hits.hip, the C-ABI unit only calls launch_fit_hits().
#pragma once
#include "bialign_host.hpp"

namespace bialign {

// What the search needs beside the DeviceBatch (which keeps its size): the spec and the result buffers.
struct HitArgs {
  int32_t max_hits, max_walks, min_score;
  int32_t search;       // 0: the profile only (a BIALIGN_RUN_FILL_ONLY run)
  int32_t lds_inputs;   // bytes of the staged inputs in LDS (BatchPlan::lds_trace, rounded up to 16); the mask follows
  int32_t mask_words;   // dwords of the mask bitset: the batch's largest (m + 1 + 31) / 32; the accepted spans follow
  const int64_t* prof_off;  // [npairs] start of a pair's profile
  int32_t* profile;     // E(j), j = 0..m, pair after pair
  int32_t* head;        // [npairs][4] = (nhits, nwalks, status, T_p); T_p is written by the OPT kernels, else 0
  int32_t* hits;        // [npairs][max_hits][4] = (start_b, end_b, score, trace_len)
  int32_t* walks;       // [npairs][max_walks][4] = (end_b, start_b, score, accepted)
  uint8_t* trace;       // pair p's slot h: max_hits * trace_off[p] + h * trace_cap[p]
  // the options, behind everything a search without them reads (every field above keeps its offset); read by the OPT
  // kernels only
  const int32_t* min_scores;  // [npairs] by pair id, or NULL: spec.min_score for every pair
  int32_t flags;        // bialign_hit_spec.flags: BIALIGN_HITS_PEAKS
  int32_t min_permille; // bialign_batch_set_hit_thresholds: 0..1000, 0 when none are set
  bool options() const { return flags != 0 || min_permille != 0 || min_scores != nullptr; }
};

// dynamic LDS of a launch: staged inputs, mask bitset, accepted spans (start, end) per hit
inline size_t fit_hits_lds(const HitArgs& h) { return (size_t)h.lds_inputs + 4 * (size_t)h.mask_words + 8 * (size_t)h.max_hits; }

// ceil(min_permille * Emax / 1000) for Emax > 0, else 0: Emax is the maximum of the pair's profile.  Every lane reads back
// the words it stored itself (behind the kernel's s_waitcnt and barrier), one wave_min64 on the negated maximum follows.
__device__ inline int permille_threshold(const int32_t* prof, int m, int c, int min_permille) {
  int emax = -0x7fffffff;
  for (int j = c; j <= m; j += 64) emax = max(emax, prof[j]);
  emax = -wave_min64(-emax);
  return emax > 0 ? (int)(((int64_t)min_permille * emax + 999) / 1000) : 0;
}

// The peak rule: every end that is no peak of the profile is masked before the first round (the mask is zero on entry).
// A block of 64 ends per trip, a lane per end; the neighbours' words were stored by other lanes of this wave, ahead of the
// kernel's s_waitcnt and barrier.  The ballot of "no peak" is the block's two mask words, stored by lanes 0 and 32.  The
// bits of ends beyond m are set: no loop looks at them, and set they say what they are, no candidates.
__device__ inline void mask_non_peaks(const int32_t* prof, uint32_t* mask, int m, int c) {
  const int words = (m + 32) >> 5;
  for (int j0 = 0; j0 <= m; j0 += 64) {
    const int j = j0 + c;
    bool peak = false;
    if (j <= m) {
      const int e = prof[j];
      peak = (j == 0 || prof[j - 1] < e) && (j == m || prof[j + 1] <= e);
    }
    const unsigned long long out = __ballot(!peak);
    const int t = (j0 >> 5) + (c >> 5);
    if ((c & 31) == 0 && t < words) mask[t] = (uint32_t)(out >> (c & 32));
  }
}

// The model is stated in include/bialign.h ("Hit search"); this is it, step by step.  All control flow is wave-uniform:
// every branch tests values that came out of a wave reduction, a readlane, or the kernel arguments.
// OPT: the search reads its options (HitArgs::options(): peak candidates, per-pair thresholds).  With OPT false the kernel
// is, text for text, the search as it was before the options existed, and a search with no option set launches that one.
template <int S, bool AFFINE, bool PACK, bool D1, bool OPT>
__global__ void __launch_bounds__(64) fit_hits_kernel(const DeviceBatch A, const HitArgs H, int npairs) {
  static_assert(!PACK || (AFFINE && !D1), "packed records: affine sweeps, not with dense mu1");
  const int pid = A.order[blockIdx.x];
  const PairDesc pd = A.pairs[pid];
  const int n = pd.n, m = pd.m;
  const int c = threadIdx.x;
  const int32_t* lay = A.layers;
  constexpr int BIG = 0x7fffffff;
  extern __shared__ __align__(16) int32_t smem[];
  uint32_t* mask = reinterpret_cast<uint32_t*>(smem) + H.lds_inputs / 4;  // bit j: end j is no candidate any more
  int32_t* spans = reinterpret_cast<int32_t*>(mask + H.mask_words);       // accepted hits: (start, end)

  // the tracebacks' own cell addressing, packed and full
  auto cell9 = [&](int pi, int pj, int a, int b, int ss) -> int {
    if (PACK) return packed_cell<S>(lay, pd, pi, pj, a, b, ss);
    return lay[cell_dword<S, 9>(pd, pi, pj, a, b, ss)];
  };
  auto cell1 = [&](int pi, int pj, int a, int b) -> int { return lay[cell_dword<S, 1>(pd, pi, pj, a, b, 0)]; };
  auto never = [](int, int, int, int) { return false; };

  // Profile: E(j), FIT's end value of row n.  Lanes stride over j; plain vector stores.
  int32_t* prof = H.profile + H.prof_off[pid];
  for (int j = c; j <= m; j += 64) {
    int e;
    if constexpr (AFFINE) {
      e = cell9(n, j, S, S, 0);
      for (int q = 1; q < 9; ++q) e = max(e, cell9(n, j, S, S, q));
    } else {
      e = cell1(n, j, S, S);
    }
    prof[j] = e;
  }
  if (!H.search) return;  // a fill-only run: status stays NOT_SEARCHED

  const int words = (m + 32) >> 5;
  for (int t = c; t < words; t += 64) mask[t] = 0;
  const TraceInputs in = stage_trace_inputs<D1>(A, pd, smem);
  const int32_t* const mu1tab = D1 ? mu1_table(A, pd) : nullptr;
  __builtin_amdgcn_s_waitcnt(0);  // the profile's stores before the rounds read it
  __syncthreads();
  // What the options add stands behind the barrier, under kernel arguments.  The pair's threshold: T_p = max(base_p,
  // ceil(min_permille * Emax_p / 1000)), the second term only for Emax_p > 0; without options it is min_score.
  int thresh = H.min_score;
  if constexpr (OPT) {
    if (H.min_scores) thresh = H.min_scores[pid];
    if (H.min_permille) thresh = max(thresh, permille_threshold(prof, m, c, H.min_permille));
    if (H.flags & BIALIGN_HITS_PEAKS) {
      mask_non_peaks(prof, mask, m, c);
      __syncthreads();  // the mask before the first round reads it
    }
  }

  uint8_t* const tbase = H.trace + (int64_t)H.max_hits * pd.trace_off;
  int32_t* const hit_rec = H.hits + (int64_t)pid * H.max_hits * 4;
  int32_t* const walk_rec = H.walks + (int64_t)pid * H.max_walks * 4;
  int nhits = 0, nwalks = 0, status;
  while (true) {
    // 1. the best unmasked candidate at or above the pair's threshold, the smallest j on a tie
    int bv = -BIG, bx = 0;
    for (int j = c; j <= m; j += 64) {
      const int e = prof[j];
      const bool masked = (mask[j >> 5] >> (j & 31)) & 1u;
      if (!masked && e >= thresh && e > bv) bv = e, bx = j;
    }
    const int best = -wave_min64(-bv);
    if (best == -BIG) { status = BIALIGN_HITS_EXHAUSTED; break; }
    const int je = wave_min64(bv == best ? bx : BIG);

    // 2. FIT's walk from (n, je, n, je), into the next free slot
    uint8_t* const out = tbase + (int64_t)nhits * pd.trace_cap;
    WalkPoint w{n, je, n, je, 0, best, 0, 0, 0};
    int how;
    if constexpr (AFFINE) {
      int endv;
      affine_end_state(cell9, n, je, S, c, &endv, &w.st);
      w.cur = endv;
      how = walk_affine<D1>(A, pd, in, mu1tab, S, c, true, false, false, cell9, never, out, pd.trace_cap, w);
    } else {
      how = walk_linear<D1>(A, pd, in, mu1tab, S, c, true, false, false, cell1, never, out, pd.trace_cap, w);
    }
    const int start = w.j;
    const int len = min(w.len, pd.trace_cap);

    // 3. accepted if complete and disjoint from every accepted span
    int meets = 0;
    for (int h = c; h < nhits; h += 64) meets |= (start < spans[2 * h + 1] && spans[2 * h] < je) ? 1 : 0;
    const bool accept = how == WALK_COMPLETE && wave_min64(meets ? 0 : 1) != 0;
    if (accept) reverse_trace(out, len, c);
    // mask start < x <= je and je itself (accepted), or je alone: a lane per mask word
    const int lo = accept ? min(start + 1, je) : je;
    for (int t = (lo >> 5) + c; t <= (je >> 5); t += 64) {
      const int first = max(lo, 32 * t) - 32 * t, last = min(je, 32 * t + 31) - 32 * t;
      mask[t] |= (0xffffffffu >> (31 - last)) & (0xffffffffu << first);
    }
    if (c == 0) {
      if (accept) {
        spans[2 * nhits] = start, spans[2 * nhits + 1] = je;
        int32_t* r = hit_rec + 4 * nhits;
        r[0] = start, r[1] = je, r[2] = best, r[3] = len;
      }
      // 4. the log, in every case
      int32_t* r = walk_rec + 4 * (int64_t)nwalks;
      r[0] = je, r[1] = start, r[2] = best, r[3] = accept ? 1 : 0;
    }
    __syncthreads();  // mask and spans before the next round reads them
    // 5.
    ++nwalks;
    if (accept) ++nhits;
    if (nhits == H.max_hits) { status = BIALIGN_HITS_MAX_HITS; break; }
    if (nwalks == H.max_walks) { status = BIALIGN_HITS_MAX_WALKS; break; }
  }
  if (c == 0) {
    int32_t* hd = H.head + 4 * (int64_t)pid;
    hd[0] = nhits, hd[1] = nwalks, hd[2] = status;
    if constexpr (OPT) hd[3] = thresh;
  }
}

// The search of pairs order[first .. first+count) on the engine's stream (bialign_hits.hip): the kernel of the batch's
// recurrence, max_shift and of the record form the chunk's sweep has just stored.
int launch_fit_hits(const bialign_batch* b, const DeviceBatch& v, const HitArgs& h, int first, int count);

}  // namespace bialign
