// bialign_local.hpp -- local alignments (BIALIGN_BATCH_LOCAL): the per-pair key the sweeps raise, and the kernel that
// decodes it.  Part of bialign_kernels.hpp (include that, not this).
#pragma once

namespace bialign {

// The best end of a pair as one 64-bit key: the maximum score wins, then the smallest (i, j) row-major.  A zeroed key
// lies below every key a sweep produces (the origin alone gives score 0); n + m < 60 000 (LOCAL_MAX_NM, checked by the
// planner) keeps i * (m + 1) + j inside 32 bits.
constexpr int LOCAL_MAX_NM = 60000;
__host__ __device__ inline unsigned long long local_key_of(int32_t score, int i, int j, int m) {
  const uint32_t hi = (uint32_t)score + 0x80000000u;  // score + 2^31: order-preserving
  const uint32_t lo = 0xffffffffu - ((uint32_t)i * (uint32_t)(m + 1) + (uint32_t)j);
  return ((unsigned long long)hi << 32) | lo;
}

// What a lane with a == 0 holds of its row (i, ., i, .) between two folds: the best E of the row so far and the smallest
// column that attains it (the lane passes over its row's columns in order).  SENT: nothing seen.
struct LocalBest {
  int best = SENT, col = 0;
  __device__ __forceinline__ void see(bool on, int e, int j) {
    const bool up = on && e > best;
    best = up ? e : best;
    col = up ? j : col;
  }
  // one vector atomicMax per lane that holds something; order-independent, so teams and strips fold as they come
  __device__ __forceinline__ void fold(unsigned long long* key, int i, int m) {
    if (best > SENT) atomicMax(key, local_key_of(best, i, col, m));
    best = SENT;
  }
};

// One thread per pair of the launch, behind its sweep in every storage mode: the key becomes the pair's score and end;
// the starts stay -1 until a traceback writes them.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) local_finish_kernel(const DeviceBatch A, int count) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= count) return;
  const int pid = A.order[t];
  const int m = A.pairs[pid].m;
  const unsigned long long key = A.local_key[pid];
  const uint32_t pos = 0xffffffffu - (uint32_t)key;
  const int i = (int)(pos / (uint32_t)(m + 1));
  A.scores[pid] = (int32_t)((uint32_t)(key >> 32) - 0x80000000u);
  int32_t* span = A.local_span + 4 * (int64_t)pid;
  span[0] = -1;
  span[1] = i;
  span[2] = -1;
  span[3] = (int)(pos - (uint32_t)i * (uint32_t)(m + 1));
}

}  // namespace bialign
