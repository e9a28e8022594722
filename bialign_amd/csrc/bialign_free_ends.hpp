// bialign_free_ends.hpp -- what the free-end modes (BIALIGN_BATCH_FIT, _OVERLAP, _LOCAL) share on the device: the mask of
// free end gaps and the floor words it sets, the per-pair end key the sweeps raise and the kernel that decodes it, and the
// end rule of the score-only sweeps.  Part of bialign_kernels.hpp (include that, not this).
#pragma once

namespace bialign {

// DeviceBatch::free_ends: whose end gaps are free in the sweeps that serve the global recurrence.  FIT sets FREE_B_ENDS,
// OVERLAP both; LOCAL sets neither (its sweeps are built for it: template parameter LOCAL).
constexpr int32_t FREE_B_ENDS = 1, FREE_A_ENDS = 2;
// The last of a workgroup's progress words (teams have at most twelve waves) holds the floor under the value at the
// lattice points (0, j, 0, j): 0 where B's end gaps are free (FREE_B_ENDS: a path may start there), else the sentinel,
// under which no value of a lattice point lies.  The sweeps' prologue writes it; boundary steps read it back where row 0
// is computed, so the mode costs the interior loops neither a register nor an instruction.
constexpr int FIT_FLOOR_WORD = LDS_PROG_WORDS - 1;
// The one before it holds the same floor for the lattice points (i, 0, i, 0): 0 where A's end gaps are free (FREE_A_ENDS,
// an overlap batch, where FIT_FLOOR_WORD is 0 as well), else the sentinel.
constexpr int COL0_FLOOR_WORD = LDS_PROG_WORDS - 2;
// the prologue's value of progress word t (threads 0 .. LDS_PROG_WORDS-1): the two floor words, zero for the teams' words
__device__ __forceinline__ int32_t prog_word_init(int t, int32_t free_ends) {
  if (t == FIT_FLOOR_WORD) return (free_ends & FREE_B_ENDS) ? 0 : SENT;
  if (t == COL0_FLOOR_WORD) return (free_ends & FREE_A_ENDS) ? 0 : SENT;
  return 0;
}

// The best end of a pair as one 64-bit key (DeviceBatch::end_key; LOCAL batches and score-only OVERLAP batches): the
// maximum score wins, then the smallest (i, j) row-major.  A zeroed key lies below every key a sweep produces (the origin
// alone gives score 0); n + m < 60 000 (END_KEY_MAX_NM, checked by the planner) keeps i * (m + 1) + j inside 32 bits.
constexpr int END_KEY_MAX_NM = 60000;
__host__ __device__ inline unsigned long long end_key_of(int32_t score, int i, int j, int m) {
  const uint32_t hi = (uint32_t)score + 0x80000000u;  // score + 2^31: order-preserving
  const uint32_t lo = 0xffffffffu - ((uint32_t)i * (uint32_t)(m + 1) + (uint32_t)j);
  return ((unsigned long long)hi << 32) | lo;
}

// LOCAL sweeps: what a lane with a == 0 holds of its row (i, ., i, .) between two folds: the best E of the row so far and
// the smallest column that attains it (the lane passes over its row's columns in order).  SENT: nothing seen.
struct RowBest {
  int best = SENT, col = 0;
  __device__ __forceinline__ void see(bool on, int e, int j) {
    const bool up = on && e > best;
    best = up ? e : best;
    col = up ? j : col;
  }
  // one vector atomicMax per lane that holds something; order-independent, so teams and strips fold as they come
  __device__ __forceinline__ void fold(unsigned long long* key, int i, int m) {
    if (best > SENT) atomicMax(key, end_key_of(best, i, col, m));
    best = SENT;
  }
};

// The end rule of the score-only (LEAN) sweeps of the global recurrence; fill_affine_slim_kernel and fill_linear_kernel
// call it in every step for the cell (i, col, i, col).  (fill_affine_kernel states the same rule in its own body, for the
// measured reason given there.)
//   owner:     the lane holds that cell: live && !ghost && aa == S.  A row has one owner per step, and a row's owner
//              passes over the columns in order, interior steps included -- which is why row n's best end and the
//              SMALLEST column that attains it can stay in its registers (best, best_col; a later column replaces them
//              only with a larger value).
//   end_value: the cell's end value E as a callable (affine: the maximum of the nine states; one layer: the value), so
//              that it is computed only where the rule reads it.
//   INTERIOR:  the step is an interior step.  Its owner lanes stay left of column m - S, so only a boundary step can be at
//              column m: everything that is written or folded there is compiled for boundary steps alone.
// Global: the cell (n, m) writes the score (pyx:509; one layer: pyx:471).  Fit (FREE_B_ENDS): row n's owner keeps the best end, and at column m
// writes it as the score and its column as end_b.  Overlap (both bits): the end cells are (i, m), i < n, and row n; every
// row's owner folds its cell on column m into the pair's key -- row n's owner its best -- and end_key_finish_kernel
// decodes the key behind the sweep.
template <bool INTERIOR, class EndValue>
__device__ __forceinline__ void lean_end_rule(const DeviceBatch& A, int pid, int n, int m, bool owner, bool act_row, int i,
                                              int col, int& best, int& best_col, EndValue&& end_value) {
  // (The lane predicates are combined with `&`, not `&&`, and the rows above n have an `if` of their own, not an `else`:
  // inlined, a chain of `&&` in an if / else-if becomes a nest of exec-mask branches that every step of a fit or overlap
  // batch walks through -- measured on fill_linear_kernel: 13.04 against 11.92 ms, with `&` 11.40.)
  const bool row_n = owner & (i == n);
  if (!A.free_ends) {
    if (!INTERIOR && (row_n & (col == m))) A.scores[pid] = end_value();
    return;
  }
  if (row_n & (INTERIOR | ((col >= 0) & (col <= m)))) {
    const int e = end_value();
    if (e > best) best = e, best_col = col;
    if (!INTERIOR && col == m) {
      if (A.free_ends & FREE_A_ENDS) {
        atomicMax(A.end_key + pid, end_key_of(best, n, best_col, m));
      } else {
        A.scores[pid] = best;
        A.span[2 * pid + 1] = best_col;
      }
    }
  }
  if (!INTERIOR && (A.free_ends & FREE_A_ENDS) && (owner & act_row & (i != n) & (col == m)))
    atomicMax(A.end_key + pid, end_key_of(end_value(), i, m, m));
}

// One thread per pair of the launch, behind its sweep in every storage mode: the key becomes the pair's score and end;
// the starts stay -1 until a traceback writes them.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) end_key_finish_kernel(const DeviceBatch A, int count) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= count) return;
  const int pid = A.order[t];
  const int m = A.pairs[pid].m;
  const unsigned long long key = A.end_key[pid];
  const uint32_t pos = 0xffffffffu - (uint32_t)key;
  const int i = (int)(pos / (uint32_t)(m + 1));
  A.scores[pid] = (int32_t)((uint32_t)(key >> 32) - 0x80000000u);
  int32_t* span = A.span + 4 * (int64_t)pid;
  span[0] = -1;
  span[1] = i;
  span[2] = -1;
  span[3] = (int)(pos - (uint32_t)i * (uint32_t)(m + 1));
}

}  // namespace bialign
