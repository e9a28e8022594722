// bialign_host.hpp -- host-side internals shared by the translation units of libbialign_hip.so:
// the batch / engine objects behind the C ABI and the kernel launchers.
//   Launching: launch() (LDS attribute, launch, error), launch_team() (the same with progress words in HBM and, for
// cross-CU teams, one such launch at a time per device), xcu_resident() (occupancy of a cross-CU grid).
//   Kernel variants are named by flag words (FillFlags, TraceFlags) through fill_affine_of / fill_linear_of /
// traceback_*_of; which variants exist is stated once (fill_affine_exists, fill_linear_exists, fill_slim_exists,
// traceback_exists), and one ladder per recurrence picks the launch for a team shape.
//   The launchers are templates on max_shift; each (max_shift, kind) is instantiated in its own translation unit
// (bialign_inst.hip, compiled once per -DBIALIGN_TU_S / -DBIALIGN_TU_KIND) so that the kernels build in parallel;
// bialign_capi.hip only dispatches.  What a batch IS on the host -- its plan -- lives in bialign_plan.hpp (BatchPlan).
#pragma once
#include "bialign_plan.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

namespace bialign {

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(BIALIGN_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                \
  } while (0)

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  hipError_t alloc(size_t count) {
    release();
    n = count;
    return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
  }
  hipError_t upload(const T* src, size_t count, hipStream_t s) {
    hipError_t e = alloc(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
  }
};

}  // namespace bialign

using bialign::DevBuf;
using bialign::DeviceBatch;
using bialign::PairDesc;
using bialign::TraceState;

struct bialign_engine {
  int device = 0;
  int num_cu = 256;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // uploads of new batches: not ordered behind running sweeps
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // Layer buffer kept between batches: hipMalloc / hipFree of tens of GB cost 0.1-6 s, the
  // sweep itself ~20 ms.  A batch takes it at creation when it is large enough and hands
  // the larger of (its own, the cached one) back at destruction; bialign_engine_trim frees it.
  int live_batches = 0;   // batches created on this engine and not yet destroyed
  bool closing = false;   // bialign_engine_destroy was called while batches were alive: the last one finishes the job
  DevBuf<int32_t> layer_cache;
  DevBuf<int32_t> layer_cache2;  // second slot: filled only when two batches were alive at once (pipelined use)
  DevBuf<int32_t> tab_cache;     // FEATURE-form batches: the per-chunk mu2 table buffer of the last one, kept likewise
};

// Every HIP event that times a batch, and the time they gave each stage (fill_ms is the sweeps' alone).  A run marks points
// on the stream as it enqueues; a mark may end a stage, which then began at the mark before it, so adjacent stages share a
// mark (a chunk's fill end is its traceback start).  finish() waits for the last mark, whichever stage it ends, and adds up
// every stage.  Events are created as marks need them and kept for the next run, which may need fewer (a re-planned batch).
enum class Stage { Shuffle, Tables, Fill, Traceback, Hits, Stats, None };
struct StageClock {
  std::vector<hipEvent_t> pool;
  std::vector<Stage> ends;  // the marks of the pending / last run: pool[0 .. ends.size()), and the stage each ends
  double total[(int)Stage::None] = {};
  ~StageClock() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
  void reset() { ends.clear(), std::fill(std::begin(total), std::end(total), 0.0); }
  hipError_t mark(hipStream_t st, Stage stage_ended = Stage::None) {
    if (ends.size() == pool.size()) {
      hipEvent_t e = nullptr;
      if (hipError_t err = hipEventCreate(&e)) return err;
      pool.push_back(e);
    }
    ends.push_back(stage_ended);
    return hipEventRecord(pool[ends.size() - 1], st);
  }
  hipError_t finish() {
    std::fill(std::begin(total), std::end(total), 0.0);
    if (!ends.empty())
      if (hipError_t err = hipEventSynchronize(pool[ends.size() - 1])) return err;
    for (size_t k = 1; k < ends.size(); ++k) {
      if (ends[k] == Stage::None) continue;
      float f = 0;
      if (hipError_t err = hipEventElapsedTime(&f, pool[k - 1], pool[k])) return err;
      total[(int)ends[k]] += f;
    }
    return hipSuccess;
  }
  double ms(Stage stage) const { return total[(int)stage]; }
};

struct bialign_batch : bialign::BatchPlan {  // the plan (bialign_plan.hpp), and what lives on the device
  bialign_engine* eng = nullptr;
  DevBuf<PairDesc> d_pairs;
  DevBuf<int32_t> d_order, d_s1, d_s2, d_layers, d_scores, d_tlen, d_complete, d_err, d_prog;
  // free ends (BatchPlan::free_ends): [npairs][4] spans, -1 ahead of every run.  Fit: the first 2 * npairs words as
  // [npairs][2] = (start_b, end_b); local and overlap: (start_a, end_a, start_b, end_b)
  DevBuf<int32_t> d_span;
  DevBuf<unsigned long long> d_end_key;  // BatchPlan::end_key: [npairs] best-end keys, zeroed ahead of every run
  int last_team = 1;  // waves per pair of the last fill launch (negative: cross-CU team)
  // Cross-CU teams need every workgroup of the launch resident at once.  The grid is sized from the
  // occupancy the runtime reports for the actual kernel (xcu_resident, cached per LEAN flavour) and
  // launches of this kind are serialised across the engines of a process; if a hand-off still times
  // out (another tenant on the device), the run is repeated with in-workgroup teams (no_xcu).
  int xcu_resident[4] = {-1, -1, -1, -1};  // [LEAN + 2 * (eight-wave workgroups)]
  bool used_xcu = false;   // a fill launch of the pending / last run was a cross-CU team
  bool no_xcu = false;     // a cross-CU launch of this batch failed once: in-workgroup teams from now on
  int recovered = 0;       // runs repeated after a hand-off timeout
  int xcu_spin_limit = 1 << 20;  // polls before a cross-CU wave gives up (~1 s); BIALIGN_XCU_SPIN_LIMIT: tests
  uint32_t pending_flags = 0;
  bool used_pack = false;       // a fill launch of the pending / last run stored packed records (BatchPlan::pack)
  bool packed_layers = false;   // ... and so did the launch whose layers are in the buffer now
  DevBuf<uint8_t> d_seq_a, d_cls_a, d_seq_b, d_cls_b, d_trace;
  DevBuf<TraceState> d_tstate;
  // Score tables.  Dense forms: d_tab holds all pairs' n x m tables (per pair mu2's, then mu1's; PairDesc::tab_off).
  // FEATURE form of mu2 (bialign_batch_create_features, bialign_mu2_build.hpp): per-residue doubles in HBM, d_tab is
  // per-chunk scratch the builder kernel fills ahead of each chunk's sweep; PairDesc::tab_off is chunk-relative.
  struct Tables {
    DevBuf<int32_t> d_tab;
    DevBuf<double> d_feat_a, d_feat_b;  // three planes each (up, down, unp), feat_tot_a / feat_tot_b doubles per plane
    int64_t feat_tot_a = 0, feat_tot_b = 0;
    DevBuf<int32_t> d_mu1;      // a dense mu1 next to feature mu2: its tables stay resident here, pair after pair,
    DevBuf<int64_t> d_mu1_off;  // ... and the builder copies a chunk's behind the mu2 tables it writes
    int build_launches = 0;     // table builds (Stage::Tables) of the pending / last run
  } tables;
  // Null batch (bialign_batch_create_null, bialign_null.hpp): d_seq_b / d_cls_b are the replica buffers the shuffle kernel
  // fills ahead of a run's sweeps from the uploaded B codes kept in d_seq / d_cls (real pair p's at d_off[p]).
  //   FEATURE form (bialign_batch_create_null_features): tables.d_feat_b holds the replica planes (feat_tot_b = R * sum of
  // len_b doubles per plane, indexed by the virtual pairs' seq_b like d_seq_b), shuffle_features_kernel fills them and
  // d_seq_b from the uploaded B features kept in d_feat, three planes of d_seq.n doubles; d_cls_b stays zero.
  //   DENSE form (bialign_batch_create_null_dense): the real pairs' tables stay resident in d_tab (pair p's at d_tab_off[p]:
  // mu2's, then mu1's), d_perm holds every replica's permutation (uint16, indexed like d_seq_b; shuffle_index_kernel fills
  // it), and tables.d_tab is per-chunk scratch as in FEATURE form, with the same plan fields, stage and launch count:
  // permute_tables_kernel writes each chunk's tables there ahead of its sweep.  The rest of a null batch is BatchPlan::null_*.
  struct Null {
    DevBuf<uint8_t> d_seq, d_cls;
    DevBuf<int64_t> d_off, d_tab_off;
    DevBuf<double> d_feat;
    DevBuf<int32_t> d_tab;
    DevBuf<uint16_t> d_perm;
    DevBuf<int32_t> d_obs;               // observed scores of the last bialign_batch_get_null_stats
    DevBuf<bialign_null_stats> d_stats;  // ... and its result
    StageClock stats_clock;              // ... and its time: the reduction runs outside a run, and leaves the run's marks alone
    int32_t model = BIALIGN_NULL_MONO;   // bialign_batch_set_null_model: which permutation the shuffle kernels make
  } null;
  // Hit search (bialign_batch_set_hits, bialign_hits.hpp): the spec (max_walks resolved) and the result buffers of the whole
  // batch, reset ahead of every run.  on false: a run touches none of this.
  struct Hits {
    bool on = false;
    bool pending = false, ran = false;  // the pending run enqueues searches; the last completed run filled the result buffers
    bialign_hit_spec spec{};
    DevBuf<int32_t> d_profile, d_head, d_rec, d_walks;  // HitArgs::profile, head, hits, walks
    DevBuf<int64_t> d_prof_off;
    DevBuf<uint8_t> d_trace;
    std::vector<int64_t> prof_off;  // [npairs + 1]
    int mask_words = 0;             // HitArgs::mask_words
    int64_t bytes = 0;
    // bialign_batch_set_hit_thresholds: the per-pair array (by pair id; empty: spec.min_score) and the permille
    DevBuf<int32_t> d_min_scores;
    int32_t min_permille = 0;
    void release() {
      on = ran = false;
      min_permille = 0;
      for (DevBuf<int32_t>* d : {&d_profile, &d_head, &d_rec, &d_walks, &d_min_scores}) d->release();
      d_prof_off.release();
      d_trace.release();
      bytes = 0;
    }
  } hits;
  StageClock clock;  // the stage times of the pending / last run (bialign_batch_wait copies fill and traceback into timing)
  bialign_timing timing{};
  bool ran = false, ran_trace = false;
  bool pending = false, pending_trace = false;  // an enqueued run not yet waited for
  hipEvent_t uploaded = nullptr;                // inputs are in HBM (recorded on the copy stream)
  ~bialign_batch() { if (uploaded) (void)hipEventDestroy(uploaded); }

  DeviceBatch view() const {
    DeviceBatch v{};
    v.pairs = d_pairs.p;
    v.order = d_order.p;
    v.seq_a = d_seq_a.p; v.cls_a = d_cls_a.p; v.seq_b = d_seq_b.p; v.cls_b = d_cls_b.p;
    v.s1 = d_s1.p; v.s2 = d_s2.p;
    v.k1 = k1; v.k2 = k2;
    v.beta = prm.gap_opening_cost; v.gamma = prm.gap_cost; v.delta = prm.shift_cost;
    v.layers = d_layers.p;
    v.scores = d_scores.p;
    v.trace = d_trace.p;
    v.trace_len = d_tlen.p;
    v.complete = d_complete.p;
    v.errflag = d_err.p;
    v.dense_tab = (dense || dense1) ? tables.d_tab.p : nullptr;
    v.dense_forms = (dense ? 1 : 0) | (dense1 ? 2 : 0);
    v.scratch = d_layers.p;  // a pair's scratch records follow its LEAN records in the same buffer
    // the wide-band affine sweep's ring follows the largest chunk's layers there (BatchPlan::ring_dwords; alloc_layers)
    v.wide_ring = ring_dwords.empty() ? nullptr : d_layers.p + max_chunk_dwords;
    v.wide_score_only = !ring_dwords.empty() && lean ? 1 : 0;
    v.tstate = d_tstate.p;
    v.resw_k = level_trace ? wide_seg : resw_k;
    v.wide_s = S;
    v.prio_mode = getenv("BIALIGN_PRIO") ? atoi(getenv("BIALIGN_PRIO")) : 1;
    v.spin_limit = 1 << 20;  // waves of one workgroup are co-resident by construction: a timeout there is a bug
    // whose end gaps are free in the sweeps of the global recurrence: B's (fit), both molecules' (overlap)
    v.free_ends = mode == bialign::AlignMode::Fit       ? bialign::FREE_B_ENDS
                  : mode == bialign::AlignMode::Overlap ? bialign::FREE_B_ENDS | bialign::FREE_A_ENDS
                                                        : 0;
    v.local = mode == bialign::AlignMode::Local;
    v.reserved0 = nullptr;
    v.span = d_span.p;
    v.end_key = d_end_key.p;
    return v;
  }
};

namespace bialign {

// Cross-CU launches of all engines of this process on one device run one after the other (each needs
// the whole device's wave slots): the stream waits for the previous such launch, the new one is recorded.
int xcu_serial_begin(bialign_engine* e);
int xcu_serial_end(bialign_engine* e);

// FEATURE form of mu2: build the tables of pairs order[first .. first+count) into the chunk's table buffer, on the
// engine's stream (bialign_mu2_build.hip).  The pairs' tab_off must be the device's.
int launch_build_mu2(bialign_batch* b, int first, int count);

// Null batch (bialign_null.hip): write the replicas of virtual pairs first .. first + count into the replica buffers, and
// reduce every real pair's replica scores (d_scores) into null.d_stats; both on the engine's stream.
int launch_shuffle_null(bialign_batch* b, int first, int count);
// DENSE-form null batch: permute the real tables' columns into the chunk's table buffer for virtual pairs
// order[first .. first+count), on the engine's stream; launch_shuffle_null must have written their permutations.
int launch_permute_tables(bialign_batch* b, int first, int count);
int launch_null_stats(bialign_batch* b, const int32_t* d_observed);

// Hit search (bialign_hits.hip): what a launch is given (search false: the profile only); its results' state ahead of a run
struct HitArgs;
HitArgs hit_args(const bialign_batch* b, bool search);
int reset_hits(bialign_batch* b, hipStream_t st);

// ---- launching: every kernel of the library starts through launch() or launch_team()
// Dynamic LDS beyond 64 KiB has to be allowed per kernel, ahead of a launch or an occupancy query.
template <typename... P>
hipError_t allow_lds(void (*kern)(P...), size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
template <typename... P, typename... A>
hipError_t try_launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  if (hipError_t e = allow_lds(kern, lds)) return e;
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  return hipGetLastError();
}
template <typename... P, typename... A>
int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  HIP_TRY(try_launch(kern, grid, block, lds, st, args...));
  return BIALIGN_OK;
}

// A launch whose workgroups hand over to each other through progress words in HBM (DeviceBatch::prog, PROG_WORDS per
// pair, zeroed per launch).  serial: they sit on different CUs and wait for each other, so all of them must be resident
// at once -- such launches run one at a time per device (xcu_serial_begin / _end) and mark the run for the fallback.
template <typename... P, typename... X>
int launch_team(bialign_batch* b, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, DeviceBatch w, int count,
                bool serial, const X&... extra) {
  const size_t words = (size_t)count * PROG_WORDS;
  if (b->d_prog.n < words) HIP_TRY(b->d_prog.alloc(words));
  HIP_TRY(hipMemsetAsync(b->d_prog.p, 0, words * sizeof(int32_t), b->eng->stream));
  w.prog = b->d_prog.p;
  w.spin_limit = b->xcu_spin_limit;
  if (!serial) return launch(kern, grid, block, lds, b->eng->stream, w, extra...);
  b->used_xcu = true;
  if (int rc = xcu_serial_begin(b->eng)) return rc;
  const hipError_t launched = try_launch(kern, grid, block, lds, b->eng->stream, w, extra...);
  const int rc = xcu_serial_end(b->eng);  // always: it releases the launch lock
  if (launched == hipSuccess && rc) return rc;
  HIP_TRY(launched);
  return BIALIGN_OK;
}

// Workgroups of `block` threads with `lds` bytes of kernel `kern` the device can hold at once, from the runtime's
// occupancy calculation for the actual code object (registers, LDS): the cap of a grid whose workgroups wait for each
// other.  0 when the runtime cannot tell.
template <typename... P>
int xcu_resident(const bialign_batch* b, void (*kern)(P...), int block, size_t lds) {
  int per_cu = 0;
  if (allow_lds(kern, lds) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), block, lds) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return per_cu * b->eng->num_cu;
}
// ... asked once per batch and cache slot (bialign_batch::xcu_resident; a batch is either DENSE or not); 0 once the
// batch has fallen back from cross-CU teams
template <typename... P>
int xcu_resident_cached(bialign_batch* b, int slot, void (*kern)(P...), int block, size_t lds) {
  if (b->no_xcu) return 0;
  int& cached = b->xcu_resident[slot];
  if (cached < 0) cached = xcu_resident(b, kern, block, lds);
  return cached;
}

// A run-time flag word as a compile-time one: fn(std::integral_constant<unsigned, flags & MASK>{}), one bit at a time.
template <unsigned MASK, unsigned F = 0, typename Fn>
int with_flags(unsigned flags, Fn&& fn) {
  if constexpr (MASK == 0) {
    return fn(std::integral_constant<unsigned, F>{});
  } else {
    constexpr unsigned BIT = MASK & (~MASK + 1);
    return (flags & BIT) ? with_flags<(MASK & ~BIT), (F | BIT)>(flags, fn) : with_flags<(MASK & ~BIT), F>(flags, fn);
  }
}

// ---- the kernels' variants by name.  The kernel templates take rows of positional booleans; the host names a variant
//      by a flag word and these functions are the only places that spell the rows out.
enum FillFlags : unsigned {
  F_XCU = 1,        // cross-CU team: gw workgroups per pair
  F_DENSE = 2,      // mu2 from dense tables
  F_LEAN = 4,       // LEAN records
  F_RESW = 8,       // strip re-sweep of the lean traceback
  F_PACK = 16,      // packed records (Pack<S>)
  F_DENSE1 = 32,    // mu1 from dense tables
  F_BETA_ANY = 64,  // affine: gap_opening_cost > 0, the general-beta algebra
  F_LOCAL = 128,    // local alignments (BIALIGN_BATCH_LOCAL)
};
enum TraceFlags : unsigned {
  T_TRACE = 1,   // walk back and write the trace (else: the score only)
  T_STRIP = 2,   // lean traceback: one strip's walk through the scratch records
  T_WIDE = 4,    // wide-band layers (bialign_wide.hpp)
  T_PACK = 8,    // packed records (affine)
  T_DENSE1 = 16, // mu1 from dense tables
  T_LEVEL = 32,  // level-checkpointed traceback: one segment's walk through the level-major scratch (bialign_wide.hpp)
};

// The instantiation plan: which sweeps exist, as (max_shift, waves per workgroup, flags).
constexpr bool fill_affine_exists(int S, int TW, unsigned F) {
  const bool xcu = F & F_XCU, dense = F & (F_DENSE | F_DENSE1), pack = F & F_PACK;
  // local alignments: in-workgroup sweeps of one wave, and of four up to s=3, in all four dense/lookup forms, full and LEAN
  if (F & F_LOCAL) return !(F & (F_XCU | F_PACK | F_RESW | F_BETA_ANY)) && (TW == 1 || (TW == 4 && S <= 3));
  // packed records: max_shift 1..BIALIGN_MAX_SHIFT_PACKED, full storage, not with dense mu1
  if (pack && (S < 1 || S > BIALIGN_MAX_SHIFT_PACKED || (F & (F_LEAN | F_DENSE1)))) return false;
  // re-sweeps and the (rare) general-beta algebra: one wave per pair, full (re-sweeps) or any (beta) records
  if (F & (F_RESW | F_BETA_ANY)) return TW == 1 && !xcu && !pack && !((F & F_RESW) && (F & F_LEAN));
  if (TW == 1) return !xcu || !dense || S <= 3;           // cross-CU teams of the dense forms: up to s=3
  if (TW == 8) return !dense && (xcu ? S == 2 : S <= 2);  // LOOKUP only (s=2: the DIET layout, also as a cross-CU team)
  return (TW == 4 || TW == 2) && !xcu && S <= 3;          // s >= 4 needs nearly all 512 registers of a SIMD lane: one wave per pair
}
constexpr bool fill_linear_exists(int TW, unsigned F) {
  if (F & (F_PACK | F_BETA_ANY)) return false;
  // local alignments, the analogous cut: one wave, and four in LOOKUP form
  if (F & F_LOCAL) return !(F & (F_XCU | F_RESW)) && (TW == 1 || (TW == 4 && !(F & (F_DENSE | F_DENSE1))));
  if (F & (F_RESW | F_XCU)) return TW == 1 && (F & (F_RESW | F_XCU)) != (F_RESW | F_XCU) && !((F & F_RESW) && (F & F_LEAN));
  return TW == 1 || TW == 2 || (!(F & (F_DENSE | F_DENSE1)) && (TW == 4 || TW == 8));  // dense forms: up to two waves
}
// fill_affine_slim_kernel: max_shift 1, LOOKUP scores, LEAN or packed records, teams of 2, 3, 6 or 12 waves
constexpr bool fill_slim_exists(int S, unsigned F) { return S == 1 && (F == F_LEAN || F == F_PACK); }
constexpr bool traceback_exists(bool affine, int S, unsigned F) {
  if ((F & T_PACK) && (!affine || S < 1 || S > BIALIGN_MAX_SHIFT_PACKED || (F & ~(T_PACK | T_TRACE)))) return false;
  if (F & T_LEVEL) return S == 0 && (F & ~T_DENSE1) == (T_LEVEL | T_TRACE);
  if (F & T_STRIP) return (F & T_TRACE) && !(F & T_WIDE);
  return !(F & T_DENSE1) || (F & T_TRACE);  // (without the walk no score is read: the LOOKUP kernels serve)
}

template <int S, int TW, unsigned F>
auto fill_affine_of() {
  static_assert(fill_affine_exists(S, TW, F), "not in the instantiation plan");
  return fill_affine_kernel<S, !(F & F_BETA_ANY), TW, (F & F_XCU) != 0, (F & F_DENSE) != 0, (F & F_LEAN) != 0, (F & F_RESW) != 0,
                            (F & F_PACK) != 0, (F & F_DENSE1) != 0, (F & F_LOCAL) != 0>;
}
template <int S, int TW, unsigned F>
auto fill_linear_of() {
  static_assert(fill_linear_exists(TW, F), "not in the instantiation plan");
  return fill_linear_kernel<S, TW, (F & F_DENSE) != 0, (F & F_LEAN) != 0, (F & F_RESW) != 0, (F & F_XCU) != 0, (F & F_DENSE1) != 0,
                            (F & F_LOCAL) != 0>;
}
template <int S, unsigned F>
auto traceback_affine_of() {
  static_assert(traceback_exists(true, S, F), "not in the instantiation plan");
  return traceback_affine_kernel<S, (F & T_TRACE) != 0, (F & T_STRIP) != 0, (F & T_WIDE) != 0, (F & T_PACK) != 0, (F & T_DENSE1) != 0,
                                 (F & T_LEVEL) != 0>;
}
template <int S, unsigned F>
auto traceback_linear_of() {
  static_assert(traceback_exists(false, S, F), "not in the instantiation plan");
  return traceback_linear_kernel<S, (F & T_TRACE) != 0, (F & T_STRIP) != 0, (F & T_WIDE) != 0, (F & T_DENSE1) != 0, (F & T_LEVEL) != 0>;
}

// the flags a batch fixes for its sweeps
inline unsigned fill_flags(const bialign_batch* b) {
  return (b->dense ? F_DENSE : 0u) | (b->dense1 ? F_DENSE1 : 0u) | (b->lean ? F_LEAN : 0u) | (b->pack_now() ? F_PACK : 0u) |
         (b->affine && b->prm.gap_opening_cost > 0 ? F_BETA_ANY : 0u);
}
// dynamic LDS of a TW-wave workgroup of the tiled sweeps
template <int S, int TW>
size_t fill_lds(const bialign_batch* b, bool affine) {
  return (affine && S == 2 && TW == 8) ? b->lds_diet8 : b->lds_base + (size_t)TW * b->lds_per_wave;
}

// ---- affine sweeps
template <int S, int TW, unsigned F>
int launch_fill_affine_t(bialign_batch* b, const DeviceBatch& v, int first, int count, int gw) {
  constexpr bool XCU = (F & F_XCU) != 0, PACK = (F & F_PACK) != 0;
  DeviceBatch w = v;
  w.order = v.order + first;
  w.team = gw;
  b->packed_layers = PACK;
  if (PACK) b->used_pack = true;
  b->last_team = XCU ? -TW * gw : TW;
  const dim3 grid(count * (XCU ? gw : 1)), block(64 * TW);
  if (XCU) return launch_team(b, fill_affine_of<S, TW, F>(), grid, block, fill_lds<S, TW>(b, true), w, count, true);
  return launch(fill_affine_of<S, TW, F>(), grid, block, fill_lds<S, TW>(b, true), b->eng->stream, w);
}

template <int S, int TW, bool LEAN>
int launch_fill_affine_slim_t(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  constexpr int PPW = 12 / TW;  // pairs per twelve-wave workgroup
  DeviceBatch w = v;
  w.order = v.order + first;
  w.team = 1;
  w.launch_pairs = count;
  w.slim_code_bytes = (int32_t)b->lds_slim_codes;
  b->packed_layers = !LEAN;
  if (!LEAN) b->used_pack = true;
  b->last_team = TW;
  return launch(fill_affine_slim_kernel<S, TW, PPW, LEAN>, dim3((count + PPW - 1) / PPW), dim3(64 * 12), b->lds_slim(TW),
                b->eng->stream, w);
}

template <int S, bool LEAN>
int launch_fill_affine_slim(bialign_batch* b, const DeviceBatch& v, int first, int count, int tw) {
  switch (tw) {
    case 2: return launch_fill_affine_slim_t<S, 2, LEAN>(b, v, first, count);
    case 3: return launch_fill_affine_slim_t<S, 3, LEAN>(b, v, first, count);
    case 6: return launch_fill_affine_slim_t<S, 6, LEAN>(b, v, first, count);
    case 12: return launch_fill_affine_slim_t<S, 12, LEAN>(b, v, first, count);
  }
  return fail(BIALIGN_E_UNSUPPORTED, "no three-waves-per-SIMD sweep for max_shift %d, team %d", S, tw);
}

// One-wave (TW = 8: eight-wave, the s=2 DIET layout) workgroups of the sweep's cross-CU kernel the device holds at
// once; 0 where there is no such kernel.  Asked of the full-record kernel also when the sweep packs.
template <int S, int TW, unsigned F>
int xcu_resident_affine(bialign_batch* b) {
  constexpr unsigned Q = (F & ~F_PACK) | F_XCU;
  if constexpr (fill_affine_exists(S, TW, Q)) {
    if (TW == 8 && !diet8_available(*b)) return 0;
    return xcu_resident_cached(b, ((F & F_LEAN) ? 1 : 0) + (TW == 8 ? 2 : 0), fill_affine_of<S, TW, Q>(), 64 * TW, fill_lds<S, TW>(b, true));
  } else {
    return 0;
  }
}

// One rung of the ladder: the TW-wave kernel (F_XCU in F: cross-CU teams of such workgroups), if it is in the
// instantiation plan and the shape asks for at least that much.  True: launched, *rc is the outcome.
template <int S, int TW, unsigned F>
bool fill_affine_rung(bialign_batch* b, const DeviceBatch& v, int first, int count, const TeamShape& ts, int* rc) {
  if constexpr (fill_affine_exists(S, TW, F)) {
    constexpr bool XCU = (F & F_XCU) != 0;
    if (XCU ? !(ts.gw > 1 && (TW == 1 || ts.tw == TW)) : ts.tw < TW) return false;
    *rc = launch_fill_affine_t<S, TW, F>(b, v, first, count, XCU ? ts.gw : 1);
    return true;
  } else {
    return false;
  }
}

// The sweep of pairs order[first .. first+count): the team shape, then the first rung of "cross-CU eight-wave, cross-CU,
// 8, 4, 2, 1" that exists for this (max_shift, form) and fits the shape.  bialign_batch::last_team is what was launched.
// (team_shape() never returns more than exists: the dense forms, capped at four waves, report 1 at s >= 4 like the rest.)
template <int S>
int launch_fill_affine(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return with_flags<F_DENSE | F_LEAN | F_PACK | F_DENSE1 | F_BETA_ANY>(fill_flags(b), [&](auto flags) -> int {
    constexpr unsigned F = decltype(flags)::value;
    if constexpr (!fill_affine_exists(S, 1, F)) {
      return fail(BIALIGN_E_UNSUPPORTED, "no affine sweep for max_shift %d in form %u", S, F);
    } else {
      TeamShape ts;  // general beta: one wave per pair
      if constexpr (!(F & F_BETA_ANY)) ts = team_shape(*b, first, count, b->eng->num_cu, xcu_resident_affine<S, 1, F>(b), xcu_resident_affine<S, 8, F>(b));
      if constexpr (fill_slim_exists(S, F)) {
        if (ts.slim) return launch_fill_affine_slim<S, (F & F_LEAN) != 0>(b, v, first, count, ts.tw);
      }
      int rc = BIALIGN_OK;
      (void)(fill_affine_rung<S, 8, F | F_XCU>(b, v, first, count, ts, &rc) || fill_affine_rung<S, 1, F | F_XCU>(b, v, first, count, ts, &rc) ||
             fill_affine_rung<S, 8, F>(b, v, first, count, ts, &rc) || fill_affine_rung<S, 4, F>(b, v, first, count, ts, &rc) ||
             fill_affine_rung<S, 2, F>(b, v, first, count, ts, &rc) || fill_affine_rung<S, 1, F>(b, v, first, count, ts, &rc));
      return rc;
    }
  });
}

// Local alignments (BatchPlan::own_sweeps): the LOCAL instantiations, in translation units of their own (kind 2).  The team
// shape comes without cross-CU teams, slim sweeps and packed records (team_shape, decide_pack); the ladder is "4, 1".
template <int S>
int launch_fill_affine_local(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return with_flags<F_DENSE | F_LEAN | F_DENSE1>(fill_flags(b) & ~(unsigned)(F_PACK | F_BETA_ANY), [&](auto flags) -> int {
    constexpr unsigned F = decltype(flags)::value | F_LOCAL;
    const TeamShape ts = team_shape(*b, first, count, b->eng->num_cu, 0);
    int rc = BIALIGN_OK;
    (void)(fill_affine_rung<S, 4, F>(b, v, first, count, ts, &rc) || fill_affine_rung<S, 1, F>(b, v, first, count, ts, &rc));
    return rc;
  });
}

// Lean traceback, one round: re-sweep the strip every unfinished pair's walk stands in ...
template <int S>
int launch_resweep_affine(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  DeviceBatch w = v;
  w.order = v.order + first;
  w.team = 1;
  return with_flags<F_DENSE | F_DENSE1 | F_BETA_ANY>(fill_flags(b), [&](auto flags) -> int {
    return launch(fill_affine_of<S, 1, decltype(flags)::value | F_RESW>(), dim3(count * b->resw_k), dim3(64), fill_lds<S, 1>(b, true),
                  b->eng->stream, w);
  });
}

// ---- tracebacks: one wave per pair.  The kernel is named by what the batch holds; the score-only form stages nothing.
inline unsigned trace_flags(const bialign_batch* b, bool do_trace) {
  return (do_trace ? T_TRACE : 0u) | (b->dense1 && do_trace ? T_DENSE1 : 0u) | (b->packed_layers ? T_PACK : 0u);
}
template <typename... P>
int launch_traceback_kernel(const bialign_batch* b, void (*kern)(P...), bool do_trace, const DeviceBatch& v, int first, int count) {
  DeviceBatch w = v;
  w.order = v.order + first;
  return launch(kern, dim3(count), dim3(64), do_trace ? b->lds_trace : 0, b->eng->stream, w, count);
}

// traceback_affine_fast_kernel (bialign_trace_fast.hpp) exists for the walk over packed records with LOOKUP scores
constexpr bool traceback_fast_exists(int S, unsigned F) { return F == (T_TRACE | T_PACK) && traceback_exists(true, S, F); }
// ... and admits a pair whose storage stays below 2^31 dwords and whose two-strip window of packed records stays below
// 2^32 bytes: its cell addresses are 32-bit byte offsets from the record 0 of the strip above the walk's
template <int S>
bool trace_fast_admits(const PairDesc& d) {
  using TF = TraceFast<S>;
  return Pack<S>::pair_dwords(d.G, d.P, d.m) < (int64_t(1) << 31) &&
         (2 * (int64_t)d.P + Geo<S>::MAXOFF + TF::W + 2) * TF::RECB < (int64_t(1) << 32);
}
// LDS of a launch of the fast kernel: the staged inputs, the candidate table, and the trace buffer -- the longest trace
// of the launch if the workgroup can spare it (BIALIGN_TRACE_LDS: tests, a smaller buffer), else flushed in pieces.
// 0: the generic kernel serves (BIALIGN_TRACE_FAST=0: tests / A-B; dense mu2; a FIT or LOCAL batch; a pair not admitted).
constexpr int TRACE_FAST_TBUF_MAX = 16 * 1024;
// Ring records of the walk's LDS window (TraceWindow<S>), 0: the kernel without the window (BIALIGN_TRACE_WINDOW=0: tests /
// A-B; the window would not fit).  It is taken where the ring ends within the 64 KB an LDS-DMA's m0 addresses, and where it
// costs no workgroup that the launch needs resident: as many per CU as without it, or all of the launch at once.
// BIALIGN_TRACE_WINDOW_K (tests): a shorter ring, down to the one without lead.
template <int S>
int trace_window_records(const bialign_batch* b, int count, size_t fixed, int tbuf) {
  using TW = TraceWindow<S>;
  const char* sw = getenv("BIALIGN_TRACE_WINDOW");
  if (sw && atoi(sw) == 0) return 0;
  int k = TW::K;
  if (const char* e = getenv("BIALIGN_TRACE_WINDOW_K"))
    while (k > TW::KMIN && k > atoi(e)) k /= 2;
  const size_t lds = 160 * 1024, with = fixed + TW::lds_bytes(k);
  if (with > 64 * 1024 || with + 64 > lds) return 0;
  const size_t res_with = lds / (with + tbuf), res_without = lds / (fixed + tbuf);
  const size_t needed = ((size_t)count + b->eng->num_cu - 1) / std::max(b->eng->num_cu, 1);
  return res_with >= std::min(res_without, needed) ? k : 0;
}
template <int S>
size_t trace_fast_lds(const bialign_batch* b, int first, int count, int* tbuf, int* wk) {
  const char* sw = getenv("BIALIGN_TRACE_FAST");  // "0": tests / A-B, the generic kernel only
  if ((sw && atoi(sw) == 0) || b->dense || b->dense1 || b->wide || b->lean) return 0;
  if (b->free_ends()) return 0;  // fit, local and overlap alignments take the generic walk: the short-chain kernel has neither the end rules nor the stop rules
  int cap = 0;
  for (int t = first; t < first + count; ++t) {
    const PairDesc& d = b->pairs[b->order[t]];
    if (!trace_fast_admits<S>(d)) return 0;
    cap = std::max(cap, d.trace_cap);
  }
  int want = std::min((cap + 63) & ~63, TRACE_FAST_TBUF_MAX);
  if (const char* e = getenv("BIALIGN_TRACE_LDS")) want = std::min(want, std::max(64, atoi(e) & ~63));
  size_t fixed = ((b->lds_trace + 15) & ~size_t(15)) + TraceFast<S>::TAB_BYTES;
  if (fixed + 64 > 160 * 1024) return 0;
  *wk = 0;
  if constexpr (TraceWindow<S>::EXISTS) *wk = trace_window_records<S>(b, count, fixed, want);
  if (*wk) fixed += TraceWindow<S>::lds_bytes(*wk);
  *tbuf = (int)std::min<size_t>(want, (160 * 1024 - fixed) & ~size_t(63));
  return fixed + *tbuf;
}

template <int S>
int launch_traceback_affine(const bialign_batch* b, const DeviceBatch& v, int first, int count, bool do_trace) {
  return with_flags<T_TRACE | T_PACK | T_DENSE1>(trace_flags(b, do_trace), [&](auto flags) -> int {
    constexpr unsigned F = decltype(flags)::value;
    if constexpr (traceback_fast_exists(S, F)) {
      int tbuf = 0, wk = 0;
      if (const size_t lds = trace_fast_lds<S>(b, first, count, &tbuf, &wk)) {
        DeviceBatch w = v;
        w.order = v.order + first;
        if constexpr (TraceWindow<S>::EXISTS)
          if (wk) return launch(traceback_affine_fast_kernel<S, true>, dim3(count), dim3(64), lds, b->eng->stream, w, count, tbuf, wk);
        return launch(traceback_affine_fast_kernel<S, false>, dim3(count), dim3(64), lds, b->eng->stream, w, count, tbuf, 0);
      }
    }
    if constexpr (traceback_exists(true, S, F)) return launch_traceback_kernel(b, traceback_affine_of<S, F>(), do_trace, v, first, count);
    else return fail(BIALIGN_E_UNSUPPORTED, "no affine traceback for max_shift %d in form %u", S, F);
  });
}
// ... the lean traceback's walk through the strip just re-swept
template <int S>
int launch_traceback_affine_strip(const bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return b->dense1 ? launch_traceback_kernel(b, traceback_affine_of<S, T_TRACE | T_STRIP | T_DENSE1>(), true, v, first, count)
                   : launch_traceback_kernel(b, traceback_affine_of<S, T_TRACE | T_STRIP>(), true, v, first, count);
}

// ---- one-layer sweeps
template <int S, int TW, unsigned F>
int launch_fill_linear_t(bialign_batch* b, const DeviceBatch& v, int first, int count, int gw) {
  constexpr bool XCU = (F & F_XCU) != 0;
  DeviceBatch w = v;
  w.order = v.order + first;
  w.team = gw;
  b->packed_layers = false;
  b->last_team = XCU ? -gw : TW;
  const dim3 grid(count * (XCU ? gw : 1)), block(64 * TW);
  if (XCU) return launch_team(b, fill_linear_of<S, TW, F>(), grid, block, fill_lds<S, TW>(b, false), w, count, true);
  return launch(fill_linear_of<S, TW, F>(), grid, block, fill_lds<S, TW>(b, false), b->eng->stream, w);
}

template <int S, int TW, unsigned F>
bool fill_linear_rung(bialign_batch* b, const DeviceBatch& v, int first, int count, const TeamShape& ts, int* rc) {
  if constexpr (fill_linear_exists(TW, F)) {
    constexpr bool XCU = (F & F_XCU) != 0;
    if (XCU ? ts.gw <= 1 : ts.tw < TW) return false;
    *rc = launch_fill_linear_t<S, TW, F>(b, v, first, count, XCU ? ts.gw : 1);
    return true;
  } else {
    return false;
  }
}

// as launch_fill_affine: cross-CU, 8, 4, 2, 1
template <int S>
int launch_fill_linear(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return with_flags<F_DENSE | F_LEAN | F_DENSE1>(fill_flags(b), [&](auto flags) -> int {
    constexpr unsigned F = decltype(flags)::value;
    const int resident = xcu_resident_cached(b, (F & F_LEAN) ? 1 : 0, fill_linear_of<S, 1, F | F_XCU>(), 64, fill_lds<S, 1>(b, false));
    const TeamShape ts = team_shape(*b, first, count, b->eng->num_cu, resident);
    int rc = BIALIGN_OK;
    (void)(fill_linear_rung<S, 1, F | F_XCU>(b, v, first, count, ts, &rc) || fill_linear_rung<S, 8, F>(b, v, first, count, ts, &rc) ||
           fill_linear_rung<S, 4, F>(b, v, first, count, ts, &rc) || fill_linear_rung<S, 2, F>(b, v, first, count, ts, &rc) ||
           fill_linear_rung<S, 1, F>(b, v, first, count, ts, &rc));
    return rc;
  });
}

// local alignments, as launch_fill_affine_local: 4, 1
template <int S>
int launch_fill_linear_local(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return with_flags<F_DENSE | F_LEAN | F_DENSE1>(fill_flags(b), [&](auto flags) -> int {
    constexpr unsigned F = decltype(flags)::value | F_LOCAL;
    const TeamShape ts = team_shape(*b, first, count, b->eng->num_cu, 0);
    int rc = BIALIGN_OK;
    (void)(fill_linear_rung<S, 4, F>(b, v, first, count, ts, &rc) || fill_linear_rung<S, 1, F>(b, v, first, count, ts, &rc));
    return rc;
  });
}

template <int S>
int launch_resweep_linear(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  DeviceBatch w = v;
  w.order = v.order + first;
  return with_flags<F_DENSE | F_DENSE1>(fill_flags(b), [&](auto flags) -> int {
    return launch(fill_linear_of<S, 1, decltype(flags)::value | F_RESW>(), dim3(count * b->resw_k), dim3(64), fill_lds<S, 1>(b, false),
                  b->eng->stream, w);
  });
}

template <int S>
int launch_traceback_linear(const bialign_batch* b, const DeviceBatch& v, int first, int count, bool do_trace) {
  return with_flags<T_TRACE | T_DENSE1>(trace_flags(b, do_trace), [&](auto flags) -> int {
    constexpr unsigned F = decltype(flags)::value;
    if constexpr (traceback_exists(false, S, F)) return launch_traceback_kernel(b, traceback_linear_of<S, F>(), do_trace, v, first, count);
    else return fail(BIALIGN_E_UNSUPPORTED, "no one-layer traceback for max_shift %d in form %u", S, F);
  });
}
template <int S>
int launch_traceback_linear_strip(const bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return b->dense1 ? launch_traceback_kernel(b, traceback_linear_of<S, T_TRACE | T_STRIP | T_DENSE1>(), true, v, first, count)
                   : launch_traceback_kernel(b, traceback_linear_of<S, T_TRACE | T_STRIP>(), true, v, first, count);
}

template <int S, int NL>
int launch_dump(const bialign_batch* b, const DeviceBatch& v, int pid, int32_t* d_out) {
  if constexpr (S >= 1 && S <= BIALIGN_MAX_SHIFT_PACKED && NL == 9) {
    if (b->packed_layers) return launch(dump_layers_kernel<S, NL, true>, dim3(256), dim3(256), 0, b->eng->stream, v, pid, d_out);
  }
  return launch(dump_layers_kernel<S, NL>, dim3(256), dim3(256), 0, b->eng->stream, v, pid, d_out);
}

// ---- wide-band path (max_shift above BIALIGN_MAX_SHIFT_TILED, bialign_wide.hpp): runtime band width,
//      one translation unit (bialign_wide.hip) for all of it
int launch_fill_wide(bialign_batch* b, const DeviceBatch& v, int first, int count);
int launch_traceback_wide(const bialign_batch* b, const DeviceBatch& v, int first, int count, bool do_trace);
// level-checkpointed traceback, one round: sweep the segment every unfinished pair's walk stands in, then walk through it
int launch_segment_wide(bialign_batch* b, const DeviceBatch& v, int first, int count);
int launch_traceback_level(const bialign_batch* b, const DeviceBatch& v, int first, int count);
int launch_dump_wide(const bialign_batch* b, const DeviceBatch& v, int pid, int32_t* d_out);

// ---- instantiation plan: kind 0 = affine fill (the big kernels), kind 1 = everything else, kind 2 = the LOCAL sweeps
#define BIALIGN_INST_KIND0(S, X)                                                                \
  X template int launch_fill_affine<S>(bialign_batch*, const DeviceBatch&, int, int);          \
  X template int launch_resweep_affine<S>(bialign_batch*, const DeviceBatch&, int, int);
#define BIALIGN_INST_KIND1(S, X)                                                                         \
  X template int launch_fill_linear<S>(bialign_batch*, const DeviceBatch&, int, int);                   \
  X template int launch_traceback_affine<S>(const bialign_batch*, const DeviceBatch&, int, int, bool);  \
  X template int launch_traceback_affine_strip<S>(const bialign_batch*, const DeviceBatch&, int, int);  \
  X template int launch_traceback_linear<S>(const bialign_batch*, const DeviceBatch&, int, int, bool);  \
  X template int launch_resweep_linear<S>(bialign_batch*, const DeviceBatch&, int, int);                \
  X template int launch_traceback_linear_strip<S>(const bialign_batch*, const DeviceBatch&, int, int);  \
  X template int launch_dump<S, 9>(const bialign_batch*, const DeviceBatch&, int, int32_t*);            \
  X template int launch_dump<S, 1>(const bialign_batch*, const DeviceBatch&, int, int32_t*);

#define BIALIGN_INST_KIND2(S, X)                                                                \
  X template int launch_fill_affine_local<S>(bialign_batch*, const DeviceBatch&, int, int);    \
  X template int launch_fill_linear_local<S>(bialign_batch*, const DeviceBatch&, int, int);

#ifndef BIALIGN_TU_S  // every other unit: the instantiations live elsewhere
BIALIGN_FOR_EACH_S(BIALIGN_INST_KIND0, extern)
BIALIGN_FOR_EACH_S(BIALIGN_INST_KIND1, extern)
BIALIGN_FOR_EACH_S(BIALIGN_INST_KIND2, extern)
#endif

}  // namespace bialign
