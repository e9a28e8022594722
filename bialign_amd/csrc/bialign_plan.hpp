// bialign_plan.hpp -- what the host decides about a batch, with no device call in it: argument checks, the int32 safety
// window, sweep geometry and LDS needs, packed records, the storage ladder (full -> LEAN / LEVEL), chunking under the
// HBM budget, and the team shape of a launch.  bialign_capi.hip calls these stage by stage around its allocations and
// uploads; tests/plan_check.hip calls the same functions on the CPU.
#pragma once
#include "bialign_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "../../include/bialign.h"

#define BIALIGN_MAX_SHIFT_PACKED 3  // packed layer records (Pack<S>) are instantiated for max_shift 1..3
#define BIALIGN_FOR_EACH_S(M, X) M(0, X) M(1, X) M(2, X) M(3, X) M(4, X) M(5, X)

namespace bialign {

int fail(int code, const char* fmt, ...);  // records the message bialign_last_error() returns (bialign_capi.hip)
enum class AlignMode { Global, Fit, Local, Overlap };

// The host's decisions about one batch.  bialign_batch (bialign_host.hpp) derives from it and adds what lives on the
// device: buffers, events, run state, the engine.
struct BatchPlan {
  bialign_params prm{};
  int affine = 0, NL = 1, S = 0;
  int npairs = 0;
  int k1 = 0, k2 = 0;
  std::vector<PairDesc> pairs;      // host mirror (layer_off valid for the pair's chunk)
  std::vector<int32_t> order;       // chunk-by-chunk launch order
  std::vector<int> chunk_begin;     // index into order, size nchunks+1
  int64_t cells = 0, trace_bytes = 0, max_chunk_dwords = 0;
  int64_t tot_a = 0, tot_b = 0, tot_tab = 0;  // extents of the code arrays and of the resident dense tables: what the upload copies
  std::vector<int64_t> pair_dwords;       // per pair: layer dwords in the batch's storage mode
  size_t lds_bytes = 0;                   // dynamic LDS of a one-wave workgroup
  size_t lds_base = 0, lds_per_wave = 0;  // team launches: lds_base + T * lds_per_wave
  size_t lds_diet8 = 0;                   // eight-wave workgroups of the s=2 affine kernel (DIET layout)
  // fill_affine_slim_kernel (bialign_fill_slim.hpp): twelve ghost rings + tables, and per pair of the workgroup its codes
  size_t lds_slim_base = 0, lds_slim_codes = 0;
  size_t lds_slim(int tw) const { return lds_slim_base + (size_t)(12 / tw) * lds_slim_codes; }
  size_t lds_trace = 0;                   // tracebacks: score tables + sequence codes
  // Packed records (Pack<S>, bialign_types.hpp): decided per batch at creation (affine, max_shift 1 or 2, LOOKUP,
  // full storage, beta <= 0, every pair long enough that most steps are interior); dropped for good when a sweep
  // meets an offset that does not fit 16 bits (device flag bit 2 -> the run is repeated with full records).
  bool pack = false, pack_failed = false;
  bool pack_now() const { return pack && !pack_failed; }
  bool packed_sizing = false;          // chunks and pair offsets were planned with the packed sizes
  std::vector<int64_t> full_dwords;    // per pair: dwords of its full-record form (for the fallback's re-plan)
  bool dense = false;       // mu2 in DENSE form (also set for the FEATURE form: its consumers are the DENSE ones)
  bool dense1 = false;      // mu1 in DENSE form (kernels with DENSE1 / D1 set; no packed records, no slim or diet sweeps)
  // FEATURE form of mu2 (bialign_batch_create_features, bialign_mu2_build.hpp): the table buffer is per-chunk scratch the
  // builder kernel fills ahead of each chunk's sweep; PairDesc::tab_off is chunk-relative.
  bool feat = false;
  int32_t feat_sw = 0;
  std::vector<int64_t> tab_dwords;     // per pair: table dwords in the chunk buffer (n*m; twice with a dense mu1 riding along)
  int64_t max_chunk_tab_dwords = 0;    // table dwords of the largest chunk
  // Null batch (bialign_batch_create_null, bialign_null.hpp): npairs above counts the VIRTUAL pairs, null_npairs real pairs x
  // null_R replicas, pair-major.  null_dense: the DENSE form, whose replicas' tables are per-chunk scratch like FEATURE's.
  int null_R = 0, null_npairs = 0;  // null_R == 0: not a null batch
  uint32_t null_seed = 0;
  int null_max_m = 0;               // longest B of the batch: sizes the shuffle's index array in LDS
  bool null_dense = false;
  bool tab_scratch() const { return feat || null_dense; }  // the table buffer is per-chunk scratch inside the chunk plan
  bool wide = false;        // max_shift above the tiled kernels: anti-diagonal path (bialign_wide.hpp), reference-order layers
  bool lean = false;        // LEAN records: the sweep keeps only the strip-bottom rows
  bool lean_trace = false;  // ... and tracebacks re-sweep one strip at a time into a scratch area
  // Level-checkpointed traceback of the wide-band path (BIALIGN_BATCH_LEVEL_TRACE, bialign_wide.hpp): `lean` is set too
  // (no full layers); a pair's region holds checkpoints, the scratch of one segment of wide_seg levels, and the ring.
  bool level_trace = false;
  int wide_seg = 0;
  // The wide-band affine sweep's ring of derived values outside the LEVEL forms (full storage and SCORE_ONLY;
  // bialign_wide.hpp): WIDE_RING levels per pair, per-chunk scratch behind the chunk's layers in the same buffer.  It counts
  // toward the budget like the tables above, not toward pair_dwords; a pair's chunk-relative offset is its
  // PairDesc::scratch_off.  (The one-layer sweep and the LEVEL forms have no such ring: the vector stays empty.)
  bool ring_scratch() const { return wide && affine && !level_trace; }
  std::vector<int64_t> ring_dwords;    // per pair (plan_storage); empty: no ring term
  int64_t max_chunk_ring_dwords = 0;   // ring dwords of the largest chunk
  int resw_k = 1;           // strips re-swept and walked per round (more when the batch has few pairs)
  // The alignment mode, one per batch (check_inputs).  Fit (BIALIGN_BATCH_FIT): free end gaps in B.  Local (BIALIGN_BATCH_LOCAL):
  // free ends in both molecules.  Overlap (BIALIGN_BATCH_OVERLAP): the global alignment whose end gaps are free in both
  // molecules.  What the host does differently for a mode it reads from the three properties below.
  AlignMode mode = AlignMode::Global;
  const char* mode_name() const {  // (for messages about a non-global mode)
    return mode == AlignMode::Fit ? "FIT" : mode == AlignMode::Local ? "LOCAL" : "OVERLAP";
  }
  // free ends: tiled bands, full storage or SCORE_ONLY; spans beside the scores; the generic tracebacks only (host:
  // trace_fast_lds); never the storage ladder's LEAN_TRACE rung (plan_storage: BIALIGN_E_NOMEM)
  bool free_ends() const { return mode != AlignMode::Global; }
  // sweeps of its own (launch_fill_*_local, best-end keys behind them): no packed records, slim kernel or cross-CU team
  // (decide_pack, slim_available, team_shape); beta <= 0 in the affine recurrence
  bool own_sweeps() const { return mode == AlignMode::Local; }
  // its sweeps raise the pair's best-end key (bialign_free_ends.hpp), which end_key_finish_kernel decodes behind them: local
  // alignments always, overlap alignments where no traceback prologue scans the end cells (SCORE_ONLY).  It sizes and
  // zeroes the key buffer, launches the finish kernel and bounds n + m (the key's position is 32 bits wide)
  bool end_key() const { return mode == AlignMode::Local || (mode == AlignMode::Overlap && lean); }
};

// What the host needs of the kernels' compile-time geometry, for a run-time (max_shift, recurrence): read from the types
// the kernels are built from, so a change there reaches the LDS sizes, layer strides and sweep lengths computed here.
struct SweepInfo {
  int W, R, RR, MAXOFF, PADB;   // Geo<S>
  int recdw, lean_recdw;        // dwords of a step's record, full and LEAN (Rec<S,NL>, Rec<S,NL,true>)
  int blk, min_goff;            // ghost feed: steps per prefetch block, age of a record when it is read
  int ring_dw, diet_ring_dw;    // ... dwords of a wave's ring, and in the DIET layout (half-length blocks)
  int ghost_np;                 // ... 16-byte pieces per (step, a)
  int slim_offtab_dw;           // ... fill_affine_slim_kernel: the workgroup's table of steady-block lane offsets
  int mu2_ring_dw, mu1_ring_dw; // dense-mu2 and dense-mu1 rings of a wave
  int xch_dw;                   // exchange array of a wave: NCOL lanes x (XCH_ROWS per band column, affine) W values
  // Pack<S>, affine sweeps of max_shift 1..BIALIGN_MAX_SHIFT_PACKED (elsewhere empty): first interior phase, dwords of a
  // full record, and the dwords a pair's packed records take and a sweep writes, from (G, P, m)
  int pack_lo = 0;
  int64_t pack_full_recdw = 0;
  int64_t (*pack_pair_dwords)(int, int, int) = nullptr;
  int64_t (*pack_written_dwords)(int, int, int) = nullptr;
};
template <int S, int NL>
constexpr SweepInfo sweep_info_of() {
  using G = Geo<S>;
  using GF = GhostFeed<S, NL>;
  SweepInfo g{G::W, G::R, G::RR, G::MAXOFF, G::PADB, Rec<S, NL>::RECDW, Rec<S, NL, true>::RECDW, GF::BLK, GF::MIN_GOFF,
              GF::RING_DW, GhostFeed<S, NL, false, 2>::RING_DW, GF::NP, slim_offtab_dw<S>(), Mu2Feed<S>::RING_DW, Mu1Feed<S>::RING_DW,
              (NL == 9 ? XCH_ROWS : 1) * G::W * NCOL};
  if constexpr (NL == 9 && S >= 1 && S <= BIALIGN_MAX_SHIFT_PACKED) {
    g.pack_lo = Pack<S>::LO;
    g.pack_full_recdw = Rec<S, 9>::RECDW;
    g.pack_pair_dwords = &Pack<S>::pair_dwords;
    g.pack_written_dwords = &Pack<S>::written_dwords;
  }
  return g;
}
#define BIALIGN_SWEEP_INFO(S, X) {sweep_info_of<S, 1>(), sweep_info_of<S, 9>()},
inline const SweepInfo g_sweep_info[][2] = {BIALIGN_FOR_EACH_S(BIALIGN_SWEEP_INFO, )};
#undef BIALIGN_SWEEP_INFO
// (the wide-band path has no tiles: an empty entry)
inline const SweepInfo& sweep_info(const BatchPlan& b) {
  static const SweepInfo none{};
  return b.wide ? none : g_sweep_info[b.S][b.affine ? 1 : 0];
}

// One launch shape: TW waves per workgroup, GW workgroups per pair (GW > 1 = cross-CU team).
struct TeamShape {
  int tw = 1, gw = 1;
  bool slim = false;  // the three-waves-per-SIMD kernel (fill_affine_slim_kernel), teams of tw = 2, 3, 6 or 12 waves
  int waves() const { return tw * gw; }
};
// fill_affine_slim_kernel exists for this batch: affine, max_shift 1, LOOKUP scores, beta <= 0, packed records, full storage
inline bool slim_available(const BatchPlan& b) {
  const char* sw = getenv("BIALIGN_SLIM");  // "0": tests / A-B, the two-wave kernels only
  const bool off = sw && atoi(sw) == 0;
  return !off && !b.own_sweeps() && b.affine && b.S == 1 && !b.dense && !b.dense1 && !b.wide && b.prm.gap_opening_cost <= 0 && (b.lean || b.pack_now());
}
inline bool diet8_available(const BatchPlan& b) {  // the eight-wave s=2 affine kernel and its LDS layout
  return b.affine && b.S == 2 && !b.dense && !b.dense1 && b.lds_diet8 <= 160 * 1024;
}

// Waves per pair.  More waves per pair = more waves per SIMD when a launch has fewer pairs than
// the chip has wave slots worth filling (256 CUs x 4 SIMDs x 2).  Wave w trails wave w-1 by
// `lag` steps and wave 0 may lead wave T-1 by at most P - lag, so T waves run without mutual
// waiting only if T*lag (+ margin) fits into P; every wave should also own at least two strips.
//  * in-workgroup teams (progress words in LDS): s<=1 kernels fit 2 waves/SIMD (TW<=8), s=2,3
//    need a whole SIMD's registers per wave (TW<=4), s>=4 one wave; LDS <= 160 KB per workgroup.
//  * cross-CU teams (one-wave workgroups, progress words in HBM, write-through stores): up to 32
//    waves per pair, used when even the largest in-workgroup team leaves most SIMDs idle (few,
//    long pairs).  Every workgroup of the launch must be resident at once (a wave spins on its
//    predecessor), so the grid is capped by the residency the runtime's occupancy calculation gives
//    for the actual kernel (xcu_resident; 0 = cross-CU teams not available for this launch).
// xcu_resident: one-wave workgroups of the cross-CU kernel the device holds at once (0: no such kernel);
// xcu8_resident: likewise its eight-wave workgroups (s=2 affine sweep only, else 0); num_cu: the device's compute units
inline TeamShape team_shape(const BatchPlan& b, int first, int count, int num_cu, int xcu_resident, int xcu8_resident = 0) {
  TeamShape ts;
  if (b.own_sweeps()) xcu_resident = xcu8_resident = 0;  // (local alignments) in-workgroup teams only
  const SweepInfo& geo = sweep_info(b);
  const int lag = 2 * (geo.R - 1) + 2 * geo.blk + 16;
  int fit_exact = PROG_WORDS;  // largest team the pairs of this launch allow: T*lag + 64 <= P (P >= 256), two strips per wave
  for (int t = first; t < first + count; ++t) {
    const PairDesc& d = b.pairs[b.order[t]];
    const int by_period = d.P >= 256 ? (d.P - 64) / lag : 1;
    fit_exact = std::max(1, std::min(fit_exact, std::min(by_period, d.NS / 2)));
  }
  int fit = 1;  // in-workgroup teams come in powers of two (kernel template parameter)
  while (fit * 2 <= fit_exact) fit *= 2;
  // LDS of a workgroup of t waves (the eight-wave s=2 affine kernel has its own, leaner layout)
  const bool diet8 = diet8_available(b);
  auto lds_of = [&](int t) { return (t == 8 && diet8) ? b.lds_diet8 : b.lds_base + (size_t)t * b.lds_per_wave; };
  // the one-layer (non-affine) kernel is small in registers at every s; the affine one fits two waves per
  // SIMD up to s=2 (s=2: eight waves only in the diet layout), one at s=3, and needs the whole SIMD beyond
  int tw = std::min(fit, !b.affine ? 8 : (b.S <= 1 ? 8 : (b.S == 2 ? (diet8 ? 8 : 4) : (b.S == 3 ? 4 : 1))));
  while (tw > 1 && lds_of(tw) > 160 * 1024) tw >>= 1;
  const bool any_dense = b.dense || b.dense1;
  if (any_dense) tw = std::min(tw, b.affine ? 4 : 2);  // dense kernels: up to 4 waves (affine), 2 (one layer) per workgroup
  // cross-CU teams (affine LOOKUP kernels only) take any size: the team is a runtime value there
  int gw = ((!b.affine || b.S <= 3 || !any_dense) && xcu_resident > 0) ? fit_exact : 1;  // (dense affine kernels: s <= 3)
  gw = std::max(1, std::min(gw, xcu_resident / std::max(count, 1)));
  // ... and, for the s=2 sweep, teams of eight-wave workgroups (one per CU, two waves per SIMD)
  int gw8 = (diet8 && xcu8_resident > 0) ? std::min(fit_exact / 8, xcu8_resident / std::max(count, 1)) : 0;

  const char* e = getenv("BIALIGN_TEAM");  // experiments / tests: "N" in-workgroup, "xN" cross-CU, "hN" N eight-wave workgroups
  if (e && !*e) e = nullptr;
  if (e && e[0] == 'x') {
    ts.gw = std::max(1, std::min(atoi(e + 1), gw));
    return ts;
  }
  if (e && e[0] == 'h') {
    if (gw8 >= 1 && tw == 8) {
      ts.tw = 8;
      ts.gw = std::max(1, std::min(atoi(e + 1), gw8));
    }
    return ts;
  }
  // in-workgroup: the smallest team that (nearly) maximises the waves running at once, given
  // how many workgroups of that size a CU holds (LDS, registers)
  // (registers: the one-layer kernels and the affine s=0 kernel (56) fit four waves per SIMD -- and four are measurably
  //  better than three for them, tools/occupancy_probe.py --, affine s=1 188-200 = two, counted as three here since round 1)
  const int waves_cu_regs = !b.affine ? 16 : (b.S == 0 ? 16 : (b.S == 1 ? 12 : (b.S == 2 ? 8 : 4)));
  auto concurrent = [&](int t) {
    const size_t lds = (lds_of(t) + 1023) / 1024 * 1024;
    const int wg_cu = (int)std::min<size_t>((160 * 1024) / lds, (size_t)(waves_cu_regs / t));
    // one workgroup per CU and more workgroups than CUs: they run in rounds, the last one partly empty (300 pairs x len 1024
    // as eight-wave workgroups: two rounds, 25.2 ms; cross-CU teams of six one-wave workgroups 20.1)
    if (wg_cu == 1 && count > num_cu) return (int64_t)count * t / ((count + num_cu - 1) / num_cu);
    return std::min<int64_t>((int64_t)count * t, (int64_t)num_cu * wg_cu * t);
  };
  // The three-waves-per-SIMD sweep (fill_affine_slim_kernel: 168 registers, no exchange array): teams of 2, 3, 6 or 12
  // waves in workgroups of twelve, one per CU.  Taken whenever it keeps at least as many waves running as the two-wave
  // kernels' best shape -- a SIMD runs three such waves at the per-wave speed of two (tools/valu_rate.hip).
  if (slim_available(b) && !(e && (e[0] == 'x' || e[0] == 'h'))) {
    // a workgroup = 12 waves = (12 / t) pairs x teams of t, one per CU: every SIMD holds exactly three waves
    auto conc_slim = [&](int t) { return std::min<int64_t>((int64_t)count * t, (int64_t)num_cu * 12); };
    auto fits = [&](int t) { return t <= fit_exact && b.lds_slim(t) <= 160 * 1024; };
    auto slim_rounds = [&](int t) { return (((int64_t)count * t + 11) / 12 + num_cu - 1) / num_cu; };
    auto slim_score = [&](int t) {  // waves at work, averaged over the launch
      int64_t strips = 0, slots = 0;
      for (int p = first; p < first + count; ++p) {
        const int ns = b.pairs[b.order[p]].NS;
        strips += ns;
        slots += (int64_t)(ns + t - 1) / t * t;
      }
      return (double)count * t / slim_rounds(t) * strips / std::max<int64_t>(slots, 1);
    };
    static const int sizes[] = {2, 3, 6, 12};  // (a one-wave team spills in hipcc's allocation: 168 registers + scratch)
    int pick = 0;
    if (e) {  // forced in-workgroup team: the slim kernel if it comes in that size
      const int want = atoi(e);
      for (int t : sizes)
        if (t == want && fits(t)) pick = t;
    } else {
      // the team that keeps most waves at work over the launch: workgroups beyond one per CU run in rounds (all pairs of a
      // launch sweep about equally long), and a team of t idles in a pair's last round unless t divides its strips
      // (2048 pairs x len 512: teams of 2 = 342 workgroups = two rounds, the second a third full, 33.8 ms; teams of 3 =
      // two full rounds, 25.7 ms.  1280 pairs: teams of 2 in one round 16.5 ms, teams of 3 in two 21.8)
      double best_s = 0;
      for (int t : sizes)
        if (fits(t)) best_s = std::max(best_s, slim_score(t));
      for (int t : sizes)
        if (!pick && fits(t) && slim_score(t) >= best_s * 0.98) pick = t;
    }
    // what the two-wave kernels' in-workgroup teams keep running at best -- at the two waves per SIMD their registers
    // really allow (concurrent() counts three, a round-1 calibration of the choice AMONG those kernels)
    int64_t best_old = 0;
    for (int c = 1; c <= tw; c *= 2) {
      const size_t lds = (lds_of(c) + 1023) / 1024 * 1024;
      const int wg_cu = (int)std::min<size_t>((160 * 1024) / lds, (size_t)std::max(1, 8 / c));
      best_old = std::max(best_old, std::min<int64_t>((int64_t)count * c, (int64_t)num_cu * wg_cu * c));
    }
    if (pick && !e && conc_slim(pick) < best_old) pick = 0;  // (e.g. 256 pairs whose period admits teams of 6: 1536 waves against 2048)
    // More pairs than one round of twelve-wave workgroups holds: the two-wave kernel sweeps them with one wave each, every
    // strip count divides, and workgroups of one wave refill a CU as they finish.  Three slim waves do the work of 2.06
    // two-wave ones on a SIMD (headline shape: 46.0 against 46.5 ms at strip efficiencies 0.96 and 0.98); a fractional
    // last round of one-wave workgroups costs about half a round (3072 pairs x len 512: 13.0 ms per 1024 against 11.4 at
    // 2048).  Measured, ms per 1024 pairs x len 512, slim / two-wave: 2048 pairs 12.8 / 11.4, 3072 11.8 / 13.0, 4096 12.4 / 11.3
    // (profiles/r03w_exchange/slim_rounds_512.log).
    if (pick && !e && slim_rounds(pick) > 1) {
      const double x = std::max(1.0, (double)count / (num_cu * 8.0));  // rounds of one-wave workgroups, two per SIMD
      const double old_score = count / ((std::ceil(x) + x) / 2);
      if (slim_score(pick) * (2.06 / 3) < old_score) pick = 0;
    }
    if (pick) {
      // A handful of long pairs still go to cross-CU teams of the two-wave kernel below when that spreads them wider: a
      // third wave on a SIMD adds a few percent, an idle CU costs all of it (117 pairs x len 1024: teams of 12 on 117 CUs
      // 11.0 ms, cross-CU teams of 13 one-wave workgroups on all CUs 9.7).  Three slim waves count as 2.06 two-wave ones.
      const double run_s = conc_slim(pick) * (2.06 / 3);
      const int g = std::min(gw, std::max(1, 2048 / count));
      if (e || !(g >= 2 && (double)count * g >= run_s * 1.4)) {
        ts.tw = pick;
        ts.slim = true;
        return ts;
      }
    }
  }
  if (e) {
    int want = atoi(e), t = 1;
    while (t * 2 <= want && t * 2 <= tw) t *= 2;
    ts.tw = t;
    return ts;
  }
  // Two-wave workgroups of the s=2 affine kernel (256 registers, two such workgroups per CU) measured
  // 20-35 % slower per pair than one- or four-wave ones at the same number of resident waves
  // (tools/team_table.sh; not so at s=1 or s=3), so that sweep goes 1 -> 4.
  const bool skip2 = b.affine && b.S == 2 && tw >= 4;
  int64_t best = 0;
  for (int c = 1; c <= tw; c *= 2)
    if (!(skip2 && c == 2)) best = std::max(best, concurrent(c));
  int t = 1;
  while (t < tw && concurrent(t) * 100 < best * 95) t *= (skip2 && t == 1) ? 4 : 2;
  ts.tw = t;
  // cross-CU: when that keeps at least 1.4 x the waves running (117 pairs x len 1024: 16 one-wave workgroups per pair
  // instead of 8 waves in one, 12.9 -> 9.7 ms; 300 x len 512: 6 instead of 4, 7.6 -> 6.7 ms; at equal wave counts the
  // in-workgroup team wins: 256 x len 1024, 15.4 vs 16.8 ms) -- or, for a handful of pairs, not more waves but spread:
  // eight waves on eight CUs beat eight waves sharing one CU's SIMDs two by two (one 928 x 933 pair: 7.6 vs 9.4 ms)
  int64_t running = concurrent(t);
  {
    const int g = std::min(gw, std::max(1, 2048 / count));
    // (s=1 affine, the in-workgroup shape leaving a third of the wave slots empty: 1.2 x is enough -- 300 pairs x len 1024 as
    //  teams of 4 in one workgroup 23.3 ms, as eight-wave workgroups in two rounds 25.2, as cross-CU teams of 5 19.9)
    const bool sparse_s1 = b.affine && b.S == 1 && !any_dense && running * 100 < 2048 * 65;
    if (g >= 2 && ((int64_t)count * g * 10 >= running * (sparse_s1 ? 12 : 14) || (t == 8 && g >= 8 && count * 8 <= num_cu))) {
      ts.tw = 1;
      ts.gw = g;
      running = (int64_t)count * g;
    }
  }
  // s=2: eight-wave workgroups spread over CUs when that keeps more waves running than either of the above
  // (64 pairs x len 2000: 4 workgroups per pair = 2048 waves, two per SIMD, against 1024 one-wave workgroups)
  if (gw8 >= 2 && (int64_t)count * gw8 * 8 * 100 >= running * 125) {
    ts.tw = 8;
    ts.gw = gw8;
  }
  return ts;
}

// Sweep geometry of one pair: strips, period, steps.
inline void sweep_geometry(const SweepInfo& g, int n, int m, int* NS, int* P, int* G) {
  *NS = (n + 1 + g.RR - 1) / g.RR;
  // one idle column between strips (P >= m+2) and ghost records old enough to prefetch
  *P = std::max(m + 2, 2 * (g.R - 1) + g.min_goff);
  *G = (*NS - 1) * *P + m + g.MAXOFF + 1;
}

inline int64_t cells_of(int n, int m, int s) {
  auto K = [s](int x) {
    int64_t t = 0;
    for (int i = 0; i <= x; ++i) t += std::min(x, i + s) - std::max(0, i - s) + 1;
    return t;
  };
  return K(n) * K(m);
}

// Dynamic LDS of a sweep's workgroup of `team` waves: per wave a ghost ring, an exchange array and the rings of the dense
// forms; shared: progress words, score tables, the molecules' codes.
// diet: the eight-wave form of the s=2 affine kernel (fill_affine_kernel, DIET): half-length ghost blocks,
// molecule A's codes not staged.  dense1: a dense-mu1 ring per wave, no sequence codes staged.
struct LdsForm {
  bool dense = false, diet = false, dense1 = false;
};
inline size_t lds_need(const SweepInfo& g, int team, int k1, int k2, int n, int m, LdsForm f = {}) {
  const size_t npad = f.diet ? 0 : code_pad(n), mpad = code_pad(m, g.PADB);
  const size_t codes = f.dense1 ? npad + mpad : 2 * npad + 2 * mpad;  // (class codes only)
  const size_t wave_dw = (f.diet ? g.diet_ring_dw : g.ring_dw) + g.xch_dw + (f.dense ? g.mu2_ring_dw : 0) + (f.dense1 ? g.mu1_ring_dw : 0);
  const size_t shared_dw = LDS_PROG_WORDS + (size_t)k1 * k1 + (size_t)k2 * k2;
  return (team * wave_dw + shared_dw) * 4 + codes;
}

// fill_affine_slim_kernel (bialign_fill_slim.hpp), a workgroup of twelve waves: twelve ghost rings, a block of sentinels,
// progress words, the ghost feed's lane-offset table, score tables (lds_need_slim_base); per pair of the workgroup both molecules' codes (lds_need_slim_codes)
inline size_t lds_need_slim_base(const SweepInfo& g, int k1, int k2) {
  return (12 * (size_t)g.ring_dw + 4 * g.ghost_np + LDS_PROG_WORDS + g.slim_offtab_dw + (size_t)k1 * k1 + (size_t)k2 * k2) * 4;
}
inline size_t lds_need_slim_codes(const SweepInfo& g, int n, int m) { return 2 * (size_t)code_pad(n) + 2 * (size_t)code_pad(m, g.PADB); }

// Cut the batch into chunks of at most budget_dw dwords of layer storage and lay the pairs of each chunk end to
// end: as few chunks as the budget allows, of about equal size (an undersized last chunk would leave SIMDs
// idle); inside a chunk the longest sweeps are launched first.
//   FEATURE-form batches: a pair's mu2 table (BatchPlan::tab_dwords) is per-chunk scratch in a buffer of its own
// and counts toward the budget with the pair's layers; its tables lie end to end like the layers (PairDesc::tab_off).
// So do a replica's permuted tables in a DENSE-form null batch.
//   Wide-band affine batches outside the LEVEL forms: a pair's ring (BatchPlan::ring_dwords) is chunk scratch likewise, end
// to end from 0 behind the largest chunk's layers (PairDesc::scratch_off), and counts toward the budget.
// layer_cap / tab_cap: a re-plan within buffers the batch already holds -- neither kind may outgrow its buffer.
inline int plan_chunks(BatchPlan& b, const std::vector<int64_t>& pair_dwords, int64_t budget_dw, int64_t layer_cap = INT64_MAX,
                       int64_t tab_cap = INT64_MAX) {
  const int npairs = b.npairs;
  const bool feat = b.tab_scratch();  // (FEATURE form, and the DENSE-form null batch: its replicas' permuted tables)
  const bool ring = !b.ring_dwords.empty();
  auto tab_of = [&](int p) { return feat ? b.tab_dwords[p] : (int64_t)0; };
  auto ring_of = [&](int p) { return ring ? b.ring_dwords[p] : (int64_t)0; };
  b.order.resize(npairs);
  std::iota(b.order.begin(), b.order.end(), 0);
  b.chunk_begin.assign(1, 0);
  b.max_chunk_dwords = 0;
  b.max_chunk_tab_dwords = 0;
  b.max_chunk_ring_dwords = 0;
  int64_t total_dw = 0;
  for (int p = 0; p < npairs; ++p) {
    if (pair_dwords[p] + tab_of(p) + ring_of(p) > budget_dw) {
      // who asks (a real pair, or a replica of real pair p / R), and for what beside its layers
      const char* const who = b.null_R ? ": one replica" : "";
      const char* const tabs = b.null_dense ? "permuted tables" : "mu2 table";
      const long long lay = (long long)pair_dwords[p] * 4, tab = (long long)tab_of(p) * 4, bud = (long long)budget_dw * 4;
      const int shown = b.null_R ? p / b.null_R : p;
      if (ring) {  // (wide bands: the ring of the affine sweep, beside the tables where those are chunk scratch too)
        const long long rng = (long long)ring_of(p) * 4;
        return feat ? fail(BIALIGN_E_NOMEM, "pair %d%s needs %lld bytes of layers, %lld of %s and %lld of the wide-band ring, budget is %lld",
                           shown, who, lay, tab, tabs, rng, bud)
                    : fail(BIALIGN_E_NOMEM, "pair %d%s needs %lld bytes of layers and %lld of the wide-band ring, budget is %lld", shown, who,
                           lay, rng, bud);
      }
      return feat ? fail(BIALIGN_E_NOMEM, "pair %d%s needs %lld bytes of layers and %lld of %s, budget is %lld", shown, who, lay, tab, tabs, bud)
                  : fail(BIALIGN_E_NOMEM, "pair %d%s needs %lld bytes of layers, budget is %lld", shown, who, lay, bud);
    }
    total_dw += pair_dwords[p] + tab_of(p) + ring_of(p);
  }
  const int64_t want_chunks = (total_dw + budget_dw - 1) / budget_dw;
  const int64_t target_dw = std::min(budget_dw, (total_dw + want_chunks - 1) / want_chunks);
  int64_t used = 0, used_tab = 0, used_ring = 0;  // layer dwords, table dwords, ring dwords of the chunk so far
  for (int p = 0; p < npairs; ++p) {
    const int64_t all = used + used_tab + used_ring;
    if (all > 0 && (all + pair_dwords[p] + tab_of(p) + ring_of(p) > budget_dw || all >= target_dw ||
                    used + pair_dwords[p] > layer_cap || used_tab + tab_of(p) > tab_cap)) {
      b.chunk_begin.push_back(p);
      used = used_tab = used_ring = 0;
    }
    if (ring) {
      b.pairs[p].scratch_off = used_ring;  // (chunk-relative in the ring area, not an offset from the pair's layers)
      used_ring += ring_of(p);
      b.max_chunk_ring_dwords = std::max(b.max_chunk_ring_dwords, used_ring);
    } else {
      b.pairs[p].scratch_off += used - b.pairs[p].layer_off;  // (relative to the pair's start until the first plan)
    }
    b.pairs[p].layer_off = used;
    used += pair_dwords[p];
    b.max_chunk_dwords = std::max(b.max_chunk_dwords, used);
    if (feat) {
      b.pairs[p].tab_off = used_tab;
      used_tab += tab_of(p);
      b.max_chunk_tab_dwords = std::max(b.max_chunk_tab_dwords, used_tab);
    }
  }
  b.chunk_begin.push_back(npairs);
  for (size_t c = 0; c + 1 < b.chunk_begin.size(); ++c)
    std::stable_sort(b.order.begin() + b.chunk_begin[c], b.order.begin() + b.chunk_begin[c + 1],
                     [&](int x, int y) {
                       return b.wide ? b.pairs[x].n + b.pairs[x].m > b.pairs[y].n + b.pairs[y].m  // levels
                                      : b.pairs[x].G > b.pairs[y].G;
                     });
  return BIALIGN_OK;
}

// A re-plan at full-record sizes of a batch laid out for packed records, within the buffers it already holds: layers
// and (FEATURE form) tables each within their own, so the batch's HBM use does not grow.
inline int replan_full_layout(BatchPlan& b, int64_t layer_cap, int64_t tab_cap) {
  b.packed_sizing = false;
  return b.feat ? plan_chunks(b, b.full_dwords, layer_cap + tab_cap, layer_cap, tab_cap) : plan_chunks(b, b.full_dwords, layer_cap);
}

// What bialign_batch_create_null adds to the virtual pairs it hands on (expand_null_pairs): the real pairs' B molecules.
// (FEATURE- and DENSE-form null batches: the shuffle's index array in LDS is uint16, so len_b <= NULL_FEAT_MAX_M)
constexpr int NULL_FEAT_MAX_M = 65535;
struct NullPlan {
  int32_t replicas;
  uint32_t seed;
  int32_t npairs;                // real pairs
  const int64_t* off_b;          // [npairs] start of real pair p's B in seq_b / cls_b
  const uint8_t *seq_b, *cls_b;  // the B codes as the caller gave them (cls_b: nullptr in FEATURE form)
  int64_t tot_b;                 // their extent
  int32_t max_m;                 // the longest B
  // FEATURE form: ft->up_b / down_b / unp_b are the real pairs' planes, indexed by off_b above like seq_b
  // DENSE form (bialign_batch_create_null_dense): the virtual pairs' mu1_off / mu2_off are their real pair's, and the
  // tables are read through the first replica of each
  bool dense = false;
  // the virtual pairs (vp points into the arrays beside it) and their parameters: SCORE_ONLY
  std::vector<int32_t> len_a, len_b;
  std::vector<int64_t> off_a, v_off_b, mu1_off, mu2_off;
  bialign_pairs vp{};
  bialign_params vprm{};
};

// ---- the stages of a batch's creation, in the order bialign_capi.hip's create_batch() runs them

// Arguments and form: the recurrence, the storage flags and which of mu1 / mu2 come as tables.
// nul != nullptr: pr describes the virtual pairs of a null batch.
inline int check_inputs(const bialign_params* prm, const bialign_scoring* sc, const bialign_pairs* pr, const bialign_features* ft,
                        const NullPlan* nul, BatchPlan& b) {
  if (!prm || !sc || !pr) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (pr->npairs < 1) return fail(BIALIGN_E_INVALID, "npairs must be >= 1");
  if (prm->max_shift < 0) return fail(BIALIGN_E_INVALID, "max_shift must be >= 0");
  if (prm->max_shift > BIALIGN_MAX_SHIFT)
    return fail(BIALIGN_E_UNSUPPORTED, "max_shift %d > %d", prm->max_shift, BIALIGN_MAX_SHIFT);
  if (sc->k1 < 1 || sc->k1 > 256 || sc->k2 < 1 || sc->k2 > 256 || !sc->s1 || !sc->s2)
    return fail(BIALIGN_E_INVALID, "scoring tables: k1,k2 must be 1..256 and tables non-NULL");
  b.prm = *prm;
  if (prm->recurrence < BIALIGN_REC_AUTO || prm->recurrence > BIALIGN_REC_LINEAR)
    return fail(BIALIGN_E_INVALID, "recurrence must be 0 (auto), 1 (affine) or 2 (non-affine)");
  b.affine = prm->recurrence == BIALIGN_REC_AUTO ? prm->gap_opening_cost != 0  // pyx:204-205, 444
                                                  : prm->recurrence == BIALIGN_REC_AFFINE;
  b.NL = b.affine ? 9 : 1;
  b.S = prm->max_shift;
  b.npairs = pr->npairs;
  b.k1 = sc->k1;
  b.k2 = sc->k2;
  b.feat = ft != nullptr;
  b.dense = b.feat || pr->mu2_dense != nullptr;  // (the FEATURE form's tables feed the DENSE consumers)
  if (b.feat) b.feat_sw = ft->structure_weight;
  b.dense1 = pr->mu1_dense != nullptr;
  if (nul) b.null_R = nul->replicas, b.null_npairs = nul->npairs, b.null_seed = nul->seed, b.null_dense = nul->dense, b.null_max_m = nul->max_m;
  b.lean_trace = (prm->flags & BIALIGN_BATCH_LEAN_TRACE) != 0;
  b.lean = b.lean_trace || (prm->flags & BIALIGN_BATCH_SCORE_ONLY) != 0;
  b.wide = prm->max_shift > BIALIGN_MAX_SHIFT_TILED;  // bialign_wide.hpp: anti-diagonal path, all layers in HBM
  constexpr uint32_t KNOWN_FLAGS =
      BIALIGN_BATCH_SCORE_ONLY | BIALIGN_BATCH_LEAN_TRACE | BIALIGN_BATCH_LEVEL_TRACE | BIALIGN_BATCH_FIT | BIALIGN_BATCH_LOCAL |
      BIALIGN_BATCH_OVERLAP;
  if (prm->flags & ~KNOWN_FLAGS) return fail(BIALIGN_E_INVALID, "unknown bits 0x%x in bialign_params.flags", prm->flags & ~KNOWN_FLAGS);
  // the mode, decoded once.  Two bits at once are refused behind the free-ends refusals, which then name the first of FIT,
  // LOCAL, OVERLAP that is set: the order in which callers meet the refusals is part of the interface
  // (tests/mode_expected.txt)
  const bool fit = (prm->flags & BIALIGN_BATCH_FIT) != 0, local = (prm->flags & BIALIGN_BATCH_LOCAL) != 0;
  const bool overlap = (prm->flags & BIALIGN_BATCH_OVERLAP) != 0;
  b.mode = fit ? AlignMode::Fit : local ? AlignMode::Local : overlap ? AlignMode::Overlap : AlignMode::Global;
  if (b.free_ends() && (prm->flags & (BIALIGN_BATCH_LEAN_TRACE | BIALIGN_BATCH_LEVEL_TRACE)))
    return fail(BIALIGN_E_UNSUPPORTED, "%s exists in full storage and in SCORE_ONLY: not with LEAN_TRACE or LEVEL_TRACE", b.mode_name());
  if (b.free_ends() && b.wide)
    return fail(BIALIGN_E_UNSUPPORTED, "%s exists for max_shift <= %d only (the tiled sweeps)", b.mode_name(), BIALIGN_MAX_SHIFT_TILED);
  if (fit && local) return fail(BIALIGN_E_INVALID, "LOCAL and FIT exclude each other");
  if (overlap && (fit || local)) return fail(BIALIGN_E_INVALID, "OVERLAP and %s exclude each other", b.mode_name());
  if (b.mode == AlignMode::Local && b.affine && prm->gap_opening_cost > 0)
    return fail(BIALIGN_E_UNSUPPORTED, "LOCAL exists for gap_opening_cost <= 0 only in the affine recurrence (no general-beta sweep)");
  if (prm->flags & BIALIGN_BATCH_LEVEL_TRACE) {
    if (b.lean) return fail(BIALIGN_E_INVALID, "LEVEL_TRACE excludes SCORE_ONLY and LEAN_TRACE");
    if (!b.wide)
      return fail(BIALIGN_E_UNSUPPORTED, "LEVEL_TRACE exists for max_shift > %d only: use LEAN_TRACE for narrower bands",
                  BIALIGN_MAX_SHIFT_TILED);
  }
  // wide bands: score-only batches of the affine recurrence keep just the ring of derived values (bialign_wide.hpp);
  // the memory-lean traceback and the one-layer recurrence's score-only form exist for the tiled sweeps only
  if (b.wide && b.lean && (b.lean_trace || !b.affine))
    return fail(BIALIGN_E_UNSUPPORTED, "LEAN_TRACE, and SCORE_ONLY of the non-affine recurrence, exist for max_shift <= %d only",
                BIALIGN_MAX_SHIFT_TILED);
  if (prm->flags & BIALIGN_BATCH_LEVEL_TRACE) b.lean = b.level_trace = true;  // (no full layers: what `lean` says)
  if (b.dense && !b.feat && !pr->mu2_off) return fail(BIALIGN_E_INVALID, "mu2_dense given without mu2_off");
  if (!b.dense && (!pr->cls_a || !pr->cls_b)) return fail(BIALIGN_E_INVALID, "cls_a / cls_b are NULL (LOOKUP form)");
  if (b.dense1 && !pr->mu1_off) return fail(BIALIGN_E_INVALID, "mu1_dense given without mu1_off");
  if (!b.dense1 && (!pr->seq_a || !pr->seq_b)) return fail(BIALIGN_E_INVALID, "seq_a / seq_b are NULL (LOOKUP form)");
  if (!pr->len_a || !pr->len_b || !pr->off_a || !pr->off_b) return fail(BIALIGN_E_INVALID, "len_a / len_b / off_a / off_b are NULL");
  return BIALIGN_OK;
}

// *colmax: the bound on what one column of an alignment adds to a score, from the largest |mu1| and |mu2| and the costs.
// FEATURE form: every feature finite and >= 0, and |mu2| bounded through the molecules' largest features.
inline int score_bound(const bialign_params* prm, const bialign_scoring* sc, const bialign_pairs* pr, const bialign_features* ft,
                       const NullPlan* nul, const BatchPlan& b, int64_t* colmax) {
  // int32 safety window: finite scores and the drift of "-infinity" cells must
  // stay within 2^28 of where they start (kernels rely on it, see THRESH).
  int64_t amax = 0;
  for (int t = 0; t < sc->k1 * sc->k1; ++t) amax = std::max<int64_t>(amax, std::llabs((long long)sc->s1[t]));
  int64_t bmax = 0;
  for (int t = 0; t < sc->k2 * sc->k2; ++t) bmax = std::max<int64_t>(bmax, std::llabs((long long)sc->s2[t]));
  // (null batch: the real pairs' tables, once each, through their first replicas -- a column permutation leaves a table's
  //  maximum where it is)
  auto dense_max = [&](const int32_t* tab, const int64_t* off) {
    int64_t mx = 0;
    for (int p = 0; p < pr->npairs; p += nul ? nul->replicas : 1) {
      const int64_t cnt = (int64_t)std::max(pr->len_a[p], 0) * std::max(pr->len_b[p], 0);
      for (int64_t t = 0; t < cnt; ++t) mx = std::max<int64_t>(mx, std::llabs((long long)tab[off[p] + t]));
    }
    return mx;
  };
  if (b.dense && !b.feat) bmax = dense_max(pr->mu2_dense, pr->mu2_off);   // dense mu2: the bound comes from the tables themselves
  if (b.feat) {  // FEATURE form: every number finite and >= 0; the bound from the molecules' largest features
    struct MolMax { int32_t len; double up, down, unp; };
    std::unordered_map<int64_t, MolMax> seen[2];  // per side: start offset -> what was checked there (molecules are shared)
    auto check = [&](int side, int p, int64_t off, int32_t len, const double* up, const double* down, const double* unp,
                     const MolMax** res) {
      MolMax& mm = seen[side][off];
      if (mm.len < len) {
        const double* arr[3] = {up, down, unp};
        static const char* const names[3] = {"up", "down", "unp"};
        double mx[3] = {0, 0, 0};
        for (int f = 0; f < 3; ++f)
          for (int32_t r = 0; r < len; ++r) {
            const double x = arr[f][off + r];
            if (!(x >= 0.0) || std::isinf(x))  // (NaN fails the comparison)
              return fail(BIALIGN_E_INVALID, "pair %d: feature %s_%c at position %d is %g: features must be finite and >= 0", p,
                          names[f], side ? 'b' : 'a', r + 1, x);
            mx[f] = std::max(mx[f], x);
          }
        mm = MolMax{len, mx[0], mx[1], mx[2]};
      }
      *res = &mm;
      return BIALIGN_OK;
    };
    bmax = 0;
    // null batch: the real pairs, once each -- a shuffle moves B's numbers and leaves their maxima, so the real pair's
    // bound serves all its replicas (virtual pair p * R is real pair p's first; its B is at the plan's off_b)
    const int nreal = nul ? nul->npairs : pr->npairs;
    for (int p = 0; p < nreal; ++p) {
      const MolMax *ma = nullptr, *mb = nullptr;
      const size_t v = nul ? (size_t)p * nul->replicas : (size_t)p;
      const int64_t off_b = nul ? nul->off_b[p] : pr->off_b[p];
      if (int rc = check(0, p, pr->off_a[v], std::max(pr->len_a[v], 0), ft->up_a, ft->down_a, ft->unp_a, &ma)) return rc;
      if (int rc = check(1, p, off_b, std::max(pr->len_b[v], 0), ft->up_b, ft->down_b, ft->unp_b, &mb)) return rc;
      const double bound = std::fabs((double)ft->structure_weight) *
                           (std::sqrt(ma->up * mb->up) + std::sqrt(ma->down * mb->down) + std::sqrt(ma->unp * mb->unp));
      if (!(bound < 1073741824.0))  // 2^30: outside any window, and an int64 could not hold much more
        return fail(BIALIGN_E_RANGE, "pair %d: structure scores may leave the int32 safety window (bound %g)", p, bound);
      bmax = std::max<int64_t>(bmax, (int64_t)std::ceil(bound));
    }
  }
  if (b.dense1) amax = dense_max(pr->mu1_dense, pr->mu1_off);  // ... and so for dense mu1
  *colmax = amax + bmax + 2 * (std::llabs((long long)prm->gap_cost) + std::llabs((long long)prm->gap_opening_cost)) +
            2 * std::llabs((long long)prm->shift_cost);
  return BIALIGN_OK;
}

// Per pair: the window check, a null batch's sum-of-squares check, sweep geometry, trace and table offsets, LDS needs.
inline int plan_pairs(const bialign_pairs* pr, const NullPlan* nul, int64_t colmax, BatchPlan& b) {
  const int S = b.S;
  const SweepInfo& geo = sweep_info(b);
  const LdsForm form{b.dense, false, b.dense1}, diet{false, true, false};
  const auto shown = [&](int p) { return nul ? p / nul->replicas : p; };  // the pair an error message names: the real one
  b.pairs.resize(pr->npairs);
  b.pair_dwords.resize(pr->npairs);
  for (int p = 0; p < pr->npairs; ++p) {
    const int n = pr->len_a[p], m = pr->len_b[p];
    if (n < 1 || m < 1)  // the reference raises IndexError on empty molecules (pyx:407)
      return fail(BIALIGN_E_INVALID, "pair %d: empty molecule (n=%d, m=%d)", shown(p), n, m);
    if ((2 * ((int64_t)n + m) + 8) * colmax >= (1 << 28))
      return fail(BIALIGN_E_RANGE, "pair %d: scores may leave the int32 safety window (n+m=%d, column bound %lld)", shown(p),
                  n + m, (long long)colmax);
    // the end's position in the pair's key is 32 bits (bialign_free_ends.hpp); an overlap batch is held to the bound in full
    // storage too, so that what the mode accepts does not depend on the storage
    if ((b.end_key() || b.mode == AlignMode::Overlap) && n + m >= END_KEY_MAX_NM)
      return fail(BIALIGN_E_UNSUPPORTED, "pair %d: %s takes n + m < %d (n+m=%d)", shown(p), b.mode_name(), END_KEY_MAX_NM, n + m);
    if (nul) {  // the reduction's int64 sum of squares: replicas * bound^2 with the window's bound on |score| (< 2^28)
      const int64_t bound = (2 * ((int64_t)n + m) + 8) * colmax;
      if (bound > 0 && bound * bound > INT64_MAX / nul->replicas)
        return fail(BIALIGN_E_RANGE, "pair %d: %d replica scores of magnitude up to %lld could overflow the int64 sum of squares",
                    shown(p), nul->replicas, (long long)bound);
    }
    PairDesc& d = b.pairs[p];
    d.n = n;
    d.m = m;
    d.NS = d.P = d.G = 0;
    if (!b.wide) sweep_geometry(geo, n, m, &d.NS, &d.P, &d.G);
    d.trace_cap = 2 * (n + m) + 2;
    if (const char* e = getenv("BIALIGN_TRACE_CAP")) d.trace_cap = std::min(d.trace_cap, std::max(1, atoi(e)));  // tests: the clip
    d.seq_a = pr->off_a[p];
    d.seq_b = pr->off_b[p];
    d.trace_off = b.trace_bytes;
    d.tab_off = b.tot_tab;  // dense forms: the pair's tables, end to end (mu2's, then mu1's); FEATURE form: plan_chunks
    b.tot_tab += (int64_t)n * m * ((b.dense ? 1 : 0) + (b.dense1 ? 1 : 0));
    if (b.feat) b.tab_dwords.push_back((int64_t)n * m * (b.dense1 ? 2 : 1));
    if (b.null_dense) b.tab_dwords.push_back((int64_t)n * m * ((b.dense ? 1 : 0) + (b.dense1 ? 1 : 0)));
    b.trace_bytes += d.trace_cap;
    b.cells += cells_of(n, m, S);
    b.tot_a = std::max<int64_t>(b.tot_a, pr->off_a[p] + n);
    b.tot_b = std::max<int64_t>(b.tot_b, pr->off_b[p] + m);
    if (!b.wide) {
      b.lds_bytes = std::max(b.lds_bytes, lds_need(geo, 1, b.k1, b.k2, n, m, form));
      b.lds_base = std::max(b.lds_base, lds_need(geo, 0, b.k1, b.k2, n, m, form));
      b.lds_diet8 = std::max(b.lds_diet8, lds_need(geo, 8, b.k1, b.k2, n, m, diet));
      b.lds_slim_codes = std::max(b.lds_slim_codes, lds_need_slim_codes(geo, n, m));
    }
    b.lds_trace = std::max<size_t>(b.lds_trace, ((size_t)b.k1 * b.k1 + (size_t)b.k2 * b.k2) * 4 +
                                                      (b.dense1 ? 1 : 2) * ((size_t)code_pad(n) + (size_t)code_pad(m)));
  }
  if (!b.wide)
    b.lds_per_wave = lds_need(geo, 1, b.k1, b.k2, 1, 1, form) - lds_need(geo, 0, b.k1, b.k2, 1, 1, form);
  if (!b.wide) b.lds_slim_base = lds_need_slim_base(geo, b.k1, b.k2);
  if (std::max(b.lds_bytes, b.lds_trace) > 160 * 1024)
    return fail(BIALIGN_E_UNSUPPORTED, "molecules too long for the LDS staging (%zu bytes needed, 160 KiB per workgroup)",
                std::max(b.lds_bytes, b.lds_trace));
  return BIALIGN_OK;
}

// Packed records (Pack<S>): for sweeps whose steps are mostly interior
inline void decide_pack(BatchPlan& b, int64_t colmax) {
  const int S = b.S;
  const SweepInfo& pki = sweep_info(b);
  const char* e = getenv("BIALIGN_PACK");  // "0" never, "1" wherever the layout allows (tests), unset: when it pays
  const bool force = e && e[0] == '1';
  bool ok = b.affine && S >= 1 && S <= BIALIGN_MAX_SHIFT_PACKED && !b.lean && !b.dense1 && !b.own_sweeps() && b.prm.gap_opening_cost <= 0 &&
            !(e && e[0] == '0') &&
            (force || colmax < 8192) &&  // offsets span a few column scores (measured: up to 2.5): beyond this they will not fit
            // s=3 runs one wave per SIMD and is bound by issue: packing pays where the device is full (512 pairs x len 512
            // +7 %, 86 pairs in cross-CU teams of 11 +25 %), not for a few long pairs (21 x len 1024: -14 %, 8 x len 2048: -15 %)
            (force || S < 3 || b.npairs >= 64);
  for (int p = 0; ok && p < b.npairs; ++p) {
    const PairDesc& d = b.pairs[p];
    const int interior = d.m - S - pki.pack_lo + 1;  // phases LO .. m - S per strip
    const int64_t packed_dw = pki.pack_written_dwords(d.G, d.P, d.m);
    const int64_t full_dw = (int64_t)d.G * pki.pack_full_recdw;
    // unless forced (tests): only where it saves a fifth of the bytes written (long enough columns, more than a strip or two)
    ok = interior >= 1 && (force || packed_dw * 5 <= full_dw * 4);
  }
  b.pack = ok;
}

// What the largest pair needs inside the budget: its layers, where tables are per-chunk scratch its tables, and the
// wide-band affine sweep's ring
inline int64_t max_pair_need(const BatchPlan& b) {
  int64_t mx = 0;
  for (int p = 0; p < b.npairs; ++p)
    mx = std::max(mx, b.pair_dwords[p] + (b.tab_scratch() ? b.tab_dwords[p] : 0) + (b.ring_dwords.empty() ? 0 : b.ring_dwords[p]));
  return mx;
}

// The HBM budget in dwords: the caller's, or 85 % of what is free; never more than 95 % of it.
inline int64_t budget_dwords(int64_t hbm_budget, size_t free_bytes) {
  const int64_t budget = hbm_budget > 0 ? hbm_budget : (int64_t)(free_bytes * 0.85);
  return std::min<int64_t>(budget, (int64_t)(free_bytes * 0.95)) / 4;
}

// The storage mode the budget allows (full or packed records; LEAN or LEVEL storage for a pair whose full layers exceed
// it), the round sizes of the reduced modes, every pair's size in that mode, and the first chunk plan.
inline int plan_storage(BatchPlan& b, int64_t budget_dw) {
  const int S = b.S;
  const SweepInfo& geo = sweep_info(b);
  std::vector<int64_t>& pair_dwords = b.pair_dwords;
  auto max_need = [&]() { return max_pair_need(b); };
  // layer storage per pair in the batch's mode (dwords); a pair's scratch records follow its LEAN records
  auto size_pairs = [&]() {
    b.ring_dwords.assign(b.ring_scratch() ? b.npairs : 0, 0);  // (the LEVEL forms' ring is part of the pair's region)
    for (int p = 0; p < b.npairs; ++p) {
      PairDesc& d = b.pairs[p];
      if (b.ring_scratch()) b.ring_dwords[p] = WIDE_RING * wide_ring_level_dwords(d.n, S);
      if (b.wide && b.level_trace) {  // checkpoints, one segment's scratch, the ring (bialign_wide.hpp)
        d.scratch_off = wide_ckpt_dwords(d.n, d.m, S, b.wide_seg, b.NL);  // relative to layer_off until the chunk layout is fixed
        pair_dwords[p] = wide_level_pair_dwords(d.n, d.m, S, b.wide_seg, b.NL);
        continue;
      }
      if (b.wide) {  // reference-order layers, every band slot of every (i, j); none at all for a score-only batch
        pair_dwords[p] = b.lean ? 16 : wide_pair_dwords(d.n, d.m, S, b.NL);
        continue;
      }
      const int64_t lean_dw = (int64_t)d.G * geo.lean_recdw;
      const int64_t scratch_dw = (int64_t)(d.m + geo.MAXOFF + 1) * geo.recdw;  // one strip's full records
      d.scratch_off = lean_dw;  // relative to layer_off until the chunk layout is fixed below
      pair_dwords[p] = b.lean_trace ? lean_dw + b.resw_k * scratch_dw : (b.lean ? lean_dw : (int64_t)d.G * geo.recdw);
      if (b.pack && !b.lean)  // (a sweep that meets an unpackable value is repeated with full records: replan_full())
        pair_dwords[p] = geo.pack_pair_dwords(d.G, d.P, d.m);
    }
  };
  // lean traceback: few pairs -> several strips per round (they re-sweep in parallel), as memory allows
  auto pick_resw_k = [&]() {
    // as many strips per round as keep ~2048 waves busy -- re-sweeps of different strips are independent, so a
    // single long pair gets up to 256 at once -- but no more scratch than about a quarter of the pair's full
    // layers (a strip's scratch is 1/NS of them): the mode exists to save memory
    int ns_max = 1;
    for (const PairDesc& d : b.pairs) ns_max = std::max(ns_max, d.NS);
    b.resw_k = (int)std::min<int64_t>(std::min<int64_t>(256, std::max(1, ns_max / 4)), std::max<int64_t>(1, 2048 / b.npairs));
    if (const char* e = getenv("BIALIGN_RESW_K")) b.resw_k = std::min(256, std::max(1, atoi(e)));  // tests
    for (size_pairs(); b.resw_k > 1 && max_need() > budget_dw; size_pairs())
      b.resw_k /= 2;
  };
  // level-checkpointed traceback: the segment length C that makes the largest pair's region smallest -- (C + 5) levels
  // of scratch and 5 per checkpoint, about 5 L / C of them: C ~ sqrt(5 L) -- one C for the whole batch
  auto pick_wide_seg = [&]() {
    int big = 0;
    for (int p = 1; p < b.npairs; ++p)
      if (wide_pair_dwords(b.pairs[p].n, b.pairs[p].m, S, b.NL) > wide_pair_dwords(b.pairs[big].n, b.pairs[big].m, S, b.NL)) big = p;
    const int n = b.pairs[big].n, m = b.pairs[big].m, L = 2 * (n + m);
    int64_t best = INT64_MAX;
    for (int C = WIDE_SEG_MIN; C <= std::max(WIDE_SEG_MIN, L); ++C) {
      const int64_t levels = wide_scratch_levels(n, m, C) + (int64_t)WIDE_RING * (wide_segments(n, m, C) - 1);
      if (levels < best) best = levels, b.wide_seg = C;
    }
    if (const char* e = getenv("BIALIGN_WIDE_SEG")) b.wide_seg = std::max(WIDE_SEG_MIN, atoi(e));  // tests
  };
  if (b.lean_trace) pick_resw_k();
  if (b.level_trace) pick_wide_seg();
  size_pairs();
  // A pair whose full layers exceed the budget is served from reduced storage instead of failing
  // (memory-lean traceback, ~1.3x the time).
  if (b.pack) {  // the fallback to full records must be possible within the same budget
    int64_t full_max = 0;
    for (int p = 0; p < b.npairs; ++p)
      full_max = std::max(full_max, (int64_t)b.pairs[p].G * geo.pack_full_recdw + (b.feat ? b.tab_dwords[p] : 0));
    if (std::max(full_max, max_need()) > budget_dw) {
      b.pack = false;
      size_pairs();
    }
  }
  if (!b.lean && !b.wide && max_need() > budget_dw) {
    if (b.free_ends())  // no silent change of mode: the memory-lean traceback has no FIT or LOCAL form
      return fail(BIALIGN_E_NOMEM, "a pair needs %lld bytes of layers, budget is %lld: a %s batch does not fall back to LEAN_TRACE",
                  (long long)max_need() * 4, (long long)budget_dw * 4, b.mode_name());
    b.lean = b.lean_trace = true;
    b.pack = false;
    pick_resw_k();
  }
  if (!b.lean && b.wide && max_need() > budget_dw) {  // ... wide bands: from checkpointed levels (bialign_wide.hpp)
    b.lean = b.level_trace = true;
    pick_wide_seg();
    size_pairs();
  }
  b.full_dwords.resize(b.npairs);
  for (int p = 0; p < b.npairs; ++p) b.full_dwords[p] = b.wide ? pair_dwords[p] : (int64_t)b.pairs[p].G * geo.recdw;
  b.packed_sizing = b.pack && !b.lean;
  return plan_chunks(b, pair_dwords, budget_dw);
}

// The allocation retry's re-plan under a smaller budget: offsets back to pair-relative, as before the first plan.
inline int replan_smaller(BatchPlan& b, int64_t budget_dw) {
  for (PairDesc& d : b.pairs) {
    if (b.ring_dwords.empty()) d.scratch_off -= d.layer_off;  // (a ring offset is not relative to the layers: plan_chunks sets it anew)
    d.layer_off = 0;
  }
  return plan_chunks(b, b.pair_dwords, budget_dw);
}

// The virtual pairs of a null batch, pair-major: v = p * R + r is real pair p against replica r, whose codes (and, in
// FEATURE form, features) start at R * (sum of len_b before p) + r * len_b[p] of the replica buffers.
inline int expand_null_pairs(const bialign_params* prm, const bialign_pairs* pr, const bialign_features* ft, int R, uint32_t seed,
                             bool dense, NullPlan& plan) {
  const size_t nv = (size_t)pr->npairs * R;
  plan.replicas = R, plan.seed = seed, plan.npairs = pr->npairs;
  plan.off_b = pr->off_b, plan.seq_b = pr->seq_b, plan.cls_b = ft ? nullptr : pr->cls_b;
  plan.tot_b = 0, plan.max_m = 0, plan.dense = dense;
  std::vector<int32_t>&len_a = plan.len_a, &len_b = plan.len_b;  // (the arrays vp points into)
  std::vector<int64_t>&off_a = plan.off_a, &off_b = plan.v_off_b, &mu1_off = plan.mu1_off, &mu2_off = plan.mu2_off;
  len_a.resize(nv), len_b.resize(nv), off_a.resize(nv), off_b.resize(nv);
  mu1_off.resize(dense && pr->mu1_dense ? nv : 0), mu2_off.resize(dense && pr->mu2_dense ? nv : 0);  // the real pair's
  int64_t before = 0;
  for (int p = 0; p < pr->npairs; ++p) {
    const int n = pr->len_a[p], m = pr->len_b[p];
    if (n < 1 || m < 1) return fail(BIALIGN_E_INVALID, "pair %d: empty molecule (n=%d, m=%d)", p, n, m);
    if (pr->off_b[p] < 0) return fail(BIALIGN_E_INVALID, "pair %d: negative off_b", p);
    if ((ft || dense) && m > NULL_FEAT_MAX_M)  // the wave shuffles' index array is uint16 (bialign_null.hpp), and so the permutations in HBM
      return fail(BIALIGN_E_UNSUPPORTED, "pair %d: B molecule of %d residues, a %s-form null batch takes up to %d", p, m,
                  ft ? "FEATURE" : "DENSE", NULL_FEAT_MAX_M);
    plan.max_m = std::max(plan.max_m, m);
    for (int r = 0; r < R; ++r) {
      const size_t v = (size_t)p * R + r;
      len_a[v] = n;
      len_b[v] = m;
      off_a[v] = pr->off_a[p];
      off_b[v] = before * R + (int64_t)r * m;
      if (!mu1_off.empty()) mu1_off[v] = pr->mu1_off[p];
      if (!mu2_off.empty()) mu2_off[v] = pr->mu2_off[p];
    }
    before += m;
    plan.tot_b = std::max<int64_t>(plan.tot_b, pr->off_b[p] + m);
  }
  bialign_pairs& vp = plan.vp;
  vp = *pr;
  vp.npairs = (int32_t)nv;
  vp.len_a = len_a.data();
  vp.len_b = len_b.data();
  vp.off_a = off_a.data();
  vp.off_b = off_b.data();
  if (ft) vp.mu2_dense = nullptr, vp.mu2_off = nullptr;  // ignored in FEATURE form
  if (!mu1_off.empty()) vp.mu1_off = mu1_off.data();
  if (!mu2_off.empty()) vp.mu2_off = mu2_off.data();
  plan.vprm = *prm;
  // SCORE_ONLY is forced (the caller refused LEAN_TRACE / LEVEL_TRACE); FIT, LOCAL and OVERLAP pass through -- the replicas are
  // scored in the observed batch's mode -- and so do unknown bits, for check_inputs to refuse
  plan.vprm.flags = BIALIGN_BATCH_SCORE_ONLY | (prm->flags & ~(uint32_t)(BIALIGN_BATCH_LEAN_TRACE | BIALIGN_BATCH_LEVEL_TRACE));
  return BIALIGN_OK;
}

}  // namespace bialign
