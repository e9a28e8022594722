/*
 * bialign.h -- C ABI of libbialign_hip.so, the MI355X (gfx950) engine for the
 * BiAlign hot path: 4-D shift-banded DP fill + traceback.
 *
 * The reference has no FFI; its boundary for this path is the method surface
 * of `cdef class BiAligner` (reference src/bialignment.pyx:155).  Each entry
 * point below names the reference code it replaces.  Everything is plain C:
 * pointers + sizes, no C++/torch types, no exceptions across the boundary.
 * Every function that can fail returns 0 on success and a negative
 * BIALIGN_E_* code otherwise; bialign_last_error() then holds a message for
 * the calling thread.
 *
 * Units of work.  A *pair* is one (A, B) molecule pair, i.e. one BiAligner
 * instance of the reference (src/bialign.py:11).  A *batch* is a set of
 * independent pairs sharing one parameter set; the reference runs a batch of
 * one.  Pairs are given in LOOKUP form:
 *     mu1(i,j) = s1[seq_a[i-1] * k1 + seq_b[j-1]]     (pyx:405-412, 435-436)
 *     mu2(k,l) = s2[cls_a[k-1] * k2 + cls_b[l-1]]     (pyx:414-429, 438-440)
 * with uint8 codes prepared by the host side (bialign_amd/scoring.py),
 * or, either of them or both, in DENSE form: one n x m table per pair
 * (bialign_pairs.mu1_dense / mu2_dense), for scores that depend on position,
 * or, mu2 only, in FEATURE form (bialign_features, bialign_batch_create_features):
 * three doubles per residue from which the GPU builds each pair's table itself.
 * A *null batch* (bialign_null_spec, bialign_batch_create_null) scores every pair against shuffles of its B
 * molecule that the GPU makes itself, for z-scores of the optimal scores; bialign_batch_create_null_features is the
 * same with mu2 in FEATURE form.
 *
 * The engine is GPU only.  There is no CPU fallback behind this ABI.
 */
#ifndef BIALIGN_H
#define BIALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIALIGN_ABI_VERSION 10

#define BIALIGN_OK 0
#define BIALIGN_E_INVALID (-1)     /* bad argument (message says which) */
#define BIALIGN_E_UNSUPPORTED (-2) /* e.g. LEAN_TRACE at max_shift above BIALIGN_MAX_SHIFT_TILED, LEVEL_TRACE at or below it */
#define BIALIGN_E_DEVICE (-3)      /* HIP runtime error */
#define BIALIGN_E_NOMEM (-4)       /* a single pair does not fit the HBM budget */
#define BIALIGN_E_RANGE (-5)       /* scores could leave the int32 safety window */

/* max_shift: any band width the reference takes (pyx:25-35; bialign.py:83 has no upper bound).  Bands up to
 * BIALIGN_MAX_SHIFT_TILED run the tiled register/LDS sweep (the fast path, all storage modes); wider bands
 * run a plain anti-diagonal kernel over layers kept in the reference's own array order (full storage, affine
 * SCORE_ONLY, or -- the reduced mode with full results there -- BIALIGN_BATCH_LEVEL_TRACE).  BIALIGN_MAX_SHIFT merely
 * bounds the index arithmetic. */
#define BIALIGN_MAX_SHIFT_TILED 5
#define BIALIGN_MAX_SHIFT 1024
/* Molecule length: the tiled sweep stages both molecules' codes (2 bytes per residue and molecule) next to
 * its exchange arrays in one workgroup's LDS, the tracebacks stage them next to the score tables: the sum
 * must fit 160 KiB, i.e. n + m below ~60 000 residues at small alphabets (BIALIGN_E_UNSUPPORTED beyond). */
#define BIALIGN_NEG_INF (-(1 << 30)) /* the reference's -infinity, pyx:303,484 */

/* bialign_params.recurrence */
#define BIALIGN_REC_AUTO 0
#define BIALIGN_REC_AFFINE 1
#define BIALIGN_REC_LINEAR 2

/* run flags */
#define BIALIGN_RUN_FILL_ONLY 1u /* optimize() without traceback() */
#define BIALIGN_RUN_ASYNC 2u     /* enqueue and return; bialign_batch_wait (or any result getter) completes the run */

/* bialign_params.flags.  SCORE_ONLY: the batch will only ever be asked for scores (optimize()
 * without a later traceback(), e.g. all-against-all scoring): the sweep keeps just the rows the
 * next strip needs instead of all layers -- 1/20 of the HBM footprint and traffic at max_shift 1 --
 * and bialign_batch_get_traces / bialign_batch_dump_layers fail with BIALIGN_E_INVALID.  Beyond
 * BIALIGN_MAX_SHIFT_TILED: the affine recurrence only (no layers at all are stored there, just a ring of the
 * last five anti-diagonal levels' derived values); BIALIGN_E_UNSUPPORTED for the non-affine one. */
#define BIALIGN_BATCH_SCORE_ONLY 1u
/* LEAN_TRACE: full results (scores and traces) from the same reduced storage: after the lean sweep
 * the traceback re-sweeps strips of lattice rows into a per-pair scratch area -- as many at a time as
 * keep the device busy and the HBM budget allows, at most a quarter of the pair's full layers -- and
 * walks through them.  A twelfth to a third of the HBM footprint of the default mode (hbm_budget_bytes
 * decides) for ~1.1-1.3x the time: for pairs whose layers would not fit otherwise.  max_shift <=
 * BIALIGN_MAX_SHIFT_TILED only (BIALIGN_E_UNSUPPORTED beyond). */
#define BIALIGN_BATCH_LEAN_TRACE 2u
/* LEVEL_TRACE: the same for bands beyond BIALIGN_MAX_SHIFT_TILED: full results (scores and traces) without the
 * pair's layers in HBM.  The anti-diagonal sweep keeps its state in a ring of the last five levels and leaves a
 * checkpoint of five levels every C levels; the traceback then sweeps one segment of C + 4 levels at a time, top
 * segment first, into a per-pair scratch addressed by level and walks through it (a traceback only ever steps 1..4
 * levels down).  Per pair (C + 4 + 5 L / C) levels instead of all L = 2(n+m), C ~ sqrt(5 L) chosen by the engine: a
 * quarter of the default mode's HBM at 300 x 300, a tenth at 3000 x 3000, for about twice the sweep time (every
 * level is swept twice).  Both recurrences, every form of mu1 / mu2.  max_shift > BIALIGN_MAX_SHIFT_TILED only
 * (BIALIGN_E_UNSUPPORTED below: LEAN_TRACE is the mode there); with SCORE_ONLY or LEAN_TRACE: BIALIGN_E_INVALID.
 * bialign_batch_dump_layers fails with BIALIGN_E_INVALID.  The engine takes this mode by itself when a wide-band
 * pair's full layers exceed the HBM budget (bialign_batch_info.storage says so). */
#define BIALIGN_BATCH_LEVEL_TRACE 4u
/* FIT (new in ABI 10 as added symbols: no existing struct or function changes): fit alignments -- molecule A inside a
 * longer molecule B, with free end gaps in B (a domain in a whole protein, a motif in a transcript).  The recurrence,
 * the guards and the band are unchanged.  The mode makes the following changes.
 *   Start.  At every lattice point (0, j, 0, j) with j >= 1, the value that the origin's 0 occupies today becomes
 *     max(recurrence value, 0).  In the affine recurrence that value is state 8, (M,M).  In the one-layer recurrence it
 *     is the cell's one value.  The origin stays 0.  All other states and cells are computed as before.
 *   End.  score = max over j in 0..m of E(j).  In the affine recurrence E(j) is the maximum of the nine states at
 *     (n, j, n, j).  In the one-layer recurrence it is that cell's value.  end_b is the smallest j that attains the maximum.
 *   Walk.  The traceback starts at (n, end_b, n, end_b).  In the affine recurrence it starts in the best state there,
 *     with ties between states broken as today at (n, m, n, m).  It applies the existing tie-breaks, unchanged.  It
 *     stops, complete, the first time it stands on a point (0, j, 0, j) whose stored value is exactly 0.  In the affine
 *     recurrence the walk must also be in state 8.  The walk is checked once on arrival, before it picks a predecessor.
 *     So start_b = j.  The origin satisfies this stop rule as it does today.  The trace describes the global alignment
 *     of A with B[start_b:end_b], in the existing byte code.
 *   Equivalence.  Write `global` for the reference's optimize() score.  For costs that keep the int32 safety window
 *     (unchanged, as the per-column bound is unchanged), the fit score is
 *     max over 0 <= j0 <= j1 <= m of global(A, B[j0:j1]).  The empty substring is included.  Its value is the layer
 *     value at (n, 0, n, 0).
 * Only B's ends are free and A is consumed whole.  A caller who wants the other direction swaps the molecules.
 * Accepted for max_shift <= BIALIGN_MAX_SHIFT_TILED, both recurrences, every form of mu1 and mu2, in full storage and
 * with SCORE_ONLY (so in all three bialign_batch_create_null* entry points, which pass it through: the replicas are
 * scored in the same mode).  With LEAN_TRACE or LEVEL_TRACE, or beyond the tiled band: BIALIGN_E_UNSUPPORTED.  A FIT
 * batch never changes its storage mode by itself: where a pair's full layers exceed the HBM budget the engine's
 * fallback to LEAN_TRACE is BIALIGN_E_NOMEM instead.  bialign_batch_get_scores returns the fit score,
 * bialign_batch_get_traces the walk above (complete keeps its meaning), bialign_batch_dump_layers the FIT layers,
 * bialign_batch_get_fit_spans the spans.  A BIALIGN_RUN_FILL_ONLY run of a full-storage FIT batch leaves the fit scores
 * and end_b (as such a run of any full-storage batch leaves the scores: the traceback kernel's prologue writes them). */
#define BIALIGN_BATCH_FIT 8u
/* LOCAL (new in ABI 10 as added symbols: no existing struct or function changes): local alignments -- the best-scoring
 * parts of A and B, with the ends of both molecules free (two multi-domain proteins that share one domain, a structured
 * motif two long transcripts have in common).  The recurrence, the guards, the band and the tie-breaks are unchanged.
 * The mode makes the following changes.
 *   Start.  At every lattice point (i, j, i, j), 0 <= i <= n, 0 <= j <= m, the value that the origin's 0 occupies today
 *     becomes max(recurrence value, 0).  In the affine recurrence that value is state 8, (M,M).  In the one-layer
 *     recurrence it is the cell's one value.  Every other state and cell is computed as before.
 *   End.  score = max over 0 <= i <= n, 0 <= j <= m of E(i, j).  In the affine recurrence E is the maximum of the nine
 *     states at (i, j, i, j).  In the one-layer recurrence it is the cell's value.  (end_a, end_b) is the smallest i, then
 *     the smallest j, that attains the maximum.  score >= 0 always: the origin gives 0 with the empty alignment.
 *   Walk.  The traceback starts at (end_a, end_b, end_a, end_b).  In the affine recurrence it starts in the best state
 *     there, with ties broken as today at (n, m, n, m).  It applies the existing tie-breaks.  It stops, complete, the
 *     first time it stands on a point (i, j, i, j) whose stored value is exactly 0.  In the affine recurrence it must
 *     also be in state 8.  It is checked once on arrival, before it picks a predecessor.  That point is
 *     (start_a, start_b).  The trace is the global alignment of A[start_a:end_a] with B[start_b:end_b], in the existing
 *     byte code.
 *   Equivalence.  For costs inside the int32 safety window, score = max over i0 <= i1, j0 <= j1 of
 *     global(A[i0:i1], B[j0:j1]).  The per-column bound is unchanged: the floor only raises values towards 0.
 * Accepted for max_shift <= BIALIGN_MAX_SHIFT_TILED, both recurrences, every form of mu1 and mu2, in full storage and
 * with SCORE_ONLY (so in all three bialign_batch_create_null* entry points, which pass it through: the replicas are
 * scored in the same mode), for pairs with n + m < 60000.  With FIT: BIALIGN_E_INVALID.  With LEAN_TRACE or LEVEL_TRACE,
 * beyond the tiled band, or with gap_opening_cost > 0 in the affine recurrence: BIALIGN_E_UNSUPPORTED.  A LOCAL batch
 * never changes its storage mode by itself: where a pair's full layers exceed the HBM budget the engine's fallback to
 * LEAN_TRACE is BIALIGN_E_NOMEM instead.  bialign_batch_get_scores returns the local score,
 * bialign_batch_get_traces the walk above (complete keeps its meaning), bialign_batch_dump_layers the LOCAL layers,
 * bialign_batch_get_local_spans the spans.  Scores and ends are there after every run, SCORE_ONLY and
 * BIALIGN_RUN_FILL_ONLY included; only the one best local hit of a pair is reported. */
#define BIALIGN_BATCH_LOCAL 64u
/* OVERLAP (new in ABI 10 as added symbols: no existing struct or function changes): overlap alignments -- the global
 * alignment whose end gaps cost nothing in either molecule ("ends-free", "semi-global": two fragments whose ends overhang
 * each other, a domain against a protein when it is not known which contains the other).  The recurrence, the guards,
 * the band and the tie-breaks are unchanged.  The mode makes the following changes.
 *   Start.  At every lattice point (0, j, 0, j) with j >= 1, and at every (i, 0, i, 0) with i >= 1, the value that the
 *     origin's 0 occupies today becomes max(recurrence value, 0).  In the affine recurrence that value is state 8.  In
 *     the one-layer recurrence it is the cell's one value.  The origin stays 0.  Every other state and cell is computed
 *     as before.
 *   End.  score = max E over the end cells (i, m, i, m), 0 <= i <= n, and (n, j, n, j), 0 <= j <= m.  E is defined as for
 *     FIT and LOCAL.  (end_a, end_b) is the end cell that attains the maximum with the smallest i, then the smallest j.
 *     This is LOCAL's order, and the order of LOCAL's key.  score >= 0 always: (0, m, 0, m) and (n, 0, n, 0) are floored
 *     starts and ends at once.
 *   Walk.  The walk starts at (end_a, end_b, end_a, end_b).  In the affine recurrence it starts in the best state there,
 *     with ties broken as today at (n, m, n, m).  It applies the existing tie-breaks.  It stops, complete, the first
 *     time it stands on a point (0, j, 0, j) or (i, 0, i, 0) whose stored value is exactly 0.  In the affine recurrence
 *     it must also be in state 8.  It is checked once on arrival, before it picks a predecessor.  That point is
 *     (start_a, start_b).  The trace is the global alignment of A[start_a:end_a] with B[start_b:end_b], in the existing
 *     byte code.
 *   Equivalence.  For costs inside the int32 safety window, score = the maximum of global(A[i0:i1], B[j0:j1]) over the
 *     windows with (i0 = 0 or j0 = 0) and (i1 = n or j1 = m).  The per-column bound is unchanged.
 * Accepted for max_shift <= BIALIGN_MAX_SHIFT_TILED, both recurrences, any sign of gap_opening_cost (as FIT), every form
 * of mu1 and mu2, in full storage and with SCORE_ONLY (so in all three bialign_batch_create_null* entry points, which pass
 * it through), for pairs with n + m < 60000 (the key's position is 32 bits wide).  With FIT or LOCAL: BIALIGN_E_INVALID.
 * With LEAN_TRACE or LEVEL_TRACE, or beyond the tiled band: BIALIGN_E_UNSUPPORTED.  There is no silent fallback to
 * LEAN_TRACE: it is BIALIGN_E_NOMEM instead.  bialign_batch_get_scores returns the overlap score,
 * bialign_batch_get_traces the walk above (complete keeps its meaning), bialign_batch_dump_layers the OVERLAP layers,
 * bialign_batch_get_overlap_spans the spans.  Scores and ends are there after every run, SCORE_ONLY and
 * BIALIGN_RUN_FILL_ONLY included. */
#define BIALIGN_BATCH_OVERLAP 128u
/* Bits of bialign_params.flags beyond the ones above: BIALIGN_E_INVALID. */

typedef struct bialign_engine bialign_engine; /* one per (process, device) */
typedef struct bialign_batch bialign_batch;   /* inputs resident in HBM */

/* BiAligner parameters that reach the DP (pyx:186-188, 230, 259). */
typedef struct bialign_params {
  int32_t gap_opening_cost; /* beta; != 0 selects the affine recurrence (pyx:204-205, 444) */
  int32_t gap_cost;         /* gamma */
  int32_t shift_cost;       /* Delta */
  int32_t max_shift;        /* s >= 0 (see BIALIGN_MAX_SHIFT_TILED) */
  int32_t recurrence;       /* BIALIGN_REC_AUTO: affine iff gap_opening_cost != 0, as optimize()
                               dispatches (pyx:444); BIALIGN_REC_AFFINE = affine_optimize() called
                               directly (pyx:474); BIALIGN_REC_LINEAR = the 13-case recurrence */
  uint32_t flags;           /* BIALIGN_BATCH_* */
} bialign_params;

/* Score tables, row-major, values already scaled (nonpyx:33: x100). */
typedef struct bialign_scoring {
  int32_t k1;        /* sequence alphabet size, 1..256 (1 with a one-entry s1 when mu1 is DENSE) */
  const int32_t* s1; /* k1*k1, unused when mu1 is DENSE */
  int32_t k2;        /* structure class count, 1..256 */
  const int32_t* s2; /* k2*k2 */
} bialign_scoring;

/* Host-side description of the pairs; copied to HBM by bialign_batch_create. */
typedef struct bialign_pairs {
  int32_t npairs;
  const int32_t* len_a; /* [npairs] n >= 1 */
  const int32_t* len_b; /* [npairs] m >= 1 */
  const int64_t* off_a; /* [npairs] start of pair p in seq_a / cls_a */
  const int64_t* off_b; /* [npairs] start of pair p in seq_b / cls_b */
  const uint8_t* seq_a; /* sequence codes of all A molecules, concatenated */
  const uint8_t* cls_a; /* structure classes, same indexing as seq_a */
  const uint8_t* seq_b;
  const uint8_t* cls_b;
  /* Optional DENSE form of mu2 (NULL = LOOKUP form above): for structure similarities that are
   * not a small class table -- the reference's RNA mode with *predicted* structures, where
   * mu2(k,l) = int(sw*(sqrt(upA upB)+sqrt(dnA dnB)+sqrt(unpA unpB))) of real-valued features
   * (pyx:416-423).  Pair p's table is mu2_dense[mu2_off[p] + (k-1)*m + (l-1)], k=1..n, l=1..m;
   * cls_a / cls_b are then ignored (may be NULL). */
  const int32_t* mu2_dense;
  const int64_t* mu2_off;
  /* Optional DENSE form of mu1 (NULL = LOOKUP form, ABI 10): position-specific sequence scores --
   * a profile / PSSM of one molecule, scores derived from embeddings, per-position weights.  Pair
   * p's table is mu1_dense[mu1_off[p] + (i-1)*m + (j-1)], i=1..n, j=1..m, values in the scale of
   * s1 (x100); seq_a / seq_b and s1 are then ignored (seq_a / seq_b may be NULL, k1 may be 1).
   * Works in every mode, alone or with dense mu2; mu1_dense without mu1_off is BIALIGN_E_INVALID,
   * and tables whose magnitude could leave the int32 safety window are BIALIGN_E_RANGE. */
  const int32_t* mu1_dense;
  const int64_t* mu1_off;
} bialign_pairs;

/* mu2 in FEATURE form: the reference's RNA mode with predicted structures (pyx:416-423),
 *     mu2(k,l) = int(sw * (sqrt(upA[k] upB[l]) + sqrt(dnA[k] dnB[l]) + sqrt(unpA[k] unpB[l])))
 * from three real numbers per residue.  Residue r (0-based) of pair p's A molecule is at [off_a[p] + r] of up_a /
 * down_a / unp_a, of its B molecule at [off_b[p] + r] of up_b / down_b / unp_b (off_a / off_b of bialign_pairs, as
 * for the code arrays): pairs may share molecules, an all-against-all batch uploads every molecule's numbers once.
 * The upload is O(sum of lengths); the GPU builds the int32 tables of a chunk just before it sweeps the chunk, with
 * the reference's IEEE double operations in the reference's order (the result equals the DENSE form's bit for bit),
 * into a scratch buffer that is part of the HBM chunk plan (hbm_budget_bytes).
 * Every feature must be finite and >= 0.  (The reference raises "math domain error" from math.sqrt only when a
 * PRODUCT is negative, so two negative numbers pass there; this ABI is stricter and refuses the sign outright.) */
typedef struct bialign_features {
  int32_t structure_weight;            /* sw, an int as in bialign.py */
  const double *up_a, *down_a, *unp_a; /* residue r (0-based) of pair p's A molecule at [off_a[p] + r] */
  const double *up_b, *down_b, *unp_b; /* ... B molecule at [off_b[p] + r] */
} bialign_features;

/* bialign_feature_info.form */
#define BIALIGN_MU2_LOOKUP 0
#define BIALIGN_MU2_DENSE 1
#define BIALIGN_MU2_FEATURE 2

typedef struct bialign_feature_info {
  int32_t form;           /* BIALIGN_MU2_* of this batch */
  int32_t build_launches; /* table-builder launches of the last run (FEATURE form: one per chunk; else 0) */
  int64_t table_bytes;    /* FEATURE: mu2 table bytes of the largest chunk (the scratch buffer's use, inside the HBM
                             budget); DENSE: bytes of all resident tables; LOOKUP: 0 */
  double build_ms;        /* HIP-event time of the builder launches of the last run; not part of fill_ms */
  /* A DENSE-form null batch (bialign_batch_create_null_dense): form is DENSE when mu2 is dense, else LOOKUP;
     build_launches counts the launches of the kernel that permutes the tables' columns, one per chunk, build_ms is their
     time; table_bytes is the largest chunk's scratch, the replicas' permuted tables of every dense form. */
} bialign_feature_info;

/* ---- Shuffled-null significance (new in ABI 10 as added symbols: no existing struct or function changes).
 * A raw bi-alignment score grows with both lengths and with composition; where it lies among the scores of A against
 * R random shuffles of B is comparable between pairs.  A null batch runs those npairs * R alignments as one SCORE_ONLY
 * batch: B is uploaded once, the GPU writes the R shuffled copies of every pair's B itself and reduces every pair's R
 * scores to exact integers (bialign_null_stats); z = (score - mean) / sd is formed by the caller from those.
 *
 * THE PERMUTATION (normative; all arithmetic uint32 unless said otherwise):
 *     mix(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *     h(seed, p, r) = mix(mix(mix(seed ^ 0x9E3779B9) + p) + r)       p = pair index in the batch, r = replica
 *     draw(t)       = (uint64(mix(h + t)) * (t + 1)) >> 32           in [0, t]
 *     perm = identity on 0..m-1;  for t = m-1 down to 1: swap(perm[t], perm[draw(t)])
 *     replica r of pair p's B:  seq'[x] = seq_b[perm[x]],  cls'[x] = cls_b[perm[x]]
 * (a residue's letter and its structure class move together).  A is never shuffled; m = 1 gives the identity.  The
 * result depends on (seed, p, r, m) only -- not on chunking, team size, launch order or device; pairs that share a B
 * molecule through off_b get different shuffles because p differs.  bialign_amd/significance.py restates it in Python.
 *
 * bialign_batch_create_null takes the LOOKUP form only: with mu1_dense or mu2_dense set it fails with
 * BIALIGN_E_UNSUPPORTED (a table's columns would have to be permuted per replica: bialign_batch_create_null_dense does).
 * FEATURE form of mu2 (RNA with real-valued structure features, bialign_features): bialign_batch_create_null_features.
 * Replica r of pair p's B then has, with the same perm,
 *     seq'[x] = seq_b[perm[x]],  up'[x] = up_b[perm[x]],  down'[x] = down_b[perm[x]],  unp'[x] = unp_b[perm[x]]
 * -- a residue's letter and its three numbers move together, and the doubles are moved, never recomputed: each is bit
 * for bit the source's.  This is the same null model as the LOOKUP RNA null, in which a position's structure annotation
 * (there its class, here its three numbers) travels with its letter.
 *
 * DENSE form of mu1 and / or mu2 (a PSSM or profile as mu1_dense, structure scores computed outside as mu2_dense):
 * bialign_batch_create_null_dense.  A residue of B carries everything indexed by it -- here a column of each table.
 * Replica r of pair p uses THE PERMUTATION above, unchanged: perm depends on (seed, p, r, m) only and is the same perm
 * the LOOKUP and FEATURE nulls use for the same (seed, p, r, m).  With it
 *     mu1'[(i-1)*m + x] = mu1[(i-1)*m + perm[x]]      (dense mu1)
 *     mu2'[(k-1)*m + x] = mu2[(k-1)*m + perm[x]]      (dense mu2)
 *     seq'[x] = seq_b[perm[x]],  cls'[x] = cls_b[perm[x]]   (whichever of mu1 / mu2 is in LOOKUP form)
 * Values are moved, never recomputed.  A is never shuffled; m = 1 gives the identity.
 *
 * THE DINUCLEOTIDE PERMUTATION (normative; the second null model, bialign_batch_set_null_model).  THE PERMUTATION keeps
 * B's single-letter composition and nothing else; neighbouring letters of nucleic acids are correlated, and a null that
 * destroys that inflates z-scores (Altschul & Erickson 1985, Workman & Krogh 1999).  This one keeps the count of every
 * ordered pair of neighbouring letters exactly.  Same mix and h(seed, p, r); the draw is
 *     uni(salt, bound) = (uint64(mix(h + salt)) * bound) >> 32       in [0, bound);  h + salt mod 2^32
 * Letters: B's sequence codes (seq_b), renumbered 0, 1, 2, ... in order of first occurrence in B -- so perm depends on
 * (seed, p, r) and B's letter pattern only, not on the score model's code order, and the host can restate it from the plain
 * string.  A position's structure class, its three feature numbers and its table columns are no part of the letter: they
 * travel with the position, as above.  m <= 2: perm is the identity.  Otherwise
 *  1. Edges.  Edge e, 0 <= e <= m-2, runs from position e to e+1: tail a(e) = B[e], head b(e) = B[e+1].  cnt[x] = edges
 *     with tail x, off[x] = sum of cnt[y] over y < x, L = the edges sorted by (tail, e): letter x owns
 *     L[off[x] .. off[x]+cnt[x]), in increasing e.  z = B[m-1].
 *  2. Last exits (Wilson's algorithm, capped).  tree = {z}, s = 0.  For the letters x ascending, skipping those with
 *     cnt[x] = 0 or in the tree:  u = x;  while u is not in the tree: { if s = CAP give up;  last[u] = uni(0x80000000 + s,
 *     cnt[u]);  s += 1;  u = b(L[off[u] + last[u]]) };  then walk again from x along last[] and add every letter met to
 *     the tree, until the tree is reached.  (L is still the sorted list here.)  CAP = 4096 draws per replica.  On giving
 *     up all choices so far are dropped and last[x] = cnt[x]-1 for every x != z with cnt[x] > 0: the original molecule's
 *     own last exits, which always form a tree.
 *  3. Order of exits.  For the letters x ascending with cnt[x] > 0:  if x != z, element last[x] is taken out of x's list
 *     (the others keep their order) and put at the list's end, and r = cnt[x]-1;  if x = z, r = cnt[x].  Then for
 *     t = r-1 down to 1: swap(L[off[x] + t], L[off[x] + uni(off[x] + t, t+1)]).
 *  4. Walk.  perm[0] = 0, cur = B[0], all ptr[] = 0.  For pos = 1 .. m-1:  e = L[off[cur] + ptr[cur]];  ptr[cur] += 1;
 *     perm[pos] = e+1;  cur = b(e).
 * Replica r of pair p is seq'[x] = seq_b[perm[x]], and classes, features and table columns go through the same perm.
 * Guarantees: perm is a permutation with perm[0] = 0; the replica has exactly B's count of every ordered letter pair, hence
 * B's count of every letter and B's first and last letter.  Without the cap every such sequence is equally likely
 * (Altschul-Erickson, BEST theorem); the capped fallback is valid but not uniform.  (Over 2460 random molecules --
 * alphabets of 1, 2, 4 and 20 letters, lengths 1 to 2000, a skewed composition per length -- the largest s was 181: the
 * fallback was never taken.)  The cap is there so that no loop on the device is unbounded.
 * Which letter carries the property: LOOKUP and FEATURE form, and DENSE form with mu1 in LOOKUP form, the sequence code;
 * a dense mu1 has no letters, and the model is refused.  The kernel keeps the edge list and perm (uint16 each), the
 * renumbered letters (uint8) and 3584 bytes of per-letter arrays in one workgroup's 160 KiB of LDS: 5 * len_b + 3584 bytes,
 * so len_b <= BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN. */
#define BIALIGN_NULL_MONO 0
#define BIALIGN_NULL_DINUCLEOTIDE 1
#define BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN 32050
typedef struct bialign_null_spec {
  int32_t replicas; /* R, 1..65535 */
  uint32_t seed;
} bialign_null_spec;

/* Pair p's R replica scores, reduced on the GPU in integer arithmetic (bit for bit reproducible):
 * mean = sum / R, sample variance = (sumsq - sum * sum / R) / (R - 1). */
typedef struct bialign_null_stats {
  int64_t sum, sumsq; /* of the replica scores and of their squares */
  int32_t min, max;
  int32_t n_ge;       /* replicas with score >= the observed score (0 when none was given) */
  int32_t replicas;
} bialign_null_stats;

typedef struct bialign_null_info {
  double shuffle_ms;     /* HIP-event time of the shuffle kernel of the last run; not part of fill_ms */
  double stats_ms;       /* ... of the last bialign_batch_get_null_stats reduction */
  int64_t replica_bytes; /* the replicas' B codes in HBM, both kinds: 2 * R * (sum of len_b); outside hbm_budget_bytes.
                            A FEATURE-form null batch adds the replicas' three planes of doubles: what was allocated
                            is codes plus planes, 26 * R * (sum of len_b).  A DENSE-form null batch adds the replicas'
                            permutations, 16 bits per residue: codes plus index arrays, 4 * R * (sum of len_b) */
} bialign_null_info;

typedef struct bialign_batch_info {
  int32_t npairs;
  int32_t nchunks;        /* HBM-budgeted chunks the batch is processed in */
  int32_t affine;         /* 1 = nine-layer affine recurrence, 0 = one layer */
  int32_t max_shift;
  int64_t cells;          /* in-band lattice points of all pairs (the unit of the metric) */
  int64_t layer_bytes;    /* algorithmic bytes: 36 B (affine) or 4 B per cell */
  int64_t hbm_layer_bytes;/* allocated size of the largest chunk's layer buffer */
  int64_t trace_bytes;    /* capacity of the trace buffer, sum of 2(n+m)+2 */
  int32_t storage;        /* 0 = all layers, BIALIGN_BATCH_SCORE_ONLY, or BIALIGN_BATCH_LEAN_TRACE / BIALIGN_BATCH_LEVEL_TRACE
                             (asked for, or chosen by the engine because a pair's full layers exceed the HBM budget) */
  int32_t reserved;
} bialign_batch_info;

typedef struct bialign_timing {
  double fill_ms;      /* HIP-event time of the fill kernels of the last run */
  double traceback_ms; /* ... of the traceback (or score-only) kernels */
  int32_t fill_launches;
  int32_t traceback_launches;
  int32_t waves_per_pair; /* team size of the last fill launch (team sweep) */
  int32_t cross_cu;       /* 1 if that team was spread over one-wave workgroups */
  int32_t recovered_runs; /* runs of this batch repeated with in-workgroup teams after a cross-CU team lost
                             co-residency (another tenant on the device); the results are those of the repeat */
  int32_t packed_records; /* 1 if the last run's sweeps stored packed layer records (affine, max_shift 1 or 2: base +
                             16-bit offsets in interior steps, decoded by the tracebacks; chosen by the engine, exact) */
} bialign_timing;

int bialign_abi_version(void);
/* 0 for a product build.  Non-zero: the library was compiled as a kernel TIMING experiment (-DBIALIGN_EXP=n,
   tools/exp_build.sh: sweeps without stores, without hand-off waits, ...) whose results are wrong by
   construction; a binding must refuse such a library (bialign_amd/_lib.py does).  Replaces nothing in the
   reference. */
int bialign_build_experiment(void);
/* Number of visible HIP devices (<0 on error). */
int bialign_device_count(void);
const char* bialign_last_error(void);

/* Replaces nothing in the reference (it has no device); one engine plays the
 * role of the Python process that owns a BiAligner. */
/* Engine: device selection + one HIP stream + event pool + the layer buffer of the last batch
 * (kept for the next one: allocating tens of GB costs far more than sweeping them).  An engine
 * and its batches are used from one thread at a time. */
int bialign_engine_create(int device, bialign_engine** out);
/* Safe in any order with bialign_batch_destroy: an engine with live batches goes when its last batch goes. */
void bialign_engine_destroy(bialign_engine* eng);
/* Give the cached layer buffer back to the device (e.g. before another library needs the HBM). */
int bialign_engine_trim(bialign_engine* eng);
/* Pre-allocate the cached layer buffer (bytes) and choose WHERE it lies: on MI355X the physical
 * region a large allocation lands in decides 10-20 % of the sweep's store rate, and a plain
 * streaming write over the buffer predicts it (profiles/r01e_placement).  Up to `tries` candidate
 * allocations are probed (two memset passes each); the fastest is kept for all later batches of
 * this engine.  For long-running users: costs `tries` large allocations once.  Needs twice the
 * buffer in free HBM while it runs, otherwise it just allocates.  *rate_gbps (may be NULL)
 * receives the kept buffer's probe rate. */
int bialign_engine_reserve(bialign_engine* eng, int64_t bytes, int tries, double* rate_gbps);

/* Upload a batch and allocate its DP storage: BiAligner.__init__ (pyx:179-197)
 * for the part that reaches the DP, plus AffineDPMatrices / SparseMatrix4D
 * allocation (pyx:478, 452).  hbm_budget_bytes = 0 lets the engine use ~85 %
 * of the free device memory; a smaller budget forces more chunks. */
int bialign_batch_create(bialign_engine* eng, const bialign_params* params,
                         const bialign_scoring* scoring, const bialign_pairs* pairs,
                         int64_t hbm_budget_bytes, bialign_batch** out);
/* As bialign_batch_create, with mu2 in FEATURE form (new in ABI 10 as added symbols: no existing struct or function
 * changes).  pairs->cls_a / cls_b / mu2_dense / mu2_off are ignored (may be NULL); mu1 is whatever `pairs` says, LOOKUP
 * or dense.  (A dense mu1 stays resident as in bialign_batch_create; a chunk's tables are copied behind its mu2 tables
 * and count in the chunk plan too.)  feat or any of its arrays NULL, a NaN, infinite or negative feature:
 * BIALIGN_E_INVALID (the message names pair and position).  A pair whose bound
 * |sw| * (sqrt(max upA max upB) + sqrt(max dnA max dnB) + sqrt(max unpA max unpB)), rounded up, could leave the int32
 * safety window: BIALIGN_E_RANGE.  A single pair whose table and layers exceed the budget: BIALIGN_E_NOMEM. */
int bialign_batch_create_features(bialign_engine* eng, const bialign_params* params,
                                  const bialign_scoring* scoring, const bialign_pairs* pairs,
                                  const bialign_features* feat, int64_t hbm_budget_bytes, bialign_batch** out);
void bialign_batch_destroy(bialign_batch* b);
int bialign_batch_get_feature_info(const bialign_batch* b, bialign_feature_info* info);
int bialign_batch_get_info(const bialign_batch* b, bialign_batch_info* info);

/* BiAligner.optimize() (pyx:443-509) followed -- unless BIALIGN_RUN_FILL_ONLY --
 * by BiAligner.traceback() (pyx:513-586), for every pair, chunk by chunk.
 * Returns after the device work has completed. */
int bialign_batch_run(bialign_batch* b, uint32_t flags);
/* Completes a BIALIGN_RUN_ASYNC run: waits for the batch's kernels, collects kernel times and the
 * device error flag.  A no-op when nothing is pending.  Lets the host prepare the next batch
 * (encoding, bialign_batch_create: uploads go through their own stream) while this one sweeps. */
int bialign_batch_wait(bialign_batch* b);
int bialign_batch_get_timing(const bialign_batch* b, bialign_timing* t);

/* Optimal scores: the return value of optimize() (pyx:471, 509). */
int bialign_batch_get_scores(const bialign_batch* b, int32_t* scores /* [npairs] */);

/* Traces: the return value of traceback() (pyx:531, 586).  Pair p's columns are
 * trace[trace_off[p] .. trace_off[p] + trace_len[p]), start -> end, one byte per
 * column = o0*8 + o1*4 + o2*2 + o3.  complete[p] == 0 is the condition under
 * which the reference prints "WARNING: incomplete traceback" (pyx:584-585);
 * it is always 1 for the non-affine recurrence.  trace must hold
 * bialign_batch_info.trace_bytes bytes. */
int bialign_batch_get_traces(const bialign_batch* b, uint8_t* trace, int64_t* trace_off,
                             int32_t* trace_len, int32_t* complete);

/* Fit alignments (BIALIGN_BATCH_FIT, new in ABI 10 as an added symbol): pair p's alignment is that of A with B[start_b[p]:end_b[p]] (0-based,
 * half open).  Both arrays are [npairs].  A batch created without FIT, or a null batch (it has no observed alignments):
 * BIALIGN_E_INVALID.  After a SCORE_ONLY or
 * BIALIGN_RUN_FILL_ONLY run end_b is valid and start_b[p] = -1 (so it is for a pair whose traceback is incomplete). */
int bialign_batch_get_fit_spans(const bialign_batch* b, int32_t* start_b, int32_t* end_b);

/* Local alignments (BIALIGN_BATCH_LOCAL, new in ABI 10 as an added symbol): pair p's alignment is that of
 * A[start_a[p]:end_a[p]] with B[start_b[p]:end_b[p]] (0-based, half open).  All four arrays are [npairs].  A batch created
 * without LOCAL (a FIT batch included), or a null batch (it has no observed alignments): BIALIGN_E_INVALID.  After a
 * SCORE_ONLY or BIALIGN_RUN_FILL_ONLY run the ends are valid and start_a[p] = start_b[p] = -1 (so they are for a pair
 * whose traceback is incomplete). */
int bialign_batch_get_local_spans(const bialign_batch* b, int32_t* start_a, int32_t* end_a, int32_t* start_b, int32_t* end_b);

/* Overlap alignments (BIALIGN_BATCH_OVERLAP, new in ABI 10 as an added symbol): the contract of
 * bialign_batch_get_local_spans.  Pair p's alignment is that of A[start_a[p]:end_a[p]] with B[start_b[p]:end_b[p]]
 * (0-based, half open).  The ends are valid after every run; the starts are -1 after a SCORE_ONLY or
 * BIALIGN_RUN_FILL_ONLY run, or for a pair whose traceback is incomplete.  A batch created without OVERLAP, or a null
 * batch: BIALIGN_E_INVALID. */
int bialign_batch_get_overlap_spans(const bialign_batch* b, int32_t* start_a, int32_t* end_a, int32_t* start_b, int32_t* end_b);

/* ---- Hit search (new in ABI 10 as added symbols: no existing struct, function or flag bit changes): every placement of A
 * in B.  A FIT batch reports the one best placement of a pair; a target often carries the query several times (repeated
 * domains, tandem hairpins, several binding sites).  Row n of the FIT layers already holds, for every end j, the score of
 * the best placement that ends there, and FIT's walk already stops at a free start.
 *   The model.  A full-storage FIT batch may be given a hit search (max_hits, max_walks, min_score).  After each chunk's
 *   traceback, while its layers are resident, the search computes per pair:
 *   Profile.  E(j) for j = 0..m, exactly FIT's E.  In the affine recurrence it is the maximum of the nine states at
 *     (n, j, n, j).  In the one-layer recurrence it is the cell's value.
 *   Greedy search.  Every end starts as a candidate.  The search repeats the following.
 *     1. Among unmasked candidates with E(j) >= min_score, take the largest E.  On a tie take the smallest j.  If there is
 *        none, stop with status EXHAUSTED.
 *     2. Walk from (n, j, n, j) by FIT's walk rule, with the same start state, tie-breaks and stop rule.  This gives
 *        start, the trace and complete.  (The one-layer walk is always complete, as in bialign_batch_get_traces.)
 *     3. The walk's span in B is [start, j).  If the walk is complete and the span intersects no accepted hit's span,
 *        accept it.  Record (start, end = j, score = E(j), trace).  Mask every end x with start < x <= j, and j itself.
 *        Otherwise discard it and mask j only.  (Spans [s, e) and [s', e') intersect when s < e' and s' < e.)
 *     4. Append (end, start, score, accepted) to the pair's walk log, in every case.
 *     5. Stop with status MAX_HITS when max_hits hits are accepted.  Stop with status MAX_WALKS when max_walks walks are
 *        made.  (In this order: the walk that accepts hit max_hits as walk max_walks gives MAX_HITS.)
 *   Consequences.  Hits are disjoint in B.  Their scores do not increase in order of acceptance.  Hit 0 is the batch's own
 *     alignment, with the same span, score and trace bytes.
 *   Parameters.  min_score >= 1.  1 <= max_hits <= 256.  max_walks >= max_hits, and 0 means 4 * max_hits.
 *   Peak candidates (flags bit BIALIGN_HITS_PEAKS).  The ends just behind an accepted hit's end each score only one gap
 *     cost less, so they are the next-best candidates, and every one of them costs a discarded walk before a farther
 *     copy's end is reached.  An end j is a peak of the profile E(0..m) when (j = 0 or E(j-1) < E(j)) and (j = m or
 *     E(j+1) <= E(j)).  With the flag, every end that is not a peak is masked before the first round.  Steps 1-5 are
 *     unchanged: the masks on acceptance, the log and the stop reasons all stay as they are.  Hit 0 is still the batch's
 *     own alignment: the smallest j that attains the maximum has E(j-1) < E(j) (or j = 0) because it is the smallest, and
 *     E(j+1) <= E(j) (or j = m) because E(j) is the maximum, so it is a peak.  The peaks are a property of the profile
 *     only.  They do not depend on the mask's later state.  flags 0 is the search without the rule, bit for bit; any
 *     other bit is BIALIGN_E_INVALID.
 *   Thresholds (bialign_batch_set_hit_thresholds).  base_p = min_score[p] if the array is given, else spec.min_score.
 *     Emax_p is the maximum of the pair's profile, which is its fit score.  T_p = max(base_p, Emax_p > 0 ?
 *     ceil(min_permille * Emax_p / 1000) : 0), formed in 64 bits.  Candidates are the ends with E(j) >= T_p: T_p stands
 *     where min_score stands in step 1.  Without thresholds T_p = spec.min_score. */
typedef struct bialign_hit_spec {
  int32_t max_hits;
  int32_t max_walks;
  int32_t min_score;
  int32_t flags; /* BIALIGN_HITS_PEAKS or 0 (the former reserved word: same offset and size) */
} bialign_hit_spec;

#define BIALIGN_HITS_PEAKS 1u /* bialign_hit_spec.flags: only the profile's peaks are candidates */

/* status of a pair's search */
#define BIALIGN_HITS_NOT_SEARCHED 0 /* no run yet, or a BIALIGN_RUN_FILL_ONLY run */
#define BIALIGN_HITS_EXHAUSTED 1
#define BIALIGN_HITS_MAX_HITS 2
#define BIALIGN_HITS_MAX_WALKS 3

typedef struct bialign_hit_info {
  bialign_hit_spec spec; /* as set, max_walks resolved (0 -> 4 * max_hits) */
  int64_t buffer_bytes;  /* HBM of the result buffers: profile, walk log, hit records, trace slots (outside hbm_budget_bytes) */
  double search_ms;      /* HIP-event time of the search kernels of the last run, summed over its chunks (events of their
                            own: not part of fill_ms or traceback_ms) */
} bialign_hit_info;

/* Give the batch a hit search (spec != NULL) or take it away again (spec == NULL); after create, ahead of a run.  Allocates
 * the result buffers for the whole batch: profile (sum of m + 1 words), walk log and hit records ([npairs][max_walks] and
 * [npairs][max_hits] records of four words), max_hits trace slots of the pair's trace capacity each; the mask of the
 * candidates and the accepted spans live in the kernel's LDS.  A batch that is not FIT, is SCORE_ONLY, or is a null batch:
 * BIALIGN_E_UNSUPPORTED (the search needs a FIT batch in full storage).  So it is when the mask (m + 1 bits), the spans and
 * the tracebacks' staged inputs together pass 160 KiB of LDS.  A bad spec: BIALIGN_E_INVALID.  An allocation that fails:
 * BIALIGN_E_NOMEM, and the batch stays usable without hits.  Without a search a run enqueues exactly what it did before:
 * no launch, no event, no allocation.  With one, the results are reset ahead of every run, as the spans are; a
 * BIALIGN_RUN_FILL_ONLY run leaves the profile and status NOT_SEARCHED, with no hits and no walks. */
int bialign_batch_set_hits(bialign_batch* b, const bialign_hit_spec* spec);
/* Per-pair thresholds of the search ("Thresholds" above); after bialign_batch_set_hits, ahead of a run.  min_score is
 * [npairs], indexed by pair id (not by launch slot), or NULL; min_permille is 0..1000.  The array is copied to HBM and its
 * bytes count in bialign_hit_info.buffer_bytes.  A later bialign_batch_set_hits call, with a spec or with NULL, clears the
 * thresholds; a later call of this function replaces them.  Refused before any device call, and the batch stays usable
 * with the thresholds it had: no search set, an entry < 1 or a permille outside 0..1000: BIALIGN_E_INVALID; a failed
 * allocation: BIALIGN_E_NOMEM. */
int bialign_batch_set_hit_thresholds(bialign_batch* b, const int32_t* min_score /* [npairs] or NULL */, int32_t min_permille /* 0..1000 */);
/* The T_p the last run used, with or without thresholds set; -1 for every pair after no run or after a
 * BIALIGN_RUN_FILL_ONLY run.  No search set: BIALIGN_E_INVALID. */
int bialign_batch_get_hit_thresholds(const bialign_batch* b, int32_t* out /* [npairs] */);
/* Pair's profile E(0..m) of the last run.  No search set or no run since: BIALIGN_E_INVALID (so for the getters below). */
int bialign_batch_get_hit_profile(const bialign_batch* b, int32_t pair, int32_t* out /* [m+1] */);
/* The accepted hits, in order of acceptance.  nhits and status are [npairs]; start_b, end_b, score and trace_len are
 * [npairs][max_hits], entries at and beyond nhits[p] are -1; hit h of pair p has its columns at
 * trace[trace_off[p * max_hits + h] .. + trace_len[p * max_hits + h]), start -> end, in the byte code of
 * bialign_batch_get_traces: the global alignment of A with B[start_b:end_b].  trace must hold max_hits *
 * bialign_batch_info.trace_bytes bytes; trace and trace_off may both be NULL. */
int bialign_batch_get_hits(const bialign_batch* b, int32_t* nhits, int32_t* status, int32_t* start_b, int32_t* end_b,
                           int32_t* score, int32_t* trace_len, uint8_t* trace, int64_t* trace_off);
/* The walk log, in the order the walks were made.  nwalks is [npairs]; the others are [npairs][max_walks], -1 at and
 * beyond nwalks[p].  start_b is where the walk stopped. */
int bialign_batch_get_hit_walks(const bialign_batch* b, int32_t* nwalks, int32_t* end_b, int32_t* start_b, int32_t* score,
                                int32_t* accepted);
int bialign_batch_get_hit_info(const bialign_batch* b, bialign_hit_info* info);

/* Test / introspection hooks.
 * dump_layers re-runs the fill of one pair and writes its layers in the
 * reference's layout [layer][i][j][k-i+s][l-j+s] (pyx:27-41, 61-71), layers in
 * itertools.product order, cells the reference never writes left 0.
 * out must hold nlayers*(n+1)*(m+1)*(2s+1)^2 int32. */
int bialign_batch_dump_layers(bialign_batch* b, int32_t pair, int32_t* out);
/* dump_mu2: pair's mu2 table as the sweep reads it, out[(k-1)*m + (l-1)], n*m int32.  FEATURE form: the table is built
 * anew for this pair; DENSE form: the uploaded table; LOOKUP form, and any null batch (its tables are the replicas'):
 * BIALIGN_E_INVALID. */
int bialign_batch_dump_mu2(bialign_batch* b, int32_t pair, int32_t* out);

/* A null batch: every pair of `pairs` against `spec->replicas` shuffles of its B molecule (THE PERMUTATION above), as a
 * SCORE_ONLY batch of npairs * replicas alignments (the flag is forced; LEAN_TRACE or LEVEL_TRACE in params->flags:
 * BIALIGN_E_INVALID).  Every max_shift and both recurrences as for SCORE_ONLY (the one-layer recurrence beyond
 * BIALIGN_MAX_SHIFT_TILED: BIALIGN_E_UNSUPPORTED).  spec NULL, replicas outside 1..65535 or npairs * replicas above
 * INT32_MAX: BIALIGN_E_INVALID; mu1_dense / mu2_dense set: BIALIGN_E_UNSUPPORTED; a pair whose replica scores could
 * overflow the int64 sum of squares (replicas * bound^2, bound from the int32 safety window's column bound):
 * BIALIGN_E_RANGE.  The replicas' codes are input data like the uploaded codes: outside hbm_budget_bytes (and
 * subtracted from the free memory a budget of 0 is taken from).  run / wait / get_timing / get_info work as for any
 * batch: bialign_batch_info.npairs is the number of real pairs, cells counts all replicas; bialign_batch_get_scores
 * fails with BIALIGN_E_INVALID (a null batch has no observed score), get_traces / dump_layers as for SCORE_ONLY. */
int bialign_batch_create_null(bialign_engine* eng, const bialign_params* params, const bialign_scoring* scoring,
                              const bialign_pairs* pairs, const bialign_null_spec* spec, int64_t hbm_budget_bytes,
                              bialign_batch** out);
/* The replica scores of the last run, pair-major: out[p * replicas + r]. */
int bialign_batch_get_null_scores(const bialign_batch* b, int32_t* out /* [npairs * replicas] */);
/* One wave per pair reduces its replica scores on the GPU.  observed: the real pairs' scores (e.g. of a SCORE_ONLY
 * batch of the same pairs) for n_ge, or NULL (n_ge = 0). */
int bialign_batch_get_null_stats(const bialign_batch* b, const int32_t* observed /* [npairs] or NULL */,
                                 bialign_null_stats* out /* [npairs] */);
int bialign_batch_get_null_info(const bialign_batch* b, bialign_null_info* info);
/* Test hook: the codes of one replica of one pair's B as the sweep reads them (len_b bytes each; the shuffle kernel is
 * run for that replica). */
int bialign_batch_dump_null_codes(bialign_batch* b, int32_t pair, int32_t replica, uint8_t* seq, uint8_t* cls);

/* The null model of a null batch of any form (added symbols: no existing struct or function changes): BIALIGN_NULL_MONO,
 * THE PERMUTATION, which a batch has until told otherwise, or BIALIGN_NULL_DINUCLEOTIDE, THE DINUCLEOTIDE PERMUTATION.
 * Valid between runs (a pending run is waited for); the model holds from the next run on, and the three dumps
 * (dump_null_codes / _features / _tables) follow it.  Refused before any device call, the batch keeping its model: not a
 * null batch, or an unknown model: BIALIGN_E_INVALID; BIALIGN_NULL_DINUCLEOTIDE on a DENSE-form null batch whose mu1 is
 * dense (B has no letters), or with a B molecule of more than BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN residues:
 * BIALIGN_E_UNSUPPORTED.  Under BIALIGN_NULL_MONO a LOOKUP-form null batch takes B of any length, as before. */
int bialign_batch_set_null_model(bialign_batch* b, int32_t model);
int bialign_batch_get_null_model(const bialign_batch* b, int32_t* model);

/* A null batch with mu2 in FEATURE form: the union of bialign_batch_create_features and bialign_batch_create_null (new in
 * ABI 10 as added symbols: no existing struct or function changes).  B's codes and features are uploaded once; the GPU
 * writes the R shuffled copies of every pair's B -- sequence codes and three planes of doubles, THE PERMUTATION above --
 * and builds each chunk's mu2 tables from the replicas' planes.  SCORE_ONLY is forced (LEAN_TRACE / LEVEL_TRACE:
 * BIALIGN_E_INVALID).  mu1 in LOOKUP form only: mu1_dense set is BIALIGN_E_UNSUPPORTED, for the reason
 * bialign_batch_create_null gives; cls_a / cls_b / mu2_dense / mu2_off are ignored (may be NULL).  A NULL argument, feat
 * or one of its arrays NULL, spec NULL, replicas outside 1..65535, npairs * replicas above INT32_MAX, a NaN, infinite or
 * negative feature (the message names pair and position): BIALIGN_E_INVALID.  The features are checked, and the pair's
 * bound (bialign_batch_create_features) is taken, on the real pairs, once each: a shuffle moves B's numbers and leaves
 * their maxima, so the real pair's bound serves all its replicas; a bound outside the int32 safety window, or replicas *
 * bound^2 outside int64: BIALIGN_E_RANGE.  The one-layer recurrence beyond BIALIGN_MAX_SHIFT_TILED, or a B molecule of
 * more than 65535 residues (the shuffle's index array is 16 bits wide): BIALIGN_E_UNSUPPORTED.
 * Memory: the replicas' planes, 24 * R * (sum of len_b) bytes, are input data like the replicas' codes -- outside
 * hbm_budget_bytes, and subtracted from the free memory a budget of 0 is taken from.  Every replica's n x m table is
 * per-chunk scratch inside the chunk plan, as for any FEATURE batch; one replica's table plus layers beyond the budget:
 * BIALIGN_E_NOMEM.
 * get_null_scores / get_null_stats / get_null_info / dump_null_codes (cls: zeros) work as for any null batch,
 * get_feature_info says FEATURE (build_ms, build_launches, table_bytes as usual); get_scores, get_traces, dump_layers
 * and dump_mu2 refuse as for null batches. */
int bialign_batch_create_null_features(bialign_engine* eng, const bialign_params* params, const bialign_scoring* scoring,
                                       const bialign_pairs* pairs, const bialign_features* feat,
                                       const bialign_null_spec* spec, int64_t hbm_budget_bytes, bialign_batch** out);
/* Test hook: the features of one replica of one pair's B as the table builder reads them (len_b doubles each; the
 * shuffle kernel is run for that replica).  Not a FEATURE-form null batch: BIALIGN_E_INVALID. */
int bialign_batch_dump_null_features(bialign_batch* b, int32_t pair, int32_t replica, double* up, double* down,
                                     double* unp);

/* A null batch with mu1 and / or mu2 in DENSE form (new in ABI 10 as added symbols: no existing struct or function
 * changes).  The null model is stated with THE PERMUTATION above: every replica's tables are the real pair's with their
 * columns permuted, on the GPU -- nothing of size R * n * m is made or uploaded by the host.  At least one of
 * pairs->mu1_dense / mu2_dense must be set (neither: BIALIGN_E_INVALID -- that batch is bialign_batch_create_null's); a
 * table without its offsets (mu1_off / mu2_off): BIALIGN_E_INVALID.  The other of mu1 / mu2 may be in LOOKUP form; its
 * codes (seq_a / seq_b for mu1, cls_a / cls_b for mu2) are then required as in bialign_batch_create_null, the codes of a
 * dense form are ignored (may be NULL).  SCORE_ONLY is forced (LEAN_TRACE / LEVEL_TRACE: BIALIGN_E_INVALID); spec,
 * replicas and npairs * replicas are checked as in bialign_batch_create_null.  The one-layer recurrence beyond
 * BIALIGN_MAX_SHIFT_TILED, or a B molecule of more than 65535 residues (the permutations are kept 16 bits wide):
 * BIALIGN_E_UNSUPPORTED.  The range checks (the int32 safety window from the tables' largest magnitude, then replicas *
 * bound^2 within int64: BIALIGN_E_RANGE) are taken on the real tables, once: a column permutation leaves a table's
 * maximum where it is.  Dense mu1 together with FEATURE mu2 in a null batch does not exist.
 * Memory: the real pairs' tables stay resident, uploaded once, 4 * (sum of n * m) bytes per dense form; like the replicas'
 * codes and permutations (bialign_null_info.replica_bytes) they are input data outside hbm_budget_bytes, and subtracted
 * from the free memory a budget of 0 is taken from.  Every replica's permuted tables are per-chunk scratch inside the
 * chunk plan (4 * n * m bytes per dense form, mu2's table first, then mu1's); one replica's tables plus layers beyond the
 * budget: BIALIGN_E_NOMEM.
 * get_null_scores / get_null_stats / get_null_info / dump_null_codes (the codes of a dense form: zeros) work as for any
 * null batch, get_feature_info as bialign_feature_info says; get_scores, get_traces, dump_layers and dump_mu2 refuse as
 * for null batches. */
int bialign_batch_create_null_dense(bialign_engine* eng, const bialign_params* params, const bialign_scoring* scoring,
                                    const bialign_pairs* pairs, const bialign_null_spec* spec, int64_t hbm_budget_bytes,
                                    bialign_batch** out);
/* Test hook: the tables of one replica of one pair as the sweep reads them, out[(i-1)*m + x], n * m int32 each (the
 * permutation and the tables are made anew for that replica).  An out pointer may be NULL -- and must be for a form the
 * batch holds in LOOKUP form.  Not a DENSE-form null batch: BIALIGN_E_INVALID. */
int bialign_batch_dump_null_tables(bialign_batch* b, int32_t pair, int32_t replica, int32_t* mu1_out, int32_t* mu2_out);

#ifdef __cplusplus
}
#endif
#endif /* BIALIGN_H */
