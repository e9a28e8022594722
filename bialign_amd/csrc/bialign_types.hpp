// bialign_types.hpp -- constants, batch descriptors, sweep geometry and record layout.  Part of bialign_kernels.hpp (include that, not this).
#pragma once

namespace bialign {

constexpr int32_t NEG = -(1 << 30);                 // reference -infinity
constexpr int32_t SENT = -(1 << 30) - (1 << 29);    // "guard failed" marker
constexpr int32_t THRESH = -(1 << 30) - (1 << 28);  // below: no valid case
constexpr int NCOL = 65;                            // 64 lanes + 1 sentinel column
constexpr int PROG_WORDS = 256;                     // cross-CU teams: progress words per pair = largest team
// in-workgroup teams: progress words of a workgroup, in LDS (teams have at most twelve waves; the last two words are the
// free-end modes' floor words, bialign_free_ends.hpp)
constexpr int LDS_PROG_WORDS = 16;
constexpr int XCH_ROWS = 12;                        // affine sweeps: exchange rows per lattice point that go through LDS
// Bytes one array of a molecule's codes takes in LDS: whole dwords, `guard` bytes around (B's codes in the sweeps: Geo<S>::PADB)
__host__ __device__ constexpr int code_pad(int len, int guard = 0) { return (len + 2 * guard + 3) & ~3; }
typedef int v4i __attribute__((ext_vector_type(4)));

struct PairDesc {
  int32_t n, m;       // lengths of A, B
  int32_t NS, P, G;   // strips, column period, total steps of the sweep
  int32_t trace_cap;  // 2(n+m)+2
  int64_t seq_a, seq_b;   // offsets into the code arrays
  int64_t layer_off;      // dword offset of this pair's records in the chunk buffer
  int64_t trace_off;      // byte offset in the trace buffer
  int64_t tab_off;        // dense forms: start of this pair's tables in DeviceBatch::dense_tab (n x m each, mu2's first)
  int64_t scratch_off;    // lean traceback: dword offset of this pair's one-strip scratch records
                          // (level traceback, bialign_wide.hpp: of its segment scratch; the ring follows it.  Wide-band affine
                          // sweep in full storage or SCORE_ONLY: of its ring in DeviceBatch::wide_ring, chunk-relative)
};

// Lean traceback: where a pair's walk stands between two strips.
struct TraceState {
  int32_t i, j, k, l;     // current lattice point
  int32_t st, cur;        // its state and layer value
  int32_t d0, d1;         // running shifts (pyx:541-545)
  int32_t len;            // columns emitted so far (end -> start order)
  int32_t strip;          // strip the current point lies in (level traceback, bialign_wide.hpp: the segment to sweep next)
  int32_t started, done;  // 0/1
};

struct DeviceBatch {
  const PairDesc* pairs;
  const int32_t* order;  // launch order (block -> pair id)
  const uint8_t *seq_a, *cls_a, *seq_b, *cls_b;
  const int32_t *s1, *s2;
  int32_t k1, k2;
  int32_t beta, gamma, delta;
  int32_t* layers;      // chunk buffer
  int32_t* scores;      // [npairs]
  uint8_t* trace;       // trace buffer
  int32_t* trace_len;   // [npairs]
  int32_t* complete;    // [npairs]
  int32_t* errflag;     // [1] sticky device-side error (team protocol timeout)
  const int32_t* dense_tab;  // dense forms (DeviceBatch::dense_forms): the pairs' mu2(k,l) / mu1(i,j) tables (else nullptr)
  int32_t* prog;        // cross-CU teams: [pairs in launch][PROG_WORDS] progress words, zeroed per launch
  int32_t team;         // cross-CU teams: workgroups (= waves) per pair
  int32_t* scratch;     // lean traceback: full records of resw_k strips per pair
  TraceState* tstate;   // lean traceback: [npairs]
  int32_t resw_k;       // lean traceback: strips re-swept (in parallel) and walked per round
                        // (level traceback, bialign_wide.hpp: levels per segment, C)
  int32_t wide_s;       // wide-band path (max_shift beyond the tiled kernels): the band half-width
  int32_t prio_mode;    // 1 = rotate wave priorities by workgroup age (fill_affine_kernel); BIALIGN_PRIO=0 switches it off
  int32_t spin_limit;   // team hand-off: polls of the partner's progress word before a wave gives up (error flag)
  // wide-band affine sweep: derived values of the last WIDE_RING levels, the chunk's pairs end to end (a pair's at its
  // PairDesc::scratch_off) -- the part of the chunk buffer behind the layers (BatchPlan::ring_dwords)
  int32_t* wide_ring;
  const void* reserved1;         // null; it keeps the fields behind it at their offsets in the kernels' argument block
  int32_t wide_score_only;       // ... 1: no layers are stored, the last level's point writes the score
  int32_t launch_pairs;     // fill_affine_slim_kernel: pairs of this launch (a workgroup holds several)
  int32_t slim_code_bytes;  // fill_affine_slim_kernel: LDS bytes of one pair's sequence and class codes
  // Which scores come as dense tables: bit 0 mu2, bit 1 mu1.  The kernels built for a LOOKUP mu1 only look at
  // dense_tab (non-null = dense mu2); those built for a dense mu1 read the bits.  (It fills what was the struct's
  // tail padding: the kernel argument block of the existing kernels keeps its size.)
  int32_t dense_forms;
  // Whose end gaps are free in the sweeps that serve the global recurrence: a mask of FREE_B_ENDS | FREE_A_ENDS
  // (bialign_free_ends.hpp).  Fit alignments (BIALIGN_BATCH_FIT) set FREE_B_ENDS, overlap alignments
  // (BIALIGN_BATCH_OVERLAP, section 7e) both bits; global batches set none, and neither do LOCAL batches, whose sweeps are
  // built for the mode (see `local`).  Wave-uniform; the sweeps read it in their prologue (the floor words, applied in
  // boundary steps where is_origin is tested) and, LEAN forms, in their end rule (lean_end_rule); the generic tracebacks
  // in their prologue (they scan row n, in an overlap batch column m too) and stop test.
  int32_t free_ends;
  // Local alignments (BIALIGN_BATCH_LOCAL): free ends in both molecules.  Wave-uniform; the
  // sweeps built for it (template parameter LOCAL) do not read it, the generic tracebacks do, beside `free_ends`.  (It
  // fills the padding behind `free_ends`.)
  int32_t local;
  void* reserved0;  // null; it keeps the fields behind it at their offsets in the kernels' argument block
  // [npairs] the best end of a pair as a 64-bit key (bialign_free_ends.hpp: end_key_of), zeroed ahead of every run and
  // raised with atomicMax by the lanes of the LOCAL sweeps and of the LEAN sweeps of overlap batches; decoded behind
  // the sweep by end_key_finish_kernel.
  unsigned long long* end_key;
  // The pairs' spans, -1 until written.  One layout rule: a fit batch has 2 words per pair, (start_b, end_b); overlap and
  // local batches have 4, (start_a, end_a, start_b, end_b).  Ends: the LEAN sweeps (fit), end_key_finish_kernel, or the
  // tracebacks' prologue; starts: the tracebacks.
  int32_t* span;
};
static_assert(sizeof(DeviceBatch) == 256, "DeviceBatch grew: the kernels' argument blocks would change");

// Dense mu1 (DeviceBatch::dense_forms bit 1): pair pd's n x m table, mu1(i,j) at [(i-1)*m + (j-1)].  It follows the
// pair's mu2 table when that one is dense too.
__host__ __device__ inline const int32_t* mu1_table(const DeviceBatch& A, const PairDesc& pd) {
  return A.dense_tab + pd.tab_off + ((A.dense_forms & 1) ? (int64_t)pd.n * pd.m : 0);
}

template <int S>
struct Geo {
  static constexpr int W = 2 * S + 1;
  static constexpr int R = 64 / W;       // lane rows per wave (incl. ghost row)
  static constexpr int RR = R - 1;       // real lattice rows per strip
  static constexpr int LIVE = R * W;     // lanes in use
  static constexpr int MAXOFF = 2 * (R - 1) + (W - 1);
  static constexpr int PADB = S + 1;     // guard bytes around B codes in LDS
};

// Record geometry: one record per step, ND dwords for each of the SL = RR*W real lanes
// (ghost and idle lanes own no storage), as NCH4 chunks [chunk][slot][4 dwords] followed by a
// [slot][TAIL] tail (64 slots, see TAILSLOTS), everything packed: a wave-wide store instruction writes one contiguous
// run of SL*16 bytes and consecutive instructions / steps continue where the last one ended,
// so every byte of a pair's region is written and L2 assembles full lines.
//   LEAN records (score-only batches): nobody will trace back, so a step keeps only what the
// next strip's ghost row replays -- the bottom real row, W slots -- in the same chunk layout.
template <int S, int NL, bool LEAN = false>
struct Rec {
  static constexpr int W = 2 * S + 1;
  static constexpr int SL = LEAN ? W : (64 / W - 1) * W;  // storage slots = real lanes (bottom row only if LEAN)
  static constexpr int ND = NL * W;
  static constexpr int NCH4 = ND / 4;
  static constexpr int TAIL = ND % 4;
  // A chunk holds SLP >= SL slots: where rounding SL up to a multiple of 8 costs at most two slots (s=2: 55 -> 56,
  // s=4: 54 -> 56) the spare lanes write them too and every chunk store covers whole 128-byte lines (-1..2 %).
  static constexpr int PADMAX = 2;  // the most pad slots a chunk takes on
  static constexpr int SLP = (!LEAN && (SL + 7) / 8 * 8 - SL <= PADMAX) ? (SL + 7) / 8 * 8 : SL;
  static constexpr int CH = SLP * 4;           // dwords per chunk
  // The tail has 64 slots, not SL: the spare lanes (ghost row, idle lanes) store don't-care values into the
  // last ones, so that a record ends on a 64-lane boundary -- at s=1 (6 x 960 + 768 B) it is 51 whole
  // 128-byte lines and consecutive records of a wave never share a line (3 % of the fill time).
  static constexpr int TAILSLOTS = LEAN ? SL : 64;
  static constexpr int RECDW = LEAN ? (SL * ND + 3) / 4 * 4 : NCH4 * CH + TAILSLOTS * TAIL;  // 16-byte pieces stay aligned
  __host__ __device__ static inline int64_t dword(int64_t g, int slot, int d) {
    return d < 4 * NCH4 ? g * RECDW + (d >> 2) * CH + slot * 4 + (d & 3)
                        : g * RECDW + NCH4 * CH + slot * TAIL + (d - 4 * NCH4);
  }
};

// ---------------------------------------------------------------------------
// Packed records (affine sweeps at max_shift 1..3, full storage).  In INTERIOR steps -- every lane's
// lattice points have all four coordinates >= 1 and lie inside the molecule -- each of a lane's ND
// layer values is either exactly -2^30 at one of six compile-time-known (state, b) positions
// (can_be_empty<W>) or lies within a few thousand of the lane's first value, so the lane record shrinks
// from ND dwords to  base + (ND - 1) halfwords  (base = M[(1,1,1,1)] of the lane's first point - 0x8000, so
// THAT value's offset is 0x8000 by construction and is not stored).  A halfword is the LOW HALF OF THE VALUE ITSELF
// (round 3; round 2 stored the offset value - base) -- no subtraction per value in the sweep: the
// offset is (halfword - low half of base) mod 2^16, exact while 0 <= value - base < 2^16;
// offset 0xffff at a can_be_empty position = -2^30: 14 dwords instead of 27 at s=1 (round 2 stored all ND offsets: 16),
// 24 instead of 45 at s=2, 32 instead of 63 at s=3 (36 in round 2).  The sweep verifies the range of every offset it stores; the first one that does
// not fit raises the device flag and the host repeats the batch with full records.  All other steps
// (strip changes, the first strip(s), the lattice border) keep full records in a second region of the
// pair's storage.  Which steps are interior is a function of the record number alone, so readers
// (ghost feed, tracebacks, dump) find a cell without any index:
//   record r = Q*P + t,  t = j + 2*il + aa  (Q = strip of the lane, t may reach into the next period)
//   phase c = r mod P, step-strip Qs = r div P;   interior  <=>  Qs >= Q0  and  LO <= c <= HI
// Layout of a packed record: NCH chunks [chunk][slot][4 dwords] like a full record's, then -- where the
// lane record is not a whole number of 16-byte chunks -- a tail [slot][TAILDW dwords].
// ---------------------------------------------------------------------------
// the six (state, band column) positions whose value can be exactly -2^30 in an interior step (= can_be_empty<W>)
__host__ __device__ constexpr bool pack_corner(int W, int st, int bb) {
  return (bb == 0 && (st == 3 || st == 5 || st == 6)) || (bb == W - 1 && (st == 1 || st == 2 || st == 7));
}

template <int S>
struct Pack {
  using G_ = Geo<S>;
  using R_ = Rec<S, 9>;
  static constexpr int ND = R_::ND;
  static constexpr int ANCHOR = 8;                     // value index (band column 0, state (1,1,1,1)) the base is taken from
  static constexpr int NHW = ND + 1;                   // halfwords of a lane record: base (2) + the other ND - 1 offsets
  static constexpr int NDW = (NHW + 1) / 2;            // ... dwords
  // whole 16-byte chunks, and a tail piece of TAILDW dwords per lane: 8 bytes at s=1 (14 dwords = 3 chunks + 2), none
  // at s=3 (32 dwords); a 12-byte tail (s=2: 23 dwords) is rounded up to a chunk -- three scalar dword stores per
  // lane (write-through ones in cross-CU teams) cost far more than the four bytes (config 4: 329 vs 165 ms)
  static constexpr int NCH = NDW / 4 + (NDW % 4 == 3 ? 1 : 0);
  static constexpr int TAILDW = NDW % 4 == 3 ? 0 : NDW % 4;
  static constexpr int NPC = NCH + (TAILDW ? 1 : 0);   // 16-byte pieces the ghost feed moves per lane record
  // tail slots: the storing lanes', rounded up so that records stay 16-byte aligned
  static constexpr int TSLOTS = TAILDW == 0 ? 0 : (TAILDW == 2 ? (R_::SL + 1) / 2 * 2 : (R_::SL + 3) / 4 * 4);
  static constexpr int RECDW = NCH * R_::CH + TSLOTS * TAILDW;
  static_assert(RECDW % 4 == 0, "packed records must stay 16-byte aligned");
  // halfword of value v (v != ANCHOR) in the lane record, and the value a halfword h >= 2 holds
  __host__ __device__ static constexpr int hw(int v) { return 2 + v - (v > ANCHOR ? 1 : 0); }
  __host__ __device__ static constexpr int val(int h) { return h - 2 < ANCHOR ? h - 2 : h - 1; }
  // dword offset of lane-record dword d of storage slot `slot` inside a packed record
  __host__ __device__ static constexpr int dwpos(int slot, int d) {
    return d < 4 * NCH ? (d >> 2) * R_::CH + slot * 4 + (d & 3) : NCH * R_::CH + slot * TAILDW + (d - 4 * NCH);
  }
  static constexpr int LO = S + 1 + G_::MAXOFF;       // first phase at which every lane has passed column S
  static constexpr int Q0 = (S + 2 + G_::RR - 1) / G_::RR;  // first strip whose ghost row is row >= S+1
  __host__ __device__ static inline int hi(int m) { return m - S; }  // last phase whose points all lie inside the molecule
  __host__ __device__ static inline bool interior(int qs, int c, int m) { return qs >= Q0 && c >= LO && c <= m - S; }
  __host__ __device__ static inline int nbs(int P, int m) { return P - (m - S - LO + 1); }  // full records per strip >= Q0
  // The sweeps' range check (fill_affine_kernel, fill_affine_slim_kernel): a lane ORs what it stores in interior steps
  // into an accumulator that is tested at the head of every step that is a multiple of CHECK and of the ghost block, and
  // after the last step.  A lane whose row leaves the lattice at a strip change CLEARS the accumulator in its next interior
  // step, so a test has to fall between the last interior step of a strip and the update of the first interior step of the
  // next.  A wave walks through nbs(P, m) non-interior steps there (phases m - S + 1 .. P - 1, then 0 .. LO - 1; every lane
  // changes its row among them, at lane 0's phase 2 il + a <= MAXOFF < LO), at least CHECK_GAP since P >= m + 2.
  static constexpr int CHECK = 16;
  static constexpr int CHECK_GAP = LO + S + 1;
  __host__ __device__ static constexpr bool check_in_every_gap(int blk) {
    return (blk & (blk - 1)) == 0 && (CHECK & (CHECK - 1)) == 0 && (blk > CHECK ? blk : CHECK) <= CHECK_GAP;
  }
  // index of the full record of a non-interior step among the pair's full records
  __host__ __device__ static inline int64_t bidx(int qs, int c, int P, int m) {
    if (qs < Q0) return (int64_t)qs * P + c;
    return (int64_t)Q0 * P + (int64_t)(qs - Q0) * nbs(P, m) + (c < LO ? c : c - (m - S + 1) + LO);
  }
  // dwords of the pair's full-record region; records 0 .. G-1
  __host__ __device__ static inline int64_t full_records(int G, int P, int m) {
    const int nst = (G + P - 1) / P;  // step-strips touched
    return nst <= Q0 ? (int64_t)nst * P : (int64_t)Q0 * P + (int64_t)(nst - Q0) * nbs(P, m);
  }
  // dwords of a pair's storage in packed form: G packed records (those of non-interior steps stay unused), then
  // its full records
  __host__ __device__ static inline int64_t pair_dwords(int G, int P, int m) {
    return (int64_t)G * RECDW + full_records(G, P, m) * R_::RECDW;
  }
  // dwords a packed sweep writes (about: idle steps at the very end write nothing in either form)
  __host__ __device__ static inline int64_t written_dwords(int G, int P, int m) {
    const int64_t f = full_records(G, P, m);
    return (G - f) * RECDW + f * R_::RECDW;
  }
  // A halfword holds the LOW HALF OF THE VALUE ITSELF (round 3; round 2 stored the offset value - base): the sweep packs
  // without a subtraction per value and checks the range through a running minimum and maximum.  Saves the s=1 sweeps
  // 2.5 % (47.1 -> 45.9 ms at the headline shape).  At s=2 and 3, where every lane unpacks the ghost row in every step,
  // it only pays with the two-at-a-time unpacking below (config-4 chunk: offsets 73.4 ms, low halves unpacked value by
  // value 75, two at a time 72.0).
  // offset of a stored halfword h against the record's base
  __host__ __device__ static inline uint32_t offset_of(uint32_t h, int base) { return (h - (uint32_t)base) & 0xffffu; }
  // ... and of both halfwords of a record dword at once (device code: one v_pk_sub_u16 for two values instead of a
  // subtraction and a mask each; the caller picks a half, which folds into the addition of the base as an SDWA operand)
  typedef unsigned short pk_u16x2 __attribute__((ext_vector_type(2)));
  __device__ static inline uint32_t offsets_of(uint32_t word, int base) {
    const pk_u16x2 w = __builtin_bit_cast(pk_u16x2, word);
    const unsigned short b = (unsigned short)base;
    return __builtin_bit_cast(uint32_t, (pk_u16x2)(w - pk_u16x2{b, b}));
  }
  // value (state st of band column bb) of a lane slot in a packed record at p
  __host__ __device__ static inline int decode(const int32_t* p, int slot, int bb, int st, bool corner) {
    const int v = bb * 9 + st;
    const int base = p[slot * 4];  // both loads issued together: one memory round trip per cell
    if (v == ANCHOR) return base + 0x8000;
    const int h = hw(v);
    const uint32_t word = (uint32_t)p[dwpos(slot, h >> 1)];
    const uint32_t e = offset_of((h & 1) ? word >> 16 : word & 0xffffu, base);
    return (corner && e == 0xffffu) ? NEG : base + (int)e;
  }
};

// Store addresses of an INTERIOR step of fill_affine_slim_kernel, factored so that host code can
// call both halves (tests/step_addr_check.hip proves them against the sweep's per-lane bookkeeping).  In an interior
// step every lane of the wave is in the same strip, so the step's record is wave-uniform:
//     byte address of a store = pair's storage + record_byte(g, q, T, w, P)   -- scalar, + RECB per step
//                             + chunk_off(lane) | tail_off(lane)              -- lane constants
//                             + chunk_imm(c)    | TAIL_IMM                    -- immediates
// Packed records (Pack<S>) in the full-storage form, the bottom row's plain records (Rec<S,9,true>) in the LEAN form.
template <int S, bool LEAN>
struct StepAddr {
  using R_ = Rec<S, 9, LEAN>;
  using PK_ = Pack<S>;
  static constexpr int W = 2 * S + 1, R = 64 / W;
  static constexpr int RECB = (LEAN ? R_::RECDW : PK_::RECDW) * 4;   // bytes from one step's record to the next
  static constexpr int NCHUNK = LEAN ? R_::NCH4 : PK_::NCH;          // 16-byte chunk stores per lane and step
  static constexpr int TAILB = (LEAN ? R_::TAIL : PK_::TAILDW) * 4;  // bytes of a lane's tail piece
  static constexpr int TAIL_IMM = NCHUNK * R_::CH * 4;               // (s=1: 2880, within a global store's immediate)
  __host__ __device__ static constexpr int chunk_imm(int c) { return c * R_::CH * 4; }
  // local strip q of wave w (team of T) at local step g: the wave's steps continue the records of strips w, w+T, ...
  __host__ __device__ static inline int64_t record(int g, int q, int T, int w, int P) {
    return (int64_t)g + (int64_t)(q * (T - 1) + w) * P;
  }
  __host__ __device__ static inline int64_t record_byte(int g, int q, int T, int w, int P) {
    return record(g, q, T, w, P) * RECB;
  }
  // lanes that own storage slots in an interior step, and the slot
  __host__ __device__ static inline int pad_idx(int lane) { return lane < W ? lane : (lane >= R * W ? W + (lane - R * W) : 64); }
  __host__ __device__ static inline bool stores(int lane) {
    const int il = lane / W;
    return (lane < R * W && (LEAN ? il == R - 1 : il != 0)) || (!LEAN && pad_idx(lane) < R_::SLP - R_::SL);
  }
  __host__ __device__ static inline bool stores_tail(int lane) {
    return stores(lane) && TAILB != 0 && (LEAN || slot(lane) < PK_::TSLOTS);
  }
  __host__ __device__ static inline int slot(int lane) {
    if (LEAN) return lane % W;
    return pad_idx(lane) < R_::SLP - R_::SL ? R_::SL + pad_idx(lane) : lane - W;
  }
  // byte offsets of the lane's chunk slot and of its tail piece (lanes without a slot: 0, they store nothing)
  __host__ __device__ static inline uint32_t chunk_off(int lane) { return stores(lane) ? (uint32_t)slot(lane) * 16u : 0u; }
  __host__ __device__ static inline uint32_t tail_off(int lane) { return stores(lane) ? (uint32_t)(slot(lane) * TAILB) : 0u; }
};

// Where layer value (state st) of lattice point (i, j, aa, bb) lives in a pair swept with packed records: dwords from
// the start of the pair's storage (layers + pd.layer_off): packed_cell's address arithmetic on its own.  The short-chain
// traceback's side path loads through it, and tests/trace_fast_check.hip proves that kernel's incremental addresses
// against it.
struct PackedAddr {
  bool packed;      // the point's step is interior: a packed record; else a full record, and only `dw` counts
  bool corner;      // packed: a can_be_empty position, offset 0xffff there means -2^30
  bool anchor;      // packed: the value the base is taken from (base + 0x8000, no halfword of its own)
  int half;         // packed: which half of dword `hdw` holds the value's halfword
  int64_t dw;       // packed: the lane record's base dword; full record: the value's dword
  int64_t hdw;      // packed: the dword of the value's halfword (anchor: as dw)
};
template <int S>
__host__ __device__ inline PackedAddr packed_addr(const PairDesc& pd, int i, int j, int aa, int bb, int st) {
  using PK = Pack<S>;
  constexpr int W = 2 * S + 1, RR = Geo<S>::RR;
  const int strip = i / RR, il = i - strip * RR + 1;
  const int t = j + 2 * il + aa, over = t >= pd.P ? 1 : 0;
  const int slot = (il - 1) * W + aa;
  PackedAddr a{};
  if (PK::interior(strip + over, t - over * pd.P, pd.m)) {
    const int v = bb * 9 + st, h = PK::hw(v);
    const int64_t rec = ((int64_t)strip * pd.P + t) * PK::RECDW;
    a.packed = true;
    a.corner = pack_corner(W, st, bb);
    a.anchor = v == PK::ANCHOR;
    a.half = h & 1;
    a.dw = rec + slot * 4;
    a.hdw = a.anchor ? a.dw : rec + PK::dwpos(slot, h >> 1);
    return a;
  }
  a.dw = (int64_t)pd.G * PK::RECDW + PK::bidx(strip + over, t - over * pd.P, pd.P, pd.m) * Rec<S, 9>::RECDW +
         Rec<S, 9>::dword(0, slot, bb * 9 + st);
  a.hdw = a.dw;
  return a;
}
// ... and the value there, `base` being the start of the pair's storage
template <int S>
__host__ __device__ inline int packed_load(const int32_t* base, const PackedAddr& a) {
  if (!a.packed) return base[a.dw];
  const int b = base[a.dw];  // both loads issued together: one memory round trip per cell
  if (a.anchor) return b + 0x8000;
  const uint32_t word = (uint32_t)base[a.hdw];
  const uint32_t e = Pack<S>::offset_of(a.half ? word >> 16 : word & 0xffffu, b);
  return (a.corner && e == 0xffffu) ? NEG : b + (int)e;
}

// Layer value (state st) of lattice point (i, j, aa, bb) of a pair swept with packed records.  (The generic tracebacks
// and the dump keep this form, and with it their device code, instruction for instruction; tests/trace_fast_check.hip
// proves it equal to packed_load(packed_addr()) on every in-band cell.)
template <int S>
__host__ __device__ inline int packed_cell(const int32_t* layers, const PairDesc& pd, int i, int j, int aa, int bb, int st) {
  using PK = Pack<S>;
  constexpr int W = 2 * S + 1, RR = Geo<S>::RR;
  const int strip = i / RR, il = i - strip * RR + 1;
  const int t = j + 2 * il + aa, over = t >= pd.P ? 1 : 0;
  const int slot = (il - 1) * W + aa;
  const int32_t* base = layers + pd.layer_off;
  if (PK::interior(strip + over, t - over * pd.P, pd.m))
    return PK::decode(base + ((int64_t)strip * pd.P + t) * PK::RECDW, slot, bb, st, pack_corner(W, st, bb));
  return base[(int64_t)pd.G * PK::RECDW + PK::bidx(strip + over, t - over * pd.P, pd.P, pd.m) * Rec<S, 9>::RECDW +
              Rec<S, 9>::dword(0, slot, bb * 9 + st)];
}

// dword index of layer value (state st) of lattice point (i, j, aa, bb).
template <int S, int NL>
__host__ __device__ inline int64_t cell_dword(const PairDesc& pd, int i, int j, int aa, int bb,
                                              int st) {
  constexpr int W = 2 * S + 1, RR = Geo<S>::RR;
  const int strip = i / RR, il = i - strip * RR + 1;
  const int64_t g = (int64_t)strip * pd.P + j + 2 * il + aa;
  return pd.layer_off + Rec<S, NL>::dword(g, (il - 1) * W + aa, bb * NL + st);
}

}  // namespace bialign
