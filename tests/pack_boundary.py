"""Test-side mirror of the packed-record range contract (Pack<S>, bialign_amd/csrc/bialign_types.hpp) and the inputs
that put one lane record exactly at its limits.  Shared by test_pack_boundary_host.py (no GPU: the case list is what
it claims to be, from the oracle alone) and test_gpu_pack_boundary.py (the sweeps agree with the verdict).

The contract: in an INTERIOR step a lane record -- the W*9 layer values of one (i, j, a) -- is stored as a base and
16-bit low halves.  base = anchor - 0x8000, the anchor being state 8 of band column 0; every value must lie in
[base, base + 0xfffe]; offset 0xffff marks -2^30 in the slots pack_corner names.  So a record fits iff
max - anchor <= 0x7ffe and anchor - min <= 0x8000.  Every other step stores full int32 records.
"""
import functools

import numpy as np

NEG = -(1 << 30)
HI_LIMIT, LO_LIMIT = 0x7FFE, 0x8000


class Geometry:
    """Sweep geometry of one pair at max_shift s.  The engine reports none of these numbers to Python, so each is
    restated once, next to the line it mirrors."""

    def __init__(self, s, n, m):
        self.S, self.n, self.m = s, n, m
        self.W = 2 * s + 1                                   # bialign_types.hpp:82  Geo<S>::W
        self.R = 64 // self.W                                # bialign_types.hpp:83  Geo<S>::R
        self.RR = self.R - 1                                 # bialign_types.hpp:84  Geo<S>::RR
        self.MAXOFF = 2 * (self.R - 1) + (self.W - 1)        # bialign_types.hpp:86  Geo<S>::MAXOFF
        self.LO = s + 1 + self.MAXOFF                        # bialign_types.hpp:169 Pack<S>::LO
        self.Q0 = (s + 2 + self.RR - 1) // self.RR           # bialign_types.hpp:170 Pack<S>::Q0
        self.HI = m - s                                      # bialign_types.hpp:171 Pack<S>::hi
        self.BLK = 8 if s <= 1 else 4                        # bialign_feed.hpp:30   GhostFeed<S,9>::BLK
        min_goff = 2 * self.BLK + 8                          # bialign_feed.hpp:45   GhostFeed::MIN_GOFF
        self.NS = (n + 1 + self.RR - 1) // self.RR           # bialign_plan.hpp  sweep_geometry
        self.P = max(m + 2, 2 * (self.R - 1) + min_goff)     # (sweep_geometry)
        self.G = (self.NS - 1) * self.P + m + self.MAXOFF + 1  # (sweep_geometry)
        self.CHECK = 16                                      # bialign_types.hpp:180 Pack<S>::CHECK

    def place(self, i, j, aa):
        """(strip, lane row, step-strip, phase) of lane record (i, j, aa): packed_cell, bialign_types.hpp:237-241."""
        strip = i // self.RR
        il = i - strip * self.RR + 1
        t = j + 2 * il + aa
        over = 1 if t >= self.P else 0
        return strip, il, strip + over, t - over * self.P

    def interior(self, qs, c):
        return qs >= self.Q0 and self.LO <= c <= self.HI     # bialign_types.hpp:172 Pack<S>::interior

    def local_step(self, i, j, aa, team=1):
        """Step g of the wave that sweeps (i, j, aa) -- the wave of a team of ``team`` that owns the record's strip --
        counted from that wave's first step (fill_affine_kernel: record = g + rec_base, rec_base = (q (T-1) + w) P)."""
        strip, il, _, _ = self.place(i, j, aa)
        return (strip // team) * self.P + j + 2 * il + aa

    def wave_steps(self, team=1, w=0):
        """H of fill_affine_kernel: the steps wave w of a team walks."""
        nsw = (self.NS - w + team - 1) // team
        return (nsw - 1) * self.P + self.m + self.MAXOFF + 1 if nsw > 0 else 0


def pack_corner(W, st, bb):
    """bialign_types.hpp:140."""
    return (bb == 0 and st in (3, 5, 6)) or (bb == W - 1 and st in (1, 2, 7))


def pack_verdict(layers, n, m, s):
    """The oracle's nine full layers [9][i][j][a][b] -> dict of int64 / bool arrays indexed [i, j, a]:
    ``hi`` = max - anchor and ``lo`` = anchor - min over the record's W*9 values (corner slots holding -2^30 do not
    count), ``interior`` = the record's step stores packed records, ``fits`` = hi <= 0x7ffe and lo <= 0x8000.
    Lane records outside the lattice (k = i + a - s not in 0..n) are never interior."""
    geo = Geometry(s, n, m)
    W = geo.W
    lay = np.asarray(layers, dtype=np.int64)
    assert lay.shape == (9, n + 1, m + 1, W, W)
    vals = lay.transpose(1, 2, 3, 0, 4)                      # [i, j, a, state, b]
    corner = np.array([[pack_corner(W, st, bb) for bb in range(W)] for st in range(9)])
    skip = corner[None, None, None] & (vals == NEG)
    anchor = vals[:, :, :, 8, 0]
    hi = np.where(skip, np.iinfo(np.int64).min, vals).max(axis=(3, 4)) - anchor
    lo = anchor - np.where(skip, np.iinfo(np.int64).max, vals).min(axis=(3, 4))
    i, j, aa = np.meshgrid(np.arange(n + 1), np.arange(m + 1), np.arange(W), indexing="ij")
    strip = i // geo.RR
    il = i - strip * geo.RR + 1
    t = j + 2 * il + aa
    over = (t >= geo.P).astype(np.int64)
    qs, c = strip + over, t - over * geo.P
    k = i + aa - s
    interior = (qs >= geo.Q0) & (c >= geo.LO) & (c <= geo.HI) & (k >= 0) & (k <= n)
    fits = (hi <= HI_LIMIT) & (lo <= LO_LIMIT)
    return dict(hi=hi, lo=lo, interior=interior, fits=fits, geo=geo)


def excess(v):
    """By how much each record misses its limits (<= 0: fits, 0: fits with no margin to spare), and on which side."""
    eh, el = v["hi"] - HI_LIMIT, v["lo"] - LO_LIMIT
    return np.maximum(eh, el), np.where(eh >= el, 0, 1)      # side 0 = hi, 1 = lo


def offenders(v):
    """Sorted (i, j, a) of the interior records that do not fit."""
    return sorted(map(tuple, np.argwhere(v["interior"] & ~v["fits"]).tolist()))


def falls_back(v):
    return bool((v["interior"] & ~v["fits"]).any())


# ---- inputs: a low-spread background and one spike -------------------------------------------------------------

#: small scores and costs: every record's hi and lo stay far below 4096 (asserted from the oracle, test_pack_boundary_host)
BACKGROUND = dict(type="Protein", simmatrix=None, structure_weight=23, gap_opening_cost=-9, gap_cost=-7, shift_cost=-11,
                  sequence_match_similarity=31, sequence_mismatch_similarity=-13, max_shift=1)
ALPHABET = "ARNDCQEGHILKMFPSTYV"   # synth.PROTEIN_ALPHABET without W: the letter the LOOKUP spike sits on
SPIKE_LETTER = "W"


def background_pair(seed, n, m):
    import random
    rng = random.Random(seed)
    draw = lambda alphabet, length: "".join(rng.choice(alphabet) for _ in range(length))
    return draw(ALPHABET, n), draw(ALPHABET, m), draw("HECT", n), draw("HECT", m)


class Case:
    """One input: a background pair and a spike of ``x`` (added to the background score) at 1-based ``pos``.
    family "mu2": dense mu2, entry (k0, l0); "mu1": dense mu1, entry (i0, j0); "lookup": the letter W at A[i0], B[j0]
    and nowhere else, the spike in its s1 entry."""

    def __init__(self, name, family, s, seed, n, m, pos, x, shoulder=0, **tags):
        self.name, self.family, self.s, self.seed, self.n, self.m = name, family, s, seed, n, m
        self.pos, self.x, self.shoulder, self.tags = tuple(pos), int(x), int(shoulder), tags

    def __repr__(self):
        return self.name

    @property
    def params(self):
        return dict(BACKGROUND, max_shift=self.s)

    @functools.cached_property
    def pair(self):
        sa, sb, ta, tb = background_pair(self.seed, self.n, self.m)
        if self.family == "lookup":
            i0, j0 = self.pos
            sa = sa[:i0 - 1] + SPIKE_LETTER + sa[i0:]
            sb = sb[:j0 - 1] + SPIKE_LETTER + sb[j0:]
        return sa, sb, ta, tb

    @functools.cached_property
    def tables(self):
        """(n+1) x (m+1) mu1, mu2 as the oracle takes them."""
        from oracle import oracle
        mu1, mu2 = oracle.mu_tables(*self.pair, self.params)
        (mu2 if self.family == "mu2" else mu1)[self.pos] += self.x
        if self.shoulder:
            # dense mu2 only: the 2s entries left of the spike in its row are lowered as well.  A spike of -X alone
            # drives lo in the records that see it at band column b >= 1 harder than hi in those that see it at b = 0
            # (there it pulls the anchor down); the shoulder pulls down the anchors of the former, so that hi leads.
            assert self.family == "mu2"
            k0, l0 = self.pos
            mu2[k0, max(1, l0 - 2 * self.s):l0] -= self.shoulder
        return mu1, mu2

    def with_x(self, x):
        return Case(self.name, self.family, self.s, self.seed, self.n, self.m, self.pos, x, self.shoulder, **self.tags)

    def key(self):
        return (self.family, self.s, self.seed, self.n, self.m, self.pos, self.x, self.shoulder)

    def make_batch(self, **kw):
        """The engine's batch of this one pair, in the case's input form."""
        return make_batch([self], **kw)


_REF = {}


def reference(case):
    """Oracle solve of a case (score, layers, trace, complete) and its verdict; computed once per distinct input."""
    k = case.key()
    if k not in _REF:
        from oracle import oracle
        ref = oracle.solve_tables(case.n, case.m, case.params, *case.tables)
        ref["verdict"] = pack_verdict(ref["layers"], case.n, case.m, case.s)
        _REF[k] = ref
    return _REF[k]


def make_batch(cases, **kw):
    """One engine batch of several cases of one family and max_shift."""
    from bialign_amd.batch import encode_flat
    from bialign_amd.engine import Batch, default_engine
    fam, params = cases[0].family, cases[0].params
    assert all(c.family == fam and c.s == cases[0].s for c in cases)
    model, fb = encode_flat([c.pair for c in cases], params)
    s1 = np.array(model.s1, dtype=np.int32)
    if fam == "lookup":
        w = model.seq_index[SPIKE_LETTER]
        assert len({c.x for c in cases}) == 1, "one s1 table per batch"
        s1[w, w] += cases[0].x
    if fam == "mu2":
        kw["mu2_dense"] = [c.tables[1][1:, 1:] for c in cases]
    if fam == "mu1":
        kw["mu1_dense"] = [c.tables[0][1:, 1:] for c in cases]
    return Batch(default_engine(), fb, None, s1, model.s2, params["gap_opening_cost"], params["gap_cost"],
                 params["shift_cost"], params["max_shift"], **kw)


# ---- the case list: fixed numbers, solved from the oracle (two runs per family and side showed the worst record's
# excess moving one for one with the spike; test_pack_boundary_host.py recomputes every claim made here) -------------
#: section a: (family, max_shift, side) -> (n, m, spike position, the spike at which the worst record fits with no margin,
#: shoulder).  A positive spike in a dense mu2 entry does not serve for the hi side: every later cell inherits it, and the
#: record whose ANCHOR sees the entry (lo side) leads the records that see it at b >= 1 by more than the two units the limits
#: differ by -- so both mu2 sides use -X, the hi side with the shoulder (Case.tables).
MARGIN_ZERO = {
    ("lookup", 1, "hi"): (130, 300, (67, 150), -32787, 0), ("lookup", 1, "lo"): (130, 300, (67, 150), 32646, 0),
    ("mu2", 1, "hi"): (130, 300, (67, 150), -32708, 1000), ("mu2", 1, "lo"): (130, 300, (67, 150), -32708, 0),
    ("lookup", 2, "hi"): (70, 90, (25, 41), -32757, 0), ("lookup", 2, "lo"): (70, 90, (25, 41), 32664, 0),
    ("mu2", 2, "hi"): (70, 90, (25, 41), -32735, 1000), ("mu2", 2, "lo"): (70, 90, (25, 41), -32701, 0),
    ("lookup", 3, "hi"): (60, 80, (19, 38), -32753, 0), ("lookup", 3, "lo"): (60, 80, (19, 38), 32618, 0),
    ("mu2", 3, "hi"): (60, 80, (19, 38), -32713, 1000), ("mu2", 3, "lo"): (60, 80, (19, 38), -32679, 0),
    ("mu1", 1, "hi"): (90, 100, (47, 60), -32704, 0), ("mu1", 1, "lo"): (90, 100, (47, 60), 32698, 0),
}
#: margins +1, 0, -1: fits with one to spare, fits exactly, misses by one -- the spike shrinks or grows by one
BOTH_SIDES = [Case(f"a-{fam}-s{s}-{side}-margin{mg:+d}", fam, s, 1, n, m, pos, x0 - (1 if x0 > 0 else -1) * mg, shoulder,
                   side=side, margin=mg)
              for (fam, s, side), (n, m, pos, x0, shoulder) in MARGIN_ZERO.items() for mg in (1, 0, -1)]
#: sections b and c: one lane record misses by exactly one (``offenders``), or -- where the step is not interior and stores
#: a full record -- a spike of any size leaves everything packed (``offenders`` empty).  LOOKUP form, max_shift 1,
#: n = 110 (six strips, the last one filled up to lane row 11 of 20), m = 280 (P = 282: the period admits teams of three,
#: the only team size at which timing() tells fill_affine_slim_kernel from fill_affine_kernel).  ``team``: the case is
#: placed in the step count of the wave that sweeps it in a team of that size, and runs with that team only.
CONFINED = [
    Case("b-first-interior-column", "lookup", 1, 2, 110, 280, (47, 28), -32779, offenders=[(47, 28, 0)]),
    Case("b-last-interior-column", "lookup", 1, 2, 110, 280, (47, 263), -32834, offenders=[(47, 263, 0)]),
    Case("b-first-interior-strip", "lookup", 1, 2, 110, 280, (24, 64), -32810, offenders=[(24, 64, 0)]),
    Case("b-row-n-of-partial-last-strip", "lookup", 1, 2, 110, 280, (110, 53), -32746, offenders=[(110, 53, 0)]),
    Case("b-column-before-first-interior", "lookup", 1, 2, 110, 280, (47, 25), -40000, offenders=[]),
    Case("b-column-after-last-interior", "lookup", 1, 2, 110, 280, (47, 264), -40000, offenders=[]),
    Case("b-strip-before-first-interior", "lookup", 1, 2, 110, 280, (10, 60), -40000, offenders=[]),
    Case("c-step-before-a-check-team1", "lookup", 1, 2, 110, 280, (87, 38), -32784, offenders=[(87, 38, 1)], team=1),
    Case("c-step-after-a-check-team1", "lookup", 1, 2, 110, 280, (87, 56), -32737, offenders=[(87, 56, 0)], team=1),
    Case("c-row-that-leaves-the-lattice-team1", "lookup", 1, 2, 110, 280, (94, 249), -32803, offenders=[(94, 249, 0)], team=1),
    Case("c-step-before-a-check-team3", "lookup", 1, 2, 110, 280, (87, 69), -32765, offenders=[(87, 69, 0)], team=3),
    Case("c-step-after-a-check-team3", "lookup", 1, 2, 110, 280, (87, 37), -32787, offenders=[(87, 37, 1)], team=3),
    Case("c-row-that-leaves-the-lattice-team3", "lookup", 1, 2, 110, 280, (54, 249), -32829, offenders=[(54, 249, 0)], team=3),
    Case("c-last-interior-step-of-sweep", "lookup", 1, 2, 110, 280, (105, 267), -32830, offenders=[(105, 267, 0)]),
    Case("c-first-interior-step-of-last-strip", "lookup", 1, 2, 110, 280, (105, 32), -32759, offenders=[(105, 32, 0)]),
]
#: section a at max_shift 2 and 3 in a cross-CU team: the period must reach 256 columns for a team of two (m = 256)
CROSS_CU = [
    Case("a-lookup-s2-xcu-hi-margin+0", "lookup", 2, 1, 50, 256, (25, 61), -32761, side="hi", margin=0),
    Case("a-lookup-s2-xcu-hi-margin-1", "lookup", 2, 1, 50, 256, (25, 61), -32762, side="hi", margin=-1),
    Case("a-lookup-s3-xcu-hi-margin+0", "lookup", 3, 1, 40, 256, (19, 58), -32779, side="hi", margin=0),
    Case("a-lookup-s3-xcu-hi-margin-1", "lookup", 3, 1, 40, 256, (19, 58), -32780, side="hi", margin=-1),
]
#: section d, one side at a time: ``record`` lies in the BOTTOM lane row of strip 2 and fits with no margin, so the strip
#: below replays a record that holds offset 0xfffe (hi) or 0x0000 (lo) through the in-sweep ghost feed -- the cooperative
#: unpack at max_shift 1, the per-lane unpack at 2.  ``marks``: (state, band column) slots of that record holding the
#: -2^30 mark (offset 0xffff).  Not covered: both limits in ONE record.
GHOST_ROW = [
    Case("d-bottom-row-s1-hi", "lookup", 1, 1, 130, 300, (59, 24), -32761, side="hi", record=(59, 24, 1), marks=[]),
    Case("d-bottom-row-s1-lo", "lookup", 1, 1, 130, 300, (59, 24), 32651, side="lo", record=(59, 24, 0),
         marks=[(1, 2), (2, 2), (7, 2)]),
    Case("d-bottom-row-s2-hi", "lookup", 2, 1, 70, 90, (32, 27), -32727, side="hi", record=(32, 27, 4),
         marks=[(3, 0), (5, 0), (6, 0)]),
    Case("d-bottom-row-s2-lo", "lookup", 2, 1, 70, 90, (32, 23), 32647, side="lo", record=(32, 23, 2), marks=[]),
]
CASES = {c.name: c for c in BOTH_SIDES + CROSS_CU + GHOST_ROW + CONFINED}
