"""Inputs whose best end is TIED, inputs in which nothing aligns, and their scaled twins at the edge of the int32 safety
window -- with what the free-end modes (FIT, LOCAL, OVERLAP, the hit search of FIT) must give for them, from the CPU
oracle alone.  Shared by test_tied_ends_host.py (no GPU: every input is what it claims to be) and
test_gpu_tied_ends.py (every copy of the tie rule, bit-exact against the oracle).

The contract (include/bialign.h, DESIGN.md sections 7c-7f): among several end cells of the best score a mode reports the
smallest in (i, j) order; the hit search takes the largest E, then the smallest j.  The expectations are those of
fit_expected / local_expected / overlap_expected / hits_expected; this module adds the inputs and ``tied``: every end
that attains the score, in the order of the rule.

The pairs are built from a few parts.  A unit u: 9 residues drawn without W and P, structure all H.  v: u's letters
reversed, structure all E -- the same self-score, and nothing of it aligns with u.  Spacers: W with structure T in A, P with
structure C in B; a spacer residue scores below zero against everything on the other side.  With the README protein
parameters a unit scores 11700 against itself in both recurrences, every exact copy of it gives the same score, and no
alignment bridges a spacer: the copies' ends tie exactly.

Where a copy must be reached through a gap whose length differs from copy to copy (the OVERLAP pairs of the team shape),
the copies with the cheaper gap carry structure mismatches (H -> E, 800 each) that make up the difference: a gap of k
residues costs 2 (150 + 50 k) in the affine recurrence and 100 k in the one-layer one -- both alignments of the
bialignment open it -- so eight more gapped residues weigh one mismatch in either recurrence.

ORACLE BUDGET: about 240 core-seconds per test module, 32 s of wall time in a pool of 16 -- see BUDGET at the end of this
module (``estimate`` gives the model's figure per mode from ``cell_seconds``; test_tied_ends_host.py prints both).
"""
import functools
import random

import numpy as np

import fit_expected as fe
import hits_expected as he
import local_expected as le
import overlap_expected as oe
import window_edge as we
from bialign_amd import synth
from free_ends_expected import LOW, NONE, cell_seconds, tables_of
from free_ends_gpu import params_of
from pack_boundary import Geometry

MODES = ("fit", "overlap", "local")
EXPECT = {"fit": fe, "overlap": oe, "local": le}
ALPHABET = "".join(ch for ch in synth.PROTEIN_ALPHABET if ch not in "WP")
UNIT_SEED, UNIT_LEN, LONG_UNIT_LEN = 11, 9, 40
TEAM_SHAPE = (101, 278)   # tests/test_gpu_fit.py: the smallest shape that admits a team of three waves at max_shift 1


def rows_per_strip(s):
    """RR of the sweeps (bialign_types.hpp, Geo<S>::RR; tests/test_gpu_local.py's rows_of is 2 RR + 4)."""
    return 64 // (2 * s + 1) - 1


# ---- parts ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def unit(length=UNIT_LEN, seed=UNIT_SEED):
    return synth._draw(random.Random(seed), ALPHABET, length), "H" * length


def mirror(u):
    return u[0][::-1], "E" * len(u[0])


def worn(u, t):
    """u with its first t structure letters turned to E: t structure matches less."""
    return u[0], "E" * t + u[1][t:]


def y(k):
    return "W" * k, "T" * k


def z(k):
    return "P" * k, "C" * k


def cat(*parts):
    return "".join(p[0] for p in parts), "".join(p[1] for p in parts)


def pair_of(a_parts, b_parts):
    a, b = cat(*a_parts), cat(*b_parts)
    return a[0], b[0], a[1], b[1]


U = unit()
V = mirror(U)
LONG = unit(LONG_UNIT_LEN, UNIT_SEED + 1)


class Input:
    """One pair.  ``modes``: the modes it is for; ``tied``: {mode: the ends the construction plants, in the rule's order}
    (FIT: columns; LOCAL, OVERLAP: (i, j)) -- a claim that test_tied_ends_host.py holds against the oracle."""

    def __init__(self, name, a_parts, b_parts, modes, tied):
        self.name, self.pair, self.modes, self.tied = name, pair_of(a_parts, b_parts), tuple(modes), tied
        self.n, self.m = len(self.pair[0]), len(self.pair[1])

    def __repr__(self):
        return self.name


def row_input(name="row", lead=2):
    """A = y u y, B = z u z u z u z: LOCAL ties on one row in three columns; FIT ties in the same columns."""
    a, b = [y(lead), U, y(2)], [z(3), U, z(4), U, z(5), U, z(3)]
    r, cols = lead + UNIT_LEN, [12, 25, 39]
    return Input(name, a, b, ("local", "fit"), dict(local=[(r, c) for c in cols], fit=cols))


def column_input(name="column", between=4):
    """A = y u y u y, B = z u z: LOCAL ties in one column on two rows."""
    a, b = [y(3), U, y(between), U, y(2)], [z(2), U, z(2)]
    return Input(name, a, b, ("local",), dict(local=[(12, 11), (21 + between, 11)]))


def cross_input(name="cross", between=4):
    """A = u y v, B = v z u: u ~ u ends on column m, v ~ v on row n -- both end lines of OVERLAP, two rows and two columns
    of LOCAL."""
    a, b = [U, y(between), V], [V, z(5), U]
    ends = [(9, 23), (18 + between, 9)]
    return Input(name, a, b, ("local", "overlap"), dict(local=ends, overlap=ends))


def overlap_row_input():
    """A = u, B = u z u z u: three tied ends on row n (OVERLAP, FIT), the last one B's end."""
    ends = [(9, 9), (9, 22), (9, 36)]
    return Input("overlap-row", [U], [U, z(4), U, z(5), U], ("overlap", "fit", "local"),
                 dict(overlap=ends, local=ends, fit=[9, 22, 36]))


def overlap_column_input(name="overlap-column", between=4):
    """A = u y u y u, B = u: three tied ends on column m, the last one A's end."""
    ends = [(9, 9), (18 + between, 9), (28 + 2 * between, 9)]
    modes = ("overlap", "local") if name == "overlap-column" else ("overlap",)
    return Input(name, [U, y(between), U, y(between + 1), U], [U], modes, dict(overlap=ends, local=ends))


def fit_far_input():
    """A = u, B = z(3) u z(55) u z(4) u z(6): E ties at j = 12, 76, 89.  A scan whose lanes stride 64 over the columns meets
    12 and 76 in one lane and 89 in another."""
    return Input("fit-far", [U], [z(3), U, z(55), U, z(4), U, z(6)], ("fit",), dict(fit=[12, 76, 89]))


def nothing_input():
    """Nothing aligns: LOCAL 0 at the origin with every cell tied, OVERLAP 0 on (0, m) tied with (n, 0), FIT's profile
    constant (every residue of A gapped)."""
    n, m = 7, 12
    return Input("nothing", [y(n)], [z(m)], MODES,
                 dict(local=[(i, j) for i in range(n + 1) for j in range(m + 1)], overlap=[(0, m), (n, 0)], fit=list(range(m + 1))))


BASE = {i.name: i for i in (row_input(), column_input(), cross_input(), overlap_row_input(), overlap_column_input(),
                            fit_far_input(), nothing_input())}
SHIFTS = (0, 1, 2, 5)
#: LOCAL costs W^2 n^2 m^2 / 4 band cells per expectation: max_shift 5 runs the one-layer recurrence only
LOCAL_AFFINE_SHIFTS = (0, 1, 2)
#: the bands whose strips are taller than the base inputs' distances; at max_shift 5 (four rows a strip) the base inputs do
TALL_SHIFTS = (0, 1, 2)
BETA_POSITIVE = ("row", "fit-far", "cross", "tall-cross-s1", "nothing")


@functools.lru_cache(maxsize=None)
def tall(s):
    """(a) The tall variants of one band: A's spacers as long as a strip, so that row's tied row lies below the first strip
    and the tied rows of the others lie in different strips."""
    rr = rows_per_strip(s)
    return {i.name: i for i in (row_input(f"tall-row-s{s}", lead=rr + 1), column_input(f"tall-column-s{s}", between=rr),
                                cross_input(f"tall-cross-s{s}", between=rr),
                                overlap_column_input(f"tall-overlap-column-s{s}", between=rr))}


def inputs_of(mode, cost, s):
    """The inputs of test_full_storage / test_score_only[mode, cost, s]."""
    out = [i for i in BASE.values() if mode in i.modes]
    if s in TALL_SHIFTS:
        out += [i for i in tall(s).values() if mode in i.modes]
    if cost == "beta>0":             # (where a gap opening is rewarded, only these keep several best ends: the oracle's word)
        out = [i for i in out if i.name in BETA_POSITIVE]
    if mode == "local" and s == 5:   # (the budget: the three inputs LOCAL is named for)
        out = [i for i in out if i.name in ("row", "column", "cross", "nothing")]
    return out


def main_cases():
    """[(mode, cost, s)]: both recurrences in every band the budget allows, and a rewarded gap opening for FIT and OVERLAP
    at max_shift 1 (LOCAL refuses it)."""
    out = []
    for mode in MODES:
        for cost in ("affine", "one-layer"):
            out += [(mode, cost, s) for s in SHIFTS if not (mode == "local" and cost == "affine" and s not in LOCAL_AFFINE_SHIFTS)]
        if mode != "local":
            out.append((mode, "beta>0", 1))
    return out


# ---- (b) the team shape at max_shift 1 ---------------------------------------------------------------------------------------

TEAM_GEO = Geometry(1, *TEAM_SHAPE)
TEAM_ROW_ENDS = [37, 150, 278]      # a boundary step ahead of the interior run, an interior step, column m
TEAM_COLUMN_ENDS = [11, 51, 83]     # strips 0, 2, 4: waves 0, 2 and 1 of a team of three


def row_n_step(j, geo=TEAM_GEO):
    """Where the sweep stores the end cell (n, j, n, j): -> "before" / "interior" / "after" the interior run of its step
    strip (pack_boundary.Geometry.place / interior: the steps that may store packed records)."""
    _, _, qs, c = geo.place(geo.n, j, geo.S)
    if geo.interior(qs, c):
        return "interior"
    return "before" if c < geo.LO and qs == geo.n // geo.RR else "after"


def team_inputs():
    """101 x 278.  A = y(92) u, and B holds three copies that end in the three step classes of row n.  FIT: exact copies (A's
    spacer is gapped for each alike).  OVERLAP: the first copy is reached from (92, 0) through a gap of 28 in B, the others
    from (0, j0) through the gap of 92 in A -- 64 residues more, eight structure mismatches in the first copy.  OVERLAP on
    column m: B = z(269) u, A's copies end in the strips of three different waves; they are reached through gaps of 2, 42
    and 74 residues of A: nine and four mismatches."""
    n, m = TEAM_SHAPE
    lead = [28, 104, 119]
    fit = Input("team-fit", [y(n - UNIT_LEN), U], [z(lead[0]), U, z(lead[1]), U, z(lead[2]), U], ("fit",), dict(fit=TEAM_ROW_ENDS))
    row = Input("team-overlap-row", [y(n - UNIT_LEN), U], [z(lead[0]), worn(U, 8), z(lead[1]), U, z(lead[2]), U], ("overlap",),
                dict(overlap=[(n, j) for j in TEAM_ROW_ENDS]))
    col = Input("team-overlap-column", [y(2), worn(U, 9), y(31), worn(U, 4), y(23), U, y(n - 83)], [z(m - UNIT_LEN), U], ("overlap",),
                dict(overlap=[(i, m) for i in TEAM_COLUMN_ENDS]))
    return {i.name: i for i in (fit, row, col)}


TEAM = team_inputs()

# ---- (c) LOCAL at the team shape of max_shift 2 --------------------------------------------------------------------------------

LOCAL_TEAM_SHIFT, LOCAL_TEAM_SIZES = 2, (1, 4)
LOCAL_TEAM_ENDS = [(20, 120), (20, 200), (42, 50)]   # rows in strips 1 and 3 of ten: waves 1 and 3 of a team of four


def local_team_input(short=False):
    """A = y u y v y, B = z v z u z u z: three tied ends -- two columns in one row, and a second row in the strip of another
    wave.  v precedes the u's in B and follows u in A, so no alignment takes two whole units; the spacers between units
    cost more than the few residues of v that pair with residues of u would add.
    ``short``: the cut-down twin, the same layout with spacers of 2 and 10 -- where local_expected is affordable."""
    if short:
        return Input("local-team-short", [y(2), U, y(10), V, y(2)], [z(2), V, z(10), U, z(10), U, z(2)], ("local",),
                     dict(local=[(11, 30), (11, 49), (30, 11)]))
    n, m = TEAM_SHAPE
    return Input("local-team", [y(11), U, y(13), V, y(n - 42)], [z(41), V, z(61), U, z(71), U, z(m - 200)], ("local",),
                 dict(local=LOCAL_TEAM_ENDS))


LOCAL_TEAM, LOCAL_TEAM_SHORT = local_team_input(), local_team_input(short=True)

# ---- (d) the hit search's mask ---------------------------------------------------------------------------------------------------

MASK_SPANS = [(23, 63), (95, 135), (158, 198)]   # an end with j % 32 == 31; (start + 1) % 32 == 0; bits 159..198: three words
MASK = Input("hits-mask", [LONG], [z(23), LONG, z(32), LONG, z(23), LONG, z(7)], ("fit",), dict(fit=[e for _, e in MASK_SPANS]))
FAR_SPANS = [(3, 12), (67, 76), (80, 89)]


def hit_spec(inp):
    """(max_hits, max_walks, min_score): min_score 1, so that nearly every end is a candidate; room for a walk from every
    end."""
    return 8, inp.m + 1, 1


def mask_words(span):
    """The mask words an accepted span [start, end) sets bits in: start + 1 .. end."""
    return sorted({x >> 5 for x in range(min(span[0] + 1, span[1]), span[1] + 1)})


# ---- (e) dense forms -----------------------------------------------------------------------------------------------------------

DENSE = [BASE[name] for name in ("row", "column", "cross", "fit-far")]


def dense_kw(inp, params):
    """The pair's own LOOKUP tables as dense mu1 and mu2."""
    mu1, mu2 = tables_of(inp.pair, params)
    return dict(mu1_dense=[np.ascontiguousarray(mu1[1:, 1:], dtype=np.int32)], mu2_dense=[np.ascontiguousarray(mu2[1:, 1:], dtype=np.int32)])


# ---- (f) scaled twins ----------------------------------------------------------------------------------------------------------

class Twin:
    """An input in LOOKUP form without a similarity matrix, every score multiplied by k (window_edge.Problem.at); ``k``: the
    largest scale the int32 safety window admits.  Scaling keeps ties exactly."""

    def __init__(self, inp, costs="affine", s=1):
        self.inp, self.costs, self.s = inp, costs, s
        self.name = f"{inp.name}-{costs}"
        self.pair, self.n, self.m, self.modes = inp.pair, inp.n, inp.m, inp.modes

    def __repr__(self):
        return self.name

    def at(self, k):
        beta, gamma, delta = we.COSTS[self.costs]
        return dict(synth.PROTEIN_PARAMS, simmatrix=None, max_shift=self.s, sequence_match_similarity=100 * k,
                    sequence_mismatch_similarity=-30 * k, structure_weight=800 * k, gap_opening_cost=beta * k, gap_cost=gamma * k,
                    shift_cost=delta * k)

    def product(self, k):
        p = self.at(k)
        amax = max(abs(p["sequence_match_similarity"]), abs(p["sequence_mismatch_similarity"]))
        return we.window(self.n, self.m, amax, abs(p["structure_weight"]), p["gap_opening_cost"], p["gap_cost"], p["shift_cost"])[1]

    @functools.cached_property
    def k(self):
        return we.edge_scale(self.product)


TWINS = {t.name: t for t in [Twin(BASE[name], costs) for name in ("row", "cross", "fit-far", "nothing") for costs in ("affine", "linear")]}


# ---- expectations ------------------------------------------------------------------------------------------------------------

def case_of(pair, params, want_layers=False):
    return len(pair[0]), len(pair[1]), params, *tables_of(pair, params), want_layers


def expected(cases, procs=None):
    """``cases``: {(mode, ...): (n, m, params, mu1, mu2, want_layers)} -> {key: the mode's expectation}; one spawn pool per
    mode."""
    out = {}
    for mode in MODES:
        part = {key: c for key, c in cases.items() if key[0] == mode}
        if part:
            out.update(EXPECT[mode].expected_many(part, procs))
    return out


def estimate(cases):
    """{mode: core-seconds} of ``expected(cases)`` by the splitters' cost model (free_ends_expected.cell_seconds)."""
    out = dict.fromkeys(MODES, 0.0)
    for (mode, *_), (n, m, params, *_) in cases.items():
        runs = {"fit": n * m * m / 2, "overlap": n * m * (n + m) / 2, "local": n * n * m * m / 4}[mode]
        out[mode] += runs * cell_seconds(params)
    return out


def tied(mode, want, n, m):
    """Every end that attains the expectation's score, in the order of the rule: FIT columns, else (i, j)."""
    if mode == "fit":
        return [int(j) for j in np.flatnonzero(he.profile(want["glob"]) == want["score"])]
    if mode == "local":
        return [(int(i), int(j)) for i, j in np.argwhere(want["ends"] == want["score"])]
    ei, ej = oe.end_cells(n, m)
    return [(int(ei[x]), int(ej[x])) for x in np.flatnonzero(want["ends"][ei, ej] == want["score"])]


def end_of(mode, want):
    return want["end_b"] if mode == "fit" else want["end"]


def magnitude(want):
    """The largest finite |value| of the expectation's layers."""
    lay = want["layers"]
    return int(np.abs(lay[(lay != NONE) & (lay > LOW)]).max())


def main_case_table(modes=MODES):
    """The cases of test_full_storage / test_score_only: {(mode, "main", input name, cost, s): case}."""
    cases = {}
    for mode, cost, s in main_cases():
        if mode in modes:
            prm = params_of("protein", cost, s)
            for inp in inputs_of(mode, cost, s):
                cases[(mode, "main", inp.name, cost, s)] = case_of(inp.pair, prm)
    return cases


def team_case_table():
    """(b): the three pairs of the team shape, both recurrences at max_shift 1; (d): the mask input."""
    cases = {}
    for inp in TEAM.values():
        for cost in ("affine", "one-layer"):
            cases[(inp.modes[0], "team", inp.name, cost, 1)] = case_of(inp.pair, params_of("protein", cost, 1))
    for cost in ("affine", "one-layer"):
        cases[("fit", "mask", MASK.name, cost, 1)] = case_of(MASK.pair, params_of("protein", cost, 1))
    return cases


def local_team_case_table():
    """(c): the cut-down twin (the pair itself is out of local_expected's reach)."""
    return {("local", "team-short", LOCAL_TEAM_SHORT.name, cost, LOCAL_TEAM_SHIFT):
            case_of(LOCAL_TEAM_SHORT.pair, params_of("protein", cost, LOCAL_TEAM_SHIFT)) for cost in ("affine", "one-layer")}


def twin_case_table(scales=("k",), want_layers=False):
    """(f): {(mode, "twin", twin name, scale): case} with scale "k" (the edge) or 1."""
    cases = {}
    for t in TWINS.values():
        for mode in t.modes:
            for scale in scales:
                cases[(mode, "twin", t.name, scale)] = case_of(t.pair, t.at(t.k if scale == "k" else scale), want_layers)
    return cases


def self_score(u, params):
    """The global score of a unit against itself: one oracle run."""
    from oracle import oracle
    return oracle.solve(u[0], u[0], u[1], u[1], params)["score"]


# ---- what the oracle says of the twins (test_tied_ends_host.py prints and re-asserts it) ------------------------------------------

#: twin -> (scale k, {mode: largest finite magnitude of the mode's expected layers at scale k})
MEASURED = {
    "row-affine": (1421, dict(local=11510100, fit=11424840)),        # 2^23.46, 2^23.45
    "row-linear": (1749, dict(local=14166900, fit=14061960)),        # 2^23.76, 2^23.75
    "cross-affine": (1711, dict(local=13859100, overlap=13859100)),  # 2^23.72
    "cross-linear": (2107, dict(local=17066700, overlap=17066700)),  # 2^24.02
    "fit-far-affine": (776, dict(fit=6285600)),                      # 2^22.58
    "fit-far-linear": (955, dict(fit=7735500)),                      # 2^22.88
    "nothing-affine": (3647, dict(fit=7221060, overlap=4959920, local=4741100)),   # 2^22.78, 2^22.24, 2^22.18
    "nothing-linear": (4488, dict(fit=4173840, overlap=2603040, local=1795200)),   # 2^21.99, 2^21.31, 2^20.78
}

#: core-seconds of the oracle runs: the splitters' model (``estimate``) and what a pool of 16 took
BUDGET = """
test_tied_ends_host.py  188 expectations (the twins at scale 1 and k, with layers): model fit 96 + overlap 181 + local 86 = 363
                        core-seconds; measured 245 core-seconds, 32 s of wall time.
test_gpu_tied_ends.py   170 expectations (the twins at scale k only, no layers, no cut-down LOCAL twin): model 95 + 181 + 54 =
                        330; measured 241 core-seconds, 32 s of wall time.
Of the model's figure 218 core-seconds are the three affine expectations of the 101 x 278 team shape (FIT 58, OVERLAP twice 80),
which (b) cannot do without: an OVERLAP expectation takes n + m + 1 oracle fills of the whole pair.  LOCAL runs the affine
recurrence up to max_shift 2 and the one-layer one up to 5 (the base inputs alone there): affine at max_shift 5 would add 35.
"""
