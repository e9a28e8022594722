"""Problems at the admitted edge of the int32 safety window, and the test-side mirror of the check that admits them.
Shared by test_window_edge_host.py (no GPU: every case is what it claims to be, from the oracle alone) and
test_gpu_window_edge.py (every DP path, bit-exact against the oracle, at that scale).

The contract (bialign_plan.hpp, score_bound and plan_pairs, "int32 safety window"): a batch is refused unless every pair has
    (2 (n + m) + 8) * colmax < 2^28,   colmax = max|mu1| + max|mu2| + 2 (|gamma| + |beta|) + 2 |delta|
with the maxima taken over the S1 / S2 tables (LOOKUP form), the dense tables, or -- FEATURE form --
ceil(|sw| (sqrt(max upA max upB) + sqrt(max downA max downB) + sqrt(max unpA max unpB))).  The kernels then assume that
finite values and drifting "-infinity" cells (NEG = -2^30 plus whatever a path adds) stay 2^28 away from each other
and from THRESH / SENT (bialign_types.hpp).

A Problem is an input at scale 1 -- a seeded pair, a cost pattern, a form -- and ``at(k)`` multiplies every score of
it (mu1, mu2, beta, gamma, delta) by k.  ``Problem.k`` is the largest k the mirror admits.  In the oracle scaling is
exact (score_k == k * score_1, equal traces), so the cases keep the tie structure of the ones the suite trusts at
scale 1.

MEASURED WITH THE ORACLE (test_window_edge_host.py prints and re-asserts them; ``-s`` shows the table).  "finite" is the
largest |value| of an in-band cell of the finite class, "drift" the largest |value - NEG| of the "-infinity" class;
no in-band value of any case lies in [NEG + 2^28, -2^28].  Admitted inputs reach finite magnitudes of 2^23 .. 2^26.4,
10 - 100 x beyond the rest of the suite, and do NOT reach THRESH: the product bounds a path no input can realise
(every column paying both maxima and every cost at once).

Per case: ``MEASURED`` at the end of this module (scale, magnitude, drift; asserted against the oracle by the host test).
In short, at scale k (n, m, max_shift as in the case lists below):
    LOOKUP protein, affine costs (-150 / -50 / -150)   finite 2^23.3 .. 2^24.0   drift <= 3.3e6  (1.2 % of 2^28, s = 8)
    LOOKUP protein, linear (beta = 0)                  finite 2^24.0 .. 2^24.5   no "-infinity" class (one layer)
    LOOKUP protein, all costs positive (100 / 30 / 40) finite 2^25.1 .. 2^25.6   drift <= 1.44e7 (5.4 %, s = 8), upwards
    dense mu1 / mu2 / both (BLOSUM62 where mu1 is dense) finite 2^23.4 .. 2^23.9 drift <= 8.0e5
    FEATURE form                                       finite 2^23.2 .. 2^23.7   drift <= 5.3e5
    RNA LOOKUP (55, 50, s2)                            finite 2^24.0             drift 7.7e5
    constant tables, all five numbers +100 k (20,24,s1) finite 0.336 * 2^28 = 2^26.4   drift 1.2 % of 2^28
    constant tables, all five numbers -100 k (20,24,s1) finite 0.076 * 2^28 = 2^24.3   drift 0.5 % of 2^28
The short members of the ragged batch run at the scale of its longest pair (100, 100) and stay below 2^23; the batch
as a whole reaches 2^23.8.
"""
import functools
import math

import numpy as np

NEG = -(1 << 30)
WINDOW = 1 << 28
INT64_MAX = (1 << 63) - 1

#: beta, gamma, delta at scale 1
COSTS = {
    "affine": (-150, -50, -150),      # synth.PROTEIN_PARAMS
    "linear": (0, -50, -150),         # the one-layer recurrence
    "positive": (100, 30, 40),        # every cost a gain: beta > 0 kernels, "-infinity" cells drift upwards
}
#: the two constant-table extremes: mu1 and mu2 the same everywhere, and (mu1, mu2, beta, gamma, delta) all equal -- the
#: input that realises most of the bound (all positive: every one of the 2 (n + m) single steps gains beta + gamma +
#: delta = 3/8 of colmax)
CONSTANT = {
    "const-positive": (100, 100, 100, 100, 100),
    "const-negative": (-100, -100, -100, -100, -100),
}
KEYS = ("up", "down", "unp")


# ---- the mirror ----------------------------------------------------------------------------------------------------

def window(n, m, amax, bmax, beta, gamma, delta):
    """-> (colmax, product): bialign_plan.hpp: score_bound's ``colmax`` and the left side of plan_pairs' per-pair check
    (tests/test_plan_host.py holds this mirror against that code)."""
    colmax = int(amax) + int(bmax) + 2 * (abs(int(gamma)) + abs(int(beta))) + 2 * abs(int(delta))
    return colmax, (2 * (int(n) + int(m)) + 8) * colmax


def feature_bound(sw, feats_a, feats_b):
    """FEATURE form: the host's bound on |mu2| from the molecules' largest features, in the same double operations."""
    total = sum(math.sqrt(float(np.max(fa)) * float(np.max(fb))) for fa, fb in zip(feats_a, feats_b))
    return int(math.ceil(abs(float(sw)) * total))


def edge_scale(product_of):
    """The largest integer k with product_of(k) < 2^28 <= product_of(k + 1); product_of must not decrease."""
    assert product_of(1) < WINDOW, "the problem does not fit the window at scale 1"
    hi = 2
    while product_of(hi) < WINDOW:
        hi *= 2
    lo = hi // 2                      # product_of(lo) < 2^28 <= product_of(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if product_of(mid) < WINDOW else (lo, mid)
    assert product_of(lo) < WINDOW <= product_of(lo + 1)
    return lo


def sumsq_max_replicas(bound):
    """Null batches: the most replicas whose sum of squares the host admits, replicas * bound^2 <= INT64_MAX."""
    return INT64_MAX // (bound * bound)


@functools.lru_cache(maxsize=None)
def band_index(n, m, s):
    i, j, a, b = np.meshgrid(np.arange(n + 1), np.arange(m + 1), np.arange(2 * s + 1), np.arange(2 * s + 1), indexing="ij")
    k, l = i + a - s, j + b - s
    return (k >= 0) & (k <= n) & (l >= 0) & (l <= m)


def classes(layers, n, m, s):
    """In-band oracle values split at -2^29 into the finite class and the "-infinity" class -> dict(finite, inf: int64
    arrays; magnitude: largest |finite value|; drift: largest |value - NEG| of the other class (0 if it is empty);
    between: how many values lie in [NEG + 2^28, -2^28], where neither class may be)."""
    band = band_index(n, m, s)
    vals = np.concatenate([np.asarray(lay, dtype=np.int64)[band] for lay in layers])
    inf = vals[vals < -(1 << 29)]
    finite = vals[vals >= -(1 << 29)]
    return dict(finite=finite, inf=inf, magnitude=int(np.abs(finite).max()),
                drift=int(np.abs(inf - NEG).max()) if inf.size else 0,
                between=int(((vals >= NEG + WINDOW) & (vals <= -WINDOW)).sum()))


# ---- problems ------------------------------------------------------------------------------------------------------

def fractional(seed, n):
    """(up, down, unp) of test_gpu_mu2_features: a probability split per residue, some entries exactly 0 or 1."""
    rng = np.random.default_rng(seed)
    raw = rng.dirichlet([0.6, 0.6, 0.9], size=n)
    kind = rng.integers(0, 6, size=n)
    up, down = raw[:, 0].copy(), raw[:, 1].copy()
    up[kind == 0] = 0.0
    down[kind == 1] = 0.0
    up[kind == 2], down[kind == 2] = 0.0, 0.0
    return up, down, 1.0 - up - down


def host_table(fa, fb, sw):
    """The (n, m) mu2 table of two feature triples as test_gpu_mu2_features builds it on the host."""
    from bialign_amd.scoring import dense_mu2_from_features
    one_based = lambda f: {k: np.concatenate([[0.0], np.asarray(v, dtype=np.float64)]) for k, v in zip(KEYS, f)}  # noqa: E731
    return dense_mu2_from_features(one_based(fa), one_based(fb), sw)


class Problem:
    """One input.  ``form``: "lookup" (protein, simmatrix None), "rna" (RNA LOOKUP: mu2 = int(sw * ...) of 0/1 features),
    "mu1" / "mu2" / "mu12" (dense tables = the oracle's mu_tables at scale 1 times k; mu1 from BLOSUM62 where it is dense),
    "feature" (RNA letters, fractional features, the GPU builds mu2).  ``costs``: a key of COSTS or of CONSTANT."""

    def __init__(self, form, n, m, s, seed, costs="affine"):
        self.form, self.n, self.m, self.s, self.seed, self.costs = form, n, m, s, seed, costs
        self.name = f"{form}-{n}x{m}-s{s}-{costs}"

    def __repr__(self):
        return self.name

    # -- the input at scale 1
    @functools.cached_property
    def pair(self):
        from bialign_amd import synth
        n, m = self.n, self.m
        if self.costs in CONSTANT:
            return "A" * n, "A" * m, "H" * n, "H" * m
        if self.form == "rna":
            return synth.rna_pair(self.seed, n, m)
        if self.form == "feature":
            draw = lambda sd, ln: "".join(np.random.default_rng(sd).choice(list("ACGU"), size=ln))  # noqa: E731
            return draw(self.seed, n), draw(self.seed + 500, m), "." * n, "." * m
        return synth.protein_pair(self.seed, n, m)

    @functools.cached_property
    def features(self):
        return fractional(self.seed * 2, self.n), fractional(self.seed * 2 + 1, self.m)

    def at(self, k):
        """The parameter dict at scale k (LOOKUP forms: all the engine sees of the scores)."""
        from bialign_amd import synth
        if self.costs in CONSTANT:
            match, sw, beta, gamma, delta = CONSTANT[self.costs]
        else:
            match, sw = 100, (400 if self.form in ("rna", "feature") else 800)
            beta, gamma, delta = COSTS[self.costs]
        base = synth.RNA_PARAMS if self.form in ("rna", "feature") else synth.PROTEIN_PARAMS
        return dict(base, simmatrix="BLOSUM62" if self.form in ("mu1", "mu12") else None, max_shift=self.s,
                    sequence_match_similarity=match * k, sequence_mismatch_similarity=-30 * k, structure_weight=sw * k,
                    gap_opening_cost=beta * k, gap_cost=gamma * k, shift_cost=delta * k)

    @functools.lru_cache(maxsize=None)
    def tables(self, k):
        """(n+1) x (m+1) int64 mu1, mu2 at scale k as the engine is to see them, in the oracle's layout."""
        from oracle import oracle
        if self.form in ("mu1", "mu2", "mu12"):     # dense: k times the oracle's tables of scale 1 (BLOSUM62 is not scaled by at())
            mu1, mu2 = oracle.mu_tables(*self.pair, self.at(1))
            return mu1.astype(np.int64) * k, mu2.astype(np.int64) * k
        mu1, mu2 = oracle.mu_tables(*self.pair, self.at(k))
        if self.form == "feature":
            mu2 = np.zeros_like(mu2)
            mu2[1:, 1:] = host_table(*self.features, self.at(k)["structure_weight"])
        return mu1.astype(np.int64), mu2.astype(np.int64)

    def maxima(self, k):
        """(max |mu1|, max |mu2|) as the host takes them for this form."""
        p = self.at(k)
        mu1, mu2 = self.tables(k)
        letters = len(set(self.pair[0] + self.pair[1]))
        # LOOKUP: the whole S1 / S2 table, whether or not a pair of letters occurs
        amax = max(abs(p["sequence_match_similarity"]), abs(p["sequence_mismatch_similarity"]) if letters > 1 else 0)
        bmax = abs(p["structure_weight"])
        if self.form in ("mu1", "mu12"):
            amax = int(np.abs(mu1[1:, 1:]).max())
        if self.form in ("mu2", "mu12"):
            bmax = int(np.abs(mu2[1:, 1:]).max())
        if self.form == "feature":
            bmax = feature_bound(p["structure_weight"], *self.features)
        return amax, bmax

    def window(self, k, n=None, m=None):
        p = self.at(k)
        return window(self.n if n is None else n, self.m if m is None else m, *self.maxima(k), p["gap_opening_cost"],
                      p["gap_cost"], p["shift_cost"])

    def product(self, k):
        return self.window(k)[1]

    @functools.cached_property
    def k(self):
        return edge_scale(self.product)

    @functools.lru_cache(maxsize=None)
    def reference(self, k=None):
        """Oracle solve at scale k (default: the edge) -> score, layers, trace (as lists), complete, classes."""
        from oracle import oracle
        k = self.k if k is None else k
        mu1, mu2 = self.tables(k)
        assert max(np.abs(mu1).max(), np.abs(mu2).max()) < 2 ** 31
        ref = oracle.solve_tables(self.n, self.m, self.at(k), mu1, mu2)
        ref["trace"] = oracle.trace_to_lists(ref["trace"])
        ref["classes"] = classes(ref["layers"], self.n, self.m, self.s)
        return ref

    def replica_score(self, k, seed, pair_index, replica):
        """Oracle score of one replica of a null batch: B's residues, and with them the columns of both tables, permuted."""
        from oracle import oracle
        from bialign_amd import significance as sg
        mu1, mu2 = self.tables(k)
        cols = np.concatenate([[0], 1 + sg.permutation(seed, pair_index, replica, self.m)])
        return oracle.solve_tables(self.n, self.m, self.at(k), mu1[:, cols], mu2[:, cols], want_trace=False)["score"]

    # -- the engine's batch of this one problem, in its form
    def make_batch(self, k=None, **kw):
        return make_batch([self], k, **kw)

    def null_batch(self, replicas, seed, k=None):
        from bialign_amd import significance as sg
        k = self.k if k is None else k
        if self.form == "feature":
            return sg.null_feature_batch(*self._molecules(), self.at(k), replicas, seed=seed)
        if self.form in ("mu1", "mu2", "mu12"):
            return sg.null_dense_batch([self.pair], self.at(k), replicas, seed=seed, **_dense_kw([self], k))
        return sg.null_batch([self.pair], self.at(k), replicas, seed=seed)

    def _molecules(self):
        fa, fb = self.features
        return [(self.pair[0], fa), (self.pair[1], fb)], [(0, 1)]


def _dense_kw(problems, k):
    kw = {}
    if problems[0].form in ("mu1", "mu12"):
        kw["mu1_dense"] = [p.tables(k)[0][1:, 1:] for p in problems]
    if problems[0].form in ("mu2", "mu12"):
        kw["mu2_dense"] = [p.tables(k)[1][1:, 1:] for p in problems]
    return kw


def batch_scale(problems):
    """The edge of a batch: one colmax for all its pairs, so the pair with the largest n + m sets the scale."""
    return min(p.k for p in problems)


def make_batch(problems, k=None, **kw):
    """One engine batch of several problems of one form, cost pattern and max_shift, all at scale k (default: the
    batch's edge)."""
    from bialign_amd.batch import make_batch as mb, make_feature_batch
    first = problems[0]
    assert all((p.form, p.costs, p.s) == (first.form, first.costs, first.s) for p in problems)
    k = batch_scale(problems) if k is None else k
    if first.form == "feature":
        assert len(problems) == 1
        return make_feature_batch(*first._molecules(), first.at(k), **kw)
    return mb([p.pair for p in problems], first.at(k), **_dense_kw(problems, k), **kw)


# ---- the cases the GPU tests use (test_window_edge_host.py checks every one of them) -----------------------------------

#: 1. tiled full layers: the shapes of test_gpu_parity.test_full_layers_vs_oracle's plans, three cost patterns each
TILED = [Problem("lookup", n, m, s, seed, costs) for n, m, s, seed in
         [(20, 24, 1, 1), (61, 64, 3, 8), (40, 50, 4, 10), (33, 45, 5, 11), (200, 200, 0, 7)]
         for costs in ("affine", "linear", "positive")]
EXTREMES = [Problem("lookup", 20, 24, 1, 0, "const-positive"), Problem("lookup", 20, 24, 1, 0, "const-negative")]
#: 2. teams and kernel variants.  s = 1: P = 282 admits teams of up to three, six strips; P = 402 and nine strips a team of four
TEAM_S1 = Problem("lookup", 110, 280, 1, 2)
TEAM4_S1 = Problem("lookup", 170, 400, 1, 25)
EIGHT_WAVE_S2 = Problem("lookup", 180, 440, 2, 51)
#: 3. reduced storage: several strips at s = 1 (slim sweep in teams of three), s = 2, s = 4; the ragged batch
REDUCED = [TEAM_S1, Problem("lookup", 75, 130, 2, 6), Problem("lookup", 60, 50, 4, 10), Problem("lookup", 110, 280, 1, 2, "linear"),
           Problem("lookup", 75, 130, 2, 6, "positive")]
RAGGED = [Problem("lookup", n, m, 1, 100 + t) for t, (n, m) in enumerate([(40, 33), (5, 90), (90, 5), (64, 64), (1, 1),
                                                                       (17, 18), (100, 100), (2, 50)])]
#: 4. wide band
WIDE = [Problem("lookup", 23, 31, 6, 5023), Problem("lookup", 40, 17, 8, 5040), Problem("lookup", 23, 31, 6, 5023, "linear"),
        Problem("lookup", 40, 17, 8, 5040, "positive")]
#: 5. forms
FORMS = [Problem("mu1", 61, 64, 1, 8), Problem("mu2", 61, 64, 2, 8), Problem("mu12", 61, 64, 3, 8),
         Problem("mu12", 40, 50, 1, 10, "linear"), Problem("feature", 61, 50, 2, 3), Problem("feature", 40, 45, 1, 4, "linear"),
         Problem("rna", 55, 50, 2, 2)]
DROPIN = Problem("lookup", 33, 29, 2, 12)
#: 6. both sides of the check through the C ABI: one per form
BOTH_SIDES = [TILED[0], FORMS[0], FORMS[1], FORMS[4]]
#: 7. null batches
NULL = [Problem("lookup", 30, 21, 1, 4700), Problem("feature", 24, 27, 1, 9), Problem("mu12", 25, 22, 1, 4702),
        Problem("lookup", 30, 21, 1, 4700, "linear")]

CASES = {}
for _p in (TILED + EXTREMES + [TEAM_S1, TEAM4_S1, EIGHT_WAVE_S2] + REDUCED + RAGGED + WIDE + FORMS + [DROPIN] + BOTH_SIDES
           + NULL):
    CASES.setdefault(_p.name, _p)

#: name -> (scale k, largest finite magnitude, largest drift of a "-infinity" cell from NEG), from the oracle at scale k;
#: the comment gives log2 of the magnitude and the drift in percent of 2^28.  Ragged-batch members at the batch's scale.
MEASURED = {
    "lookup-20x24-s1-affine": (1747, 13451900, 873500),               # 2^23.68, 0.33 %
    "lookup-20x24-s1-linear": (2150, 20016500, 0),                    # 2^24.25, 0.00 %
    "lookup-20x24-s1-positive": (2255, 48662900, 2367750),            # 2^25.54, 0.88 %
    "lookup-61x64-s3-affine": (650, 15177500, 975000),                # 2^23.86, 0.36 %
    "lookup-61x64-s3-linear": (800, 20944000, 0),                     # 2^24.32, 0.00 %
    "lookup-61x64-s3-positive": (839, 51380360, 2642850),             # 2^25.61, 0.98 %
    "lookup-40x50-s4-affine": (892, 13603000, 1471800),               # 2^23.70, 0.55 %
    "lookup-40x50-s4-linear": (1098, 19632240, 0),                    # 2^24.23, 0.00 %
    "lookup-40x50-s4-positive": (1151, 49147700, 4834200),            # 2^25.55, 1.80 %
    "lookup-33x45-s5-affine": (1023, 14874420, 1739100),              # 2^23.83, 0.65 %
    "lookup-33x45-s5-linear": (1259, 20194360, 0),                    # 2^24.27, 0.00 %
    "lookup-33x45-s5-positive": (1320, 48708000, 6085200),            # 2^25.54, 2.27 %
    "lookup-200x200-s0-affine": (207, 16731810, 0),                   # 2^24.00, 0.00 %
    "lookup-200x200-s0-linear": (255, 23722650, 0),                   # 2^24.50, 0.00 %
    "lookup-200x200-s0-positive": (267, 36069030, 0),                 # 2^25.10, 0.00 %
    "lookup-20x24-s1-const-positive": (3495, 90171000, 3145500),      # 2^26.43, 1.17 %
    "lookup-20x24-s1-const-negative": (3495, 20271000, 1398000),      # 2^24.27, 0.52 %
    "lookup-110x280-s1-affine": (212, 11369560, 106000),              # 2^23.44, 0.04 %
    "lookup-170x400-s1-affine": (146, 11563200, 73000),               # 2^23.46, 0.03 %
    "lookup-180x440-s2-affine": (134, 11628520, 134000),              # 2^23.47, 0.05 %
    "lookup-75x130-s2-affine": (401, 12519220, 401000),               # 2^23.58, 0.15 %
    "lookup-60x50-s4-affine": (735, 16023000, 1102500),               # 2^23.93, 0.41 %
    "lookup-110x280-s1-linear": (262, 16964500, 0),                   # 2^24.02, 0.00 %
    "lookup-75x130-s2-positive": (517, 47119380, 1085700),            # 2^25.49, 0.40 %
    "lookup-40x33-s1-affine": (411, 4738830, 205500),                 # 2^22.18, 0.08 %
    "lookup-5x90-s1-affine": (411, 4225080, 205500),                  # 2^22.01, 0.08 %
    "lookup-90x5-s1-affine": (411, 4225080, 205500),                  # 2^22.01, 0.08 %
    "lookup-64x64-s1-affine": (411, 11162760, 205500),                # 2^23.41, 0.08 %
    "lookup-1x1-s1-affine": (411, 452100, 135630),                    # 2^18.79, 0.05 %
    "lookup-17x18-s1-affine": (411, 2749590, 205500),                 # 2^21.39, 0.08 %
    "lookup-100x100-s1-affine": (411, 14648040, 205500),              # 2^23.80, 0.08 %
    "lookup-2x50-s1-affine": (411, 2539980, 205500),                  # 2^21.28, 0.08 %
    "lookup-23x31-s6-affine": (1446, 13737000, 2385900),              # 2^23.71, 0.89 %
    "lookup-40x17-s8-affine": (1375, 10408750, 3300000),              # 2^23.31, 1.23 %
    "lookup-23x31-s6-linear": (1780, 19633400, 0),                    # 2^24.23, 0.00 %
    "lookup-40x17-s8-positive": (1774, 42717920, 14369400),           # 2^25.35, 5.35 %
    "mu1-61x64-s1-affine": (400, 11420000, 280000),                   # 2^23.45, 0.10 %
    "mu2-61x64-s2-affine": (650, 15177500, 650000),                   # 2^23.86, 0.24 %
    "mu12-61x64-s3-affine": (400, 11980000, 600000),                  # 2^23.51, 0.22 %
    "mu12-40x50-s1-linear": (679, 15481200, 0),                       # 2^23.88, 0.00 %
    "feature-61x50-s2-affine": (612, 9843269, 459000),                # 2^23.23, 0.17 %
    "feature-40x45-s1-linear": (984, 13412074, 0),                    # 2^23.68, 0.00 %
    "rna-55x50-s2-affine": (1026, 17308620, 769500),                  # 2^24.04, 0.29 %
    "lookup-33x29-s2-affine": (1271, 12964200, 1271000),              # 2^23.63, 0.47 %
    "lookup-30x21-s1-affine": (1525, 12062750, 762500),               # 2^23.52, 0.28 %
    "feature-24x27-s1-affine": (1313, 9406141, 525200),               # 2^23.17, 0.20 %
    "mu12-25x22-s1-affine": (1144, 12469600, 800800),                 # 2^23.57, 0.30 %
    "lookup-30x21-s1-linear": (1877, 17268400, 0),                    # 2^24.04, 0.00 %
}
