"""One table of cases that, between them, launch every instantiated sweep and walk once.

tests/variant_check.hip prints the instantiation plan from the predicates of bialign_host.hpp; ``CASES`` below holds, per
case, what a test needs to force one variant: recurrence, max_shift, form, storage, the sign of the gap opening cost, the
alignment mode, the environment switches, a shape.  ``keys(case)`` names the variants the case launches -- fill, re-sweep,
traceback -- in the words of the program's lines.  tests/test_variant_cases_host.py (CPU) holds the two together: the keys
of all cases are the instantiated variants, and the planner (tests/plan_check.hip) plans for every case what it claims.
tests/test_gpu_variants.py runs the cases against the oracle.

Shapes are the smallest that admit the team: n the first length with two strips per wave (strips of 64 // (2 s + 1) - 1
rows), m the first multiple of ten at which team_shape's period condition (T * lag + 64 <= P, P >= 256) holds for that n.
They were read off plan_check and are the same for both recurrences; the host test asks plan_check again.
"""
import collections
import functools
import types

import numpy as np

from bialign_amd import synth

SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE, LOCAL = 1, 2, 4, 64       # bialign_params.flags
STORAGE_FLAG = dict(full=0, score_only=SCORE_ONLY, lean_trace=LEAN_TRACE, level_trace=LEVEL_TRACE)
FORMS = ("lookup", "mu1", "mu2", "mu12")
LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
BETA_ANY = 60      # a gap opening cost > 0: the general-beta algebra
WIDE_S = 6         # the narrowest band of the wide path
SHIFTS = range(6)
#: the environment switches a case may set; a test clears the others of them
SWITCHES = ("BIALIGN_TEAM", "BIALIGN_SLIM", "BIALIGN_PACK", "BIALIGN_RESW_K", "BIALIGN_TRACE_FAST", "BIALIGN_TRACE_WINDOW",
            "BIALIGN_TRACE_WINDOW_K", "BIALIGN_WIDE_SEG", "BIALIGN_WIDE_PARTS")

# ---- shapes ------------------------------------------------------------------------------------------------------------
#: one wave per pair: three strips and a few rows, columns that are no multiple of a ghost block (max_shift 1: the fewest
#: columns at which decide_pack admits packed records)
ONE_WAVE = {0: (130, 37), 1: (45, 45), 2: (29, 41), 3: (21, 38), 4: (40, 50), 5: (33, 45)}
#: (team, max_shift) -> the smallest (n, m) whose plan has that team; "xN" takes the shape of N waves in a workgroup
TEAM_SHAPE = {
    ("2", 0): (190, 380), ("2", 1): (61, 260), ("2", 2): (34, 260), ("2", 3): (25, 260), ("2", 4): (19, 260), ("2", 5): (13, 260),
    ("3", 1): (101, 280), ("3", 4): (31, 260), ("3", 5): (21, 260),
    ("4", 0): (442, 700), ("4", 1): (141, 350), ("4", 2): (78, 260), ("4", 3): (57, 260), ("4", 4): (43, 260), ("4", 5): (29, 260),
    ("6", 1): (221, 500),
    ("8", 0): (946, 1330), ("8", 1): (301, 640), ("8", 2): (166, 430), ("8", 3): (121, 390), ("8", 4): (91, 350), ("8", 5): (61, 320),
    ("12", 1): (461, 930),
    ("h2", 2): (342, 800),
}
#: local alignments, one wave: two strips, nine columns (an expectation costs about W^2 n^2 m^2 / 4 oracle cells)
LOCAL_ONE = {0: (65, 9), 1: (22, 9), 2: (13, 9), 3: (10, 9), 4: (8, 9), 5: (6, 9)}
WIDE_SHAPE = (23, 31)

# ---- which teams the table forces, per recurrence: (BIALIGN_TEAM, the max_shifts, the forms) ---------------------------
AFFINE_TEAMS = [("1", SHIFTS, FORMS), ("2", range(4), FORMS), ("4", range(4), FORMS), ("8", range(3), ("lookup",)),
                ("x2", range(4), FORMS), ("x3", (4, 5), ("lookup",)), ("h2", (2,), ("lookup",))]
LINEAR_TEAMS = [("1", SHIFTS, FORMS), ("2", SHIFTS, FORMS), ("4", SHIFTS, ("lookup",)), ("8", SHIFTS, ("lookup",)),
                ("x2", SHIFTS, FORMS)]
AFFINE_LOCAL_TEAMS = [("1", SHIFTS, FORMS), ("4", range(4), FORMS)]
LINEAR_LOCAL_TEAMS = [("1", SHIFTS, FORMS), ("4", SHIFTS, ("lookup",))]
PACKED_SHIFTS, PACKED_FORMS = (1, 2, 3), ("lookup", "mu2")      # packed records: affine, full storage, beta <= 0
SLIM_TEAMS = ("2", "3", "6", "12")                               # the three-waves-per-SIMD sweep: affine, max_shift 1, LOOKUP
WINDOW_SHIFTS = (1, 2)                                           # the short-chain walk's LDS window


class Case(collections.namedtuple("Case", "rec s form storage beta local env shape fill_only")):
    """rec: "affine" | "linear"; form: which of mu1 / mu2 come as dense tables; storage: "full" | "score_only" |
    "lean_trace" | "level_trace"; beta: -1 | +1, the sign of the gap opening cost (0: the one-layer recurrence); env: the
    BIALIGN_* switches, sorted (name, value) pairs; fill_only: the run stops behind the sweep (the score-only traceback)."""
    __slots__ = ()

    @property
    def environ(self):
        return dict(self.env)

    @property
    def team(self):
        return self.environ.get("BIALIGN_TEAM", "1")

    @property
    def kind(self):
        """The molecules and lookup tables.  Proteins, but for the affine sweeps at max_shift 3 with both tables dense: a
        workgroup's LDS holds the lookup tables too, and with BLOSUM62's 24 x 24 entries team_shape finds four waves 8 bytes
        above 160 KiB and plans two; with RNA's 4 x 4 they fit.  (Every team of that form, so that their results compare.)"""
        return "rna" if (self.rec, self.s, self.form) == ("affine", 3, "mu12") else "protein"

    def inputs(self, tie=False):
        """(shape, form, kind, planted): what pair_of / tables_of draw the molecules and tables from."""
        return self.shape, self.form, self.kind, bool(tie)

    @property
    def wide(self):
        return self.s > 5

    @property
    def packed(self):
        return self.environ.get("BIALIGN_PACK") == "1"

    @property
    def slim(self):
        return self.environ.get("BIALIGN_SLIM") == "1"

    @property
    def id(self):
        words = [self.rec, f"s{self.s}", self.form, self.storage, {-1: "neg", 0: "zero", 1: "pos"}[self.beta]]
        words += ["local"] if self.local else []
        words += ["fillonly"] if self.fill_only else []
        words += [k[len("BIALIGN_"):].lower() + v for k, v in self.env]
        return "-".join(words)

    def params(self, tie=False):
        """The alignment parameters; ``tie``: shift_cost 0, where most columns of a trace have several candidates."""
        p = dict(synth.RNA_PARAMS if self.kind == "rna" else synth.PROTEIN_PARAMS, max_shift=self.s)
        if self.rec == "linear":
            p.update(LIN)
        elif self.beta > 0:
            p.update(gap_opening_cost=BETA_ANY)
        if tie:
            p.update(shift_cost=0)
        return p

    def has_walk(self):
        """A traceback kernel writes a trace."""
        return not self.fill_only and self.storage != "score_only"

    def tie_dense(self):
        """The case runs a second time with shift_cost 0."""
        return self.has_walk() and self.s >= 1

    def plan(self):
        """What the planner must decide: tw, gw, slim, pack, storage."""
        t = self.team
        tw, gw = (1, int(t[1:])) if t[0] == "x" else (8, int(t[1:])) if t[0] == "h" else (int(t), 1)
        return dict(tw=tw, gw=gw, slim=int(self.slim), pack=int(self.packed), storage=STORAGE_FLAG[self.storage])


def case(rec, s, form="lookup", storage="full", beta=None, local=False, shape=None, fill_only=False, **env):
    beta = (-1 if rec == "affine" else 0) if beta is None else beta
    env = {"BIALIGN_" + k.upper(): str(v) for k, v in env.items()}
    if s <= 5:
        env.setdefault("BIALIGN_TEAM", "1")
        env.setdefault("BIALIGN_PACK", "0")
        env.setdefault("BIALIGN_SLIM", "0")
    if shape is None:
        team = env.get("BIALIGN_TEAM", "1")
        shape = (WIDE_SHAPE if s > 5 else (LOCAL_ONE if local else ONE_WAVE)[s] if team == "1" else
                 TEAM_SHAPE[(team.lstrip("x"), s)])
    return Case(rec, s, form, storage, beta, local, tuple(sorted(env.items())), shape, fill_only)


def _cases():
    out = []
    # the sweeps of global alignments, full and LEAN records, every team; packed records beside the full ones
    for rec, teams in (("affine", AFFINE_TEAMS), ("linear", LINEAR_TEAMS)):
        for team, shifts, forms in teams:
            for s in shifts:
                for form in forms:
                    for storage in ("full", "score_only"):
                        out.append(case(rec, s, form, storage, team=team))
                    if rec == "affine" and s in PACKED_SHIFTS and form in PACKED_FORMS:   # (the generic walk over packed records)
                        out.append(case(rec, s, form, team=team, pack=1, trace_fast=0))
    # the general-beta algebra: one wave
    for s in SHIFTS:
        for form in FORMS:
            for storage in ("full", "score_only"):
                out.append(case("affine", s, form, storage, beta=1))
    # the three-waves-per-SIMD sweep: LEAN and packed records
    for team in SLIM_TEAMS:
        out.append(case("affine", 1, storage="score_only", team=team, slim=1))
        out.append(case("affine", 1, team=team, slim=1, pack=1, trace_fast=0))
    # the memory-lean traceback: strip re-sweeps and the strip walk (mu2 forms: two strips per round)
    for rec, betas in (("affine", (-1, 1)), ("linear", (0,))):
        for s in SHIFTS:
            for form in FORMS:
                for beta in betas:
                    out.append(case(rec, s, form, "lean_trace", beta=beta, **(dict(resw_k=2) if form == "mu2" else {})))
    # local alignments: their own sweeps, one wave and four
    for rec, teams in (("affine", AFFINE_LOCAL_TEAMS), ("linear", LINEAR_LOCAL_TEAMS)):
        for team, shifts, forms in teams:
            for s in shifts:
                for form in forms:
                    for storage in ("full", "score_only"):
                        out.append(case(rec, s, form, storage, local=True, team=team))
    # the traceback kernels that only read the score (a fill-only run of a full-storage batch), full and packed records
    for rec in ("affine", "linear"):
        for s in SHIFTS:
            out.append(case(rec, s, fill_only=True))
            if rec == "affine" and s in PACKED_SHIFTS:
                out.append(case(rec, s, fill_only=True, pack=1))
    # the short-chain walk over packed records: without the LDS window, with it, with the shortest ring
    for s in PACKED_SHIFTS:
        out.append(case("affine", s, pack=1, trace_window=0))
        if s in WINDOW_SHIFTS:
            out.append(case("affine", s, pack=1))
            out.append(case("affine", s, pack=1, trace_window_k=4))
    # the wide-band path's walks: full layers (with and without the trace), checkpointed levels
    for rec in ("affine", "linear"):
        for form in ("lookup", "mu1"):
            out.append(case(rec, WIDE_S, form))
            out.append(case(rec, WIDE_S, form, "level_trace", wide_seg=8, wide_parts=2))
        out.append(case(rec, WIDE_S, fill_only=True))
    return out


CASES = _cases()

#: Variants the predicates build and no batch can reach: key -> (the line of team_shape / decide_pack that excludes it, the
#: Case whose plan shows the refusal).  Empty: every instantiated kernel can be launched.
UNREACHABLE = {}


# ---- a case -> the variants it launches --------------------------------------------------------------------------------

def flagset(*names):
    return frozenset(n for n in names if n)


def keys(c):
    """The variant keys of a case, as tests/variant_check.hip prints them: ("fill_affine" | "fill_linear" | "fill_slim", S,
    TW, flags), ("trace_affine" | "trace_linear", S, flags), ("trace_fast", S, window)."""
    out = set()
    dense2, dense1 = c.form in ("mu2", "mu12"), c.form in ("mu1", "mu12")
    d2, d1 = "DENSE" if dense2 else None, "DENSE1" if dense1 else None
    lean = c.storage != "full"
    if c.wide:      # the sweeps of the wide path take the band as a run-time value: only its walks are variants
        if c.storage == "level_trace":
            out.add((f"trace_{c.rec}", 0, flagset("TRACE", "LEVEL", d1)))
        elif c.fill_only:
            out.add((f"trace_{c.rec}", 0, flagset("WIDE")))
        else:
            out.add((f"trace_{c.rec}", 0, flagset("TRACE", "WIDE", d1)))
        return out
    plan = c.plan()
    if c.slim:
        out.add(("fill_slim", c.s, plan["tw"], flagset("LEAN" if lean else "PACK")))
    else:
        out.add((f"fill_{c.rec}", c.s, plan["tw"],
                 flagset(d2, d1, "LEAN" if lean else None, "LOCAL" if c.local else None, "PACK" if c.packed else None,
                         "BETA_ANY" if c.beta > 0 else None, "XCU" if plan["gw"] > 1 else None)))
    if c.storage == "lean_trace":
        out.add((f"fill_{c.rec}", c.s, 1, flagset("RESW", d2, d1, "BETA_ANY" if c.beta > 0 else None)))
        out.add((f"trace_{c.rec}", c.s, flagset("TRACE", "STRIP", d1)))
    elif c.storage == "full":
        env = c.environ
        if c.fill_only:
            out.add((f"trace_{c.rec}", c.s, flagset("PACK" if c.packed else None)))
        elif c.packed and c.form == "lookup" and not c.local and env.get("BIALIGN_TRACE_FAST") != "0":
            out.add(("trace_fast", c.s, int(env.get("BIALIGN_TRACE_WINDOW") != "0")))
        else:
            out.add((f"trace_{c.rec}", c.s, flagset("TRACE", d1, "PACK" if c.packed else None)))
    return out


def parse_variants(text):
    """The output of tests/variant_check.hip -> {key: instantiated by a ladder}."""
    out = {}
    for line in text.splitlines():
        kind, *words = line.split()
        w = dict(x.split("=") for x in words)
        flags = frozenset(w["F"].split("+")) - {"0"} if "F" in w else None
        if kind == "trace_fast":
            key = (kind, int(w["S"]), int(w["window"]))
        elif kind.startswith("trace_"):
            key = (kind, int(w["S"]), flags)
        else:
            key = (kind, int(w["S"]), int(w["TW"]), flags)
        assert key not in out, line
        out[key] = w["ladder"] == "1"
    return out


# ---- the inputs of a case, and the oracle on them ----------------------------------------------------------------------

#
# Two families of inputs per shape.  Plain: unrelated random molecules and tables of random integers.  Planted (the tie-dense
# runs): B carries a mutated copy of A along a random monotone path of min(n, m) matches, and the dense tables are raised
# along the same path.  With unrelated molecules and shift_cost 0 the sequence and the structure alignment part ways
# wherever that gains, the walk spends its time at the band's edge, where a column has one candidate, and 70 to 90 % of the
# columns are tied (long pairs at max_shift 1: 0.85 to 0.89 whatever the seed); with planted ones the two alignments
# agree, the walk stays inside the band, and 96 to 100 % are.

def planted_path(shape):
    """[(i, j)], 0-based and increasing in both: the matches of the planted pair of a shape."""
    import random
    n, m = shape
    rng, k = random.Random(9300 + 7 * n + m), min(n, m)
    return list(zip(sorted(rng.sample(range(n), k)), sorted(rng.sample(range(m), k))))


@functools.lru_cache(maxsize=None)
def pair_of(shape, kind="protein", planted=False):
    """(seqA, seqB, strA, strB) of a shape.  (RNA: the planted form leaves the molecules alone -- its cases read both
    scores from tables.)"""
    import random
    n, m = shape
    pair = (synth.rna_pair if kind == "rna" else synth.protein_pair)(9100 + 7 * n + m, n, m)
    if not planted or kind == "rna":
        return pair
    rng = random.Random(9400 + 7 * n + m)
    sa, sb, ta, tb = pair
    sb, tb = list(sb), list(tb)
    for i, j in planted_path(shape):    # a tenth of the copied letters mutate
        sb[j] = rng.choice(synth.PROTEIN_ALPHABET) if rng.random() < 0.1 else sa[i]
        tb[j] = rng.choice(synth.PROTEIN_SS_ALPHABET) if rng.random() < 0.1 else ta[i]
    return sa, "".join(sb), ta, "".join(tb)


@functools.lru_cache(maxsize=None)
def tables_of(shape, form, planted=False):
    """(mu1 table | None, mu2 table | None): seeded random integers, as tests/test_gpu_dense_mu1.py and _mu2.py draw them;
    planted: drawn below 100 and raised by 1000 / 800 along the planted path."""
    n, m = shape
    rng = np.random.default_rng(9200 + 7 * n + m)
    t1 = rng.integers(-400, (101 if planted else 1101), size=(n, m)).astype(np.int32)
    t2 = rng.integers(-300, (101 if planted else 901), size=(n, m)).astype(np.int32)
    if planted:
        for i, j in planted_path(shape):
            t1[i, j] += 1000
            t2[i, j] += 800
    return (t1 if form in ("mu1", "mu12") else None), (t2 if form in ("mu2", "mu12") else None)


def frozen(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=64)
def mu_tables(inputs, params):
    """The (n+1) x (m+1) score tables the oracle reads for ``inputs`` = (shape, form, kind, planted): the lookup scores,
    with the dense tables in their place."""
    from oracle import oracle
    shape, form, kind, planted = inputs
    mu1, mu2 = (np.array(t, dtype=np.int32) for t in oracle.mu_tables(*pair_of(shape, kind, planted), dict(params)))
    t1, t2 = tables_of(shape, form, planted)
    if t1 is not None:
        mu1[1:, 1:] = t1
    if t2 is not None:
        mu2[1:, 1:] = t2
    return mu1, mu2


@functools.lru_cache(maxsize=32)
def oracle_ref(inputs, params, want_trace=True):
    """The oracle's dict(score, layers, trace, complete), once per (inputs, parameters) among neighbouring cases (the
    table keeps the cases of one shape together; the largest layers take 140 MB)."""
    from oracle import oracle
    ahead = _AHEAD.get((inputs, params))
    if ahead is not None:
        return ahead.result()
    mu1, mu2 = mu_tables(inputs, params)
    return oracle.solve_tables(*inputs[0], dict(params), mu1, mu2, want_trace)


#: oracle runs started ahead of their tests: (inputs, parameters) -> future
_AHEAD = {}
HEAVY_CELLS = 3e6      # band cells (n m W^2) from which an oracle run takes several seconds


def heavy_runs():
    """The (inputs, parameters) of the few oracle runs that take 5 to 10 s: the slim team of twelve and the cross-CU team of
    eight-wave workgroups."""
    out = []
    for c in CASES:
        for tie in ((False, True) if c.tie_dense() else (False,)):
            key = (c.inputs(tie), frozen(c.params(tie)))
            if not c.local and c.shape[0] * c.shape[1] * (2 * c.s + 1) ** 2 >= HEAVY_CELLS and key not in out:
                out.append(key)
    return out


def solve_ahead(pool, keys):
    """Start the oracle runs of ``keys`` on the threads of ``pool`` (the oracle is C behind ctypes: it runs beside the
    tests); oracle_ref waits for them."""
    from oracle import oracle
    oracle.lib()
    for inputs, params in keys:
        mu1, mu2 = mu_tables(inputs, params)
        _AHEAD[(inputs, params)] = pool.submit(oracle.solve_tables, *inputs[0], dict(params), mu1, mu2, True)


def drop_ahead():
    _AHEAD.clear()


# ---- tie density: candidates per column of the oracle's trace ----------------------------------------------------------

def candidates_per_column(inputs, params):
    """A walk over the oracle's layers by the reference's rule, built from bialignment.affine_recursion_cases, affine_score
    and guard_case (the one-layer recurrence: recursion_cases): per column of the trace, end to start, how many (source,
    offset) candidates attain the cell's value.  The walk's columns are asserted to be the oracle's trace."""
    from oracle import oracle
    from bialign_amd import bialignment as ba
    n, m = inputs[0]
    prm = dict(params)
    s = prm["max_shift"]
    ref = oracle_ref(inputs, params)
    mu1, mu2 = mu_tables(inputs, params)
    lay = ref["layers"]
    me = types.SimpleNamespace(mu1=lambda i, j: int(mu1[i, j]), mu2=lambda k, l: int(mu2[k, l]), _params=prm,
                               beta=prm["gap_opening_cost"], gamma=prm["gap_cost"], max_shift=s,
                               states=ba.AffineDPMatrices(0, 0, 0).states)
    cell = lambda layer, x: int(lay[layer, x[0], x[1], x[2] - x[0] + s, x[3] - x[1] + s])  # noqa: E731
    idx, counts, cols = [n, m, n, m], [], []
    if prm["gap_opening_cost"] == 0:
        while True:
            hits = [off for off, sc in ba.BiAligner.recursion_cases(me, idx)
                    if ba.guard_case(off, idx, s) and cell(0, [a - b for a, b in zip(idx, off)]) + sc == cell(0, idx)]
            if not hits:
                break
            counts.append(len(hits))
            cols.append(list(hits[0]))
            idx = [a - b for a, b in zip(idx, hits[0])]
    else:
        states = [list(st) for st in ba.AffineDPMatrices(0, 0, 0).states]
        shift = lambda x, t: (t[0] + x[0] - x[2], t[1] + x[1] - x[3])  # noqa: E731
        end = [cell(t, idx) for t in range(9)]
        best = [t for t in range(9) if end[t] == max(end)]
        state = states[min(best, key=lambda t: sum(abs(v) for v in shift(states[t], (0, 0))))]
        total = (0, 0)
        while not (idx == [0, 0, 0, 0] and state == [1, 1, 1, 1]):
            cur = cell(states.index(state), idx)
            hits = [(src, off) for src, off, sc in ba.BiAligner.affine_recursion_cases(me, state, idx)
                    if cell(states.index(list(src)), [a - b for a, b in zip(idx, off)]) + sc == cur]
            if not hits:
                break
            counts.append(len(hits))

            def key(h):
                d = shift(h[0], shift(h[1], total))
                return abs(d[0]) + abs(d[1]), abs(d[1])
            src, off = min(hits, key=key)       # (the first minimum)
            total = shift(off, total)
            cols.append(list(off))
            idx = [a - b for a, b in zip(idx, off)]
            state = list(src)
    assert cols[::-1] == oracle.trace_to_lists(ref["trace"]), "the counting walk left the oracle's trace"
    return counts


def tie_density(inputs, params):
    """The share of the trace's columns with two or more candidates."""
    counts = candidates_per_column(inputs, params)
    return sum(c >= 2 for c in counts) / max(len(counts), 1)
