"""The inputs of tests/tied_ends.py are what they claim to be -- from the CPU oracle alone, no GPU: each has the tied best
ends its construction plants, where it plants them (one row, several rows in different strips, both end lines, one lane
and another of a 64-lane scan, the step classes of the team shape, the mask words of the hit search); the greedy hit
search finds one hit per copy; the pair in which nothing aligns has its constant profile and its ends; every scaled twin
sits at the last scale the int32 safety window admits with the ties of scale 1.

That the inputs bite: for every tied input the LAST best end -- what ``np.argmax`` over the reversed candidates would give --
differs from the expectation's, so an engine that broke ties towards the larger row, column, lane or strip would fail.

Oracle budget: about 245 core-seconds, 32 s of wall time in a pool of 16 (model: 363); the model's and the measured
figures are recorded in ``tied_ends.BUDGET``, and ``-s`` shows this run's.  All oracle runs of the module are made once
(``ref``).
"""
import math
import os
import resource
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hits_expected as he
import tied_ends as te
import window_edge as we
from free_ends_gpu import params_of

READ_ME = ("affine", "one-layer")   # the README costs: the constructions' claims hold for these to the cell


@pytest.fixture(scope="module")
def ref():
    cases = te.main_case_table()
    cases.update(te.team_case_table())
    cases.update(te.local_team_case_table())
    cases.update(te.twin_case_table(scales=("k", 1), want_layers=True))
    t0, c0 = time.time(), sum(resource.getrusage(resource.RUSAGE_CHILDREN)[:2])
    out = te.expected(cases)
    est = te.estimate(cases)
    print(f"\noracle budget: {len(cases)} expectations, model " + ", ".join(f"{k} {v:.0f}" for k, v in est.items()) +
          f" = {sum(est.values()):.0f} core-seconds; measured {sum(resource.getrusage(resource.RUSAGE_CHILDREN)[:2]) - c0:.0f} "
          f"core-seconds, {time.time() - t0:.1f} s of wall time")
    return out


def check_tie(mode, want, inp, claim=None):
    """At least two best ends, the expectation takes the first, the last differs; ``claim``: and they are exactly these."""
    ends = te.tied(mode, want, inp.n, inp.m)
    assert len(ends) >= 2, (inp, mode, ends)
    assert ends == sorted(ends) and te.end_of(mode, want) == ends[0] != ends[-1], (inp, mode, ends)
    if claim is not None:
        assert ends == claim, (inp, mode)
    return ends


# ---- the table's inputs, and (a) their tall variants ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode,cost,s", te.main_cases(), ids=lambda v: str(v))
def test_inputs_tie_where_they_claim(mode, cost, s, ref):
    inputs = te.inputs_of(mode, cost, s)
    assert inputs and "nothing" in [i.name for i in inputs]
    for inp in inputs:
        want = ref[(mode, "main", inp.name, cost, s)]
        # (a rewarded gap opening changes which ends tie, not that they do)
        check_tie(mode, want, inp, inp.tied[mode] if cost in READ_ME else None)
        if cost in READ_ME and inp.name != "nothing":
            if not (mode == "fit" and "row" in inp.name and inp.name != "overlap-row"):   # (FIT of y u y gaps the spacers)
                assert want["score"] == 11700, (inp, mode)


def test_where_the_ties_lie():
    """The claims' geometry: one row; one column; both end lines; lanes of a 64-lane scan; strips per band."""
    import test_gpu_local as tgl
    b = te.BASE
    assert len({i for i, _ in b["row"].tied["local"]}) == 1 and len({j for _, j in b["row"].tied["local"]}) == 3
    assert len({j for _, j in b["column"].tied["local"]}) == 1 and len({i for i, _ in b["column"].tied["local"]}) == 2
    cross = b["cross"]
    assert [(i == cross.n, j == cross.m) for i, j in cross.tied["overlap"]] == [(False, True), (True, False)]
    assert all(i == b["overlap-row"].n for i, _ in b["overlap-row"].tied["overlap"]) and len(b["overlap-row"].tied["overlap"]) == 3
    assert all(j == b["overlap-column"].m for _, j in b["overlap-column"].tied["overlap"]) and len(b["overlap-column"].tied["overlap"]) == 3
    far = b["fit-far"]
    assert far.m == 95 and [j % 64 for j in far.tied["fit"]] == [12, 12, 25]   # one lane twice, and another
    assert (b["nothing"].n, b["nothing"].m) == (7, 12) and len(b["nothing"].tied["local"]) == 104
    for s in te.SHIFTS:
        rr = te.rows_per_strip(s)
        assert tgl.rows_of(s) == 2 * rr + 4
        pick = (lambda name: te.tall(s)[f"tall-{name}-s{s}"]) if s in te.TALL_SHIFTS else (lambda name: b[name])
        strips = lambda inp, mode: [i // rr for i, _ in inp.tied[mode]]   # noqa: E731
        assert len(set(strips(pick("column"), "local"))) == 2, s
        assert len(set(strips(pick("cross"), "local"))) == 2 and len(set(strips(pick("cross"), "overlap"))) == 2, s
        assert len(set(strips(pick("overlap-column"), "overlap"))) == 3, s
        if s in te.TALL_SHIFTS:
            assert set(strips(pick("row"), "local")) == {1}, s           # below the first strip
            assert {i.name for i in te.inputs_of("local", "one-layer", s)} >= {f"tall-{x}-s{s}" for x in ("row", "column", "cross")}


# ---- (b) the team shape ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", READ_ME)
def test_team_inputs(cost, ref):
    geo = te.TEAM_GEO
    assert (geo.NS, geo.P) == (6, 280)   # six strips and a period of 280: a team of three
    for inp in te.TEAM.values():
        assert (inp.n, inp.m) == te.TEAM_SHAPE
        mode = inp.modes[0]
        check_tie(mode, ref[(mode, "team", inp.name, cost, 1)], inp, inp.tied[mode])
    assert te.TEAM["team-fit"].tied["fit"] == te.TEAM_ROW_ENDS == [j for _, j in te.TEAM["team-overlap-row"].tied["overlap"]]
    assert [te.row_n_step(j) for j in te.TEAM_ROW_ENDS] == ["before", "interior", "after"]
    assert te.TEAM_ROW_ENDS[-1] == geo.m   # B ends with a copy
    waves = [(i // geo.RR) % 3 for i, _ in te.TEAM["team-overlap-column"].tied["overlap"]]
    assert sorted(waves) == [0, 1, 2], waves


# ---- (c) LOCAL at the team shape of max_shift 2 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", READ_ME)
def test_local_team_input_by_its_parts(cost, ref):
    """The pair itself is out of local_expected's reach (about n m oracle fills of 101 x 278).  Its parts: a unit's score
    against itself; the cut-down twin of the same layout, whose best local score is that and whose tied ends are the
    planted ones; and the layout of the pair -- the units stand where the claim says, the rest is spacers."""
    params = params_of("protein", cost, te.LOCAL_TEAM_SHIFT)
    assert te.self_score(te.U, params) == te.self_score(te.V, params) == 11700
    short = te.LOCAL_TEAM_SHORT
    want = ref[("local", "team-short", short.name, cost, te.LOCAL_TEAM_SHIFT)]
    assert want["score"] == 11700
    check_tie("local", want, short, short.tied["local"])
    full = te.LOCAL_TEAM
    assert (full.n, full.m) == te.TEAM_SHAPE
    sa, sb, ta, tb = full.pair
    for inp in (short, full):   # the same layout: u then v in A; v, u, u in B; the ends are the units' ends
        a, b = inp.pair[0], inp.pair[1]
        (r1, c2), (_, c3), (r2, c1) = inp.tied["local"]
        assert [a[r - 9:r] for r in (r1, r2)] == [te.U[0], te.V[0]] and a.count("W") == inp.n - 18
        assert [b[c - 9:c] for c in (c1, c2, c3)] == [te.V[0], te.U[0], te.U[0]] and b.count("P") == inp.m - 27
        assert c1 < c2 < c3 and r1 < r2
    rr = te.rows_per_strip(te.LOCAL_TEAM_SHIFT)
    rows = sorted({i for i, _ in full.tied["local"]})
    assert len(rows) == 2 and len({(i // rr) % max(te.LOCAL_TEAM_SIZES) for i in rows}) == 2   # strips of different waves
    assert len({j for i, j in full.tied["local"] if i == rows[0]}) == 2                           # two columns in one row
    # spacers long enough that gapping them costs more than a unit scores (the twin's are shorter: checked by the oracle)
    assert min(len(x) for x in sa.replace(te.U[0], " ").replace(te.V[0], " ").split()) >= 11


# ---- the hit search: fit-far and (d) the mask input ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", READ_ME)
def test_greedy_finds_one_hit_per_copy(cost, ref):
    for inp, key, spans in ((te.BASE["fit-far"], ("fit", "main", "fit-far", cost, 1), te.FAR_SPANS),
                            (te.MASK, ("fit", "mask", te.MASK.name, cost, 1), te.MASK_SPANS)):
        want = ref[key]
        check_tie("fit", want, inp, [e for _, e in spans])
        for rule in (min, max):
            hits, walks, status = he.greedy(want["glob"], te.hit_spec(inp), rule)
            assert [h[:2] for h in hits] == spans and status == "exhausted", (inp, rule, hits, status)
            assert len(walks) > len(hits)   # min_score 1: ends beside the copies are candidates too
    # the aligning pair of test_nothing_aligns under hits=(3, 1): three hits in three walks, the first the batch's own
    hits, walks, status = he.greedy(ref[("fit", "main", "row", cost, 1)]["glob"], he.resolve((3, 1)), min)
    assert [h[1] for h in hits] == te.BASE["row"].tied["fit"] and len(walks) == 3 and status == "max_hits"
    # ... and fit-far's twin at the window's edge: the same three spans
    twin = te.TWINS["fit-far-" + ("affine" if cost == "affine" else "linear")]
    for rule in (min, max):
        hits, _, status = he.greedy(ref[("fit", "twin", twin.name, "k")]["glob"], te.hit_spec(twin), rule)
        assert [h[:2] for h in hits] == te.FAR_SPANS and status == "exhausted"
    assert te.MASK.n >= 40
    (s1, e1), (s2, e2), (s3, e3) = te.MASK_SPANS
    assert e1 % 32 == 31 and (s2 + 1) % 32 == 0 and len(te.mask_words((s3, e3))) == 3
    assert all(len(te.mask_words(sp)) >= 2 for sp in te.MASK_SPANS)


# ---- nothing aligns --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", READ_ME)
def test_nothing_aligns(cost, ref):
    inp = te.BASE["nothing"]
    for s in te.SHIFTS:
        fit = ref[("fit", "main", "nothing", cost, s)]
        gapped = -1000 if cost == "affine" else -700   # every residue of A in a gap, in both alignments
        assert he.profile(fit["glob"]).tolist() == [gapped] * (inp.m + 1) and (fit["score"], fit["end_b"]) == (gapped, 0)
        ovl = ref[("overlap", "main", "nothing", cost, s)]
        assert (ovl["score"], ovl["end"]) == (0, (0, inp.m)) and te.tied("overlap", ovl, inp.n, inp.m) == [(0, inp.m), (inp.n, 0)]
        if ("local", cost, s) in te.main_cases():
            loc = ref[("local", "main", "nothing", cost, s)]
            assert (loc["score"], loc["end"]) == (0, (0, 0)) and (loc["ends"] == 0).all()


# ---- (f) the scaled twins --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(te.TWINS))
def test_twin_sits_at_the_edge_with_the_ties_of_scale_one(name, ref):
    t = te.TWINS[name]
    k = t.k
    assert k >= 2 and t.product(k) < we.WINDOW <= t.product(k + 1)   # the mirror admits k and refuses k + 1
    measured = {}
    for mode in t.modes:
        one, edge = ref[(mode, "twin", name, 1)], ref[(mode, "twin", name, "k")]
        assert edge["score"] == k * one["score"]
        ends = check_tie(mode, edge, t)
        assert ends == te.tied(mode, one, t.n, t.m)
        measured[mode] = te.magnitude(edge)
        assert measured[mode] == k * te.magnitude(one) < t.product(k)
        print(f"{name:18s} {mode:8s} k={k:5d} finite=2^{math.log2(measured[mode]):.2f} ({measured[mode]}) score={edge['score']}")
    assert te.MEASURED[name] == (k, measured)


def test_measured_lists_every_twin_and_no_other():
    assert set(te.MEASURED) == set(te.TWINS)
