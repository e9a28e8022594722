"""The packed-record boundary cases are what tests/pack_boundary.py says they are -- from the oracle alone, no GPU:
the background is low-spread, every (family, side) has a case that fits with no margin and one that misses by one,
every confined case has exactly its intended record out of range and at the intended step, and the verdict helper
is right on hand-built layers."""
import numpy as np
import pytest

import pack_boundary as pb
from pack_boundary import BOTH_SIDES, CONFINED, CROSS_CU, GHOST_ROW, NEG, Geometry, excess, offenders, pack_verdict, reference


def test_verdict_on_hand_built_layers():
    n, m, s = 45, 60, 1
    geo = Geometry(s, n, m)
    rng = np.random.default_rng(7)
    lay = rng.integers(1000, 1200, size=(9, n + 1, m + 1, 3, 3)).astype(np.int32)
    v = pack_verdict(lay, n, m, s)
    assert v["interior"].any() and v["fits"].all() and not pb.falls_back(v)
    # interior: strip >= Q0 (rows from 20), phase j + 2 il + a in LO .. m - s, k = i + a - s inside the molecule
    assert v["interior"][25, 40, 1] and not v["interior"][5, 40, 1] and not v["interior"][25, 2, 1]
    assert geo.place(25, 40, 1) == (1, 6, 1, 53) and geo.interior(1, 53)
    assert not v["interior"][45, 20, 2]          # k = n + 1
    # one value one too high
    i, j, a = 25, 40, 1
    hot = lay.copy()
    hot[4, i, j, a, 2] = hot[8, i, j, a, 0] + 0x7FFE
    v = pack_verdict(hot, n, m, s)
    assert v["hi"][i, j, a] == 0x7FFE and v["fits"][i, j, a] and offenders(v) == []
    hot[4, i, j, a, 2] += 1
    v = pack_verdict(hot, n, m, s)
    assert v["hi"][i, j, a] == 0x7FFF and offenders(v) == [(i, j, a)]
    # ... and one too low; exactly at the limit fits
    low = lay.copy()
    low[0, i, j, a, 1] = low[8, i, j, a, 0] - 0x8000
    assert offenders(pack_verdict(low, n, m, s)) == []
    low[0, i, j, a, 1] -= 1
    v = pack_verdict(low, n, m, s)
    assert v["lo"][i, j, a] == 0x8001 and offenders(v) == [(i, j, a)]
    # a corner slot at -2^30 does not count; the same value in any other slot does
    mark = lay.copy()
    mark[3, i, j, a, 0] = NEG                    # state 3, band column 0: a pack_corner slot
    assert offenders(pack_verdict(mark, n, m, s)) == []
    mark[4, i, j, a, 0] = NEG
    assert offenders(pack_verdict(mark, n, m, s)) == [(i, j, a)]
    # the same overflow in a step that is not interior stores a full record: no fallback
    edge = lay.copy()
    edge[4, 5, 40, 1, 2] += 0x10000
    v = pack_verdict(edge, n, m, s)
    assert not v["fits"][5, 40, 1] and not pb.falls_back(v)


@pytest.mark.parametrize("key", sorted({(c.family, c.s, c.seed, c.n, c.m, c.pos) for c in BOTH_SIDES + CROSS_CU + GHOST_ROW + CONFINED}), ids=str)
def test_background_is_low_spread(key):
    fam, s, seed, n, m, pos = key
    v = reference(pb.Case("background", fam, s, seed, n, m, pos, 0))["verdict"]
    assert v["interior"].sum() > 100
    assert v["hi"][v["interior"]].max() < 4096 and v["lo"][v["interior"]].max() < 4096


@pytest.mark.parametrize("case", BOTH_SIDES + CROSS_CU, ids=repr)
def test_margin_is_what_the_case_says(case):
    v = reference(case)["verdict"]
    ex, side = excess(v)
    ex = np.where(v["interior"], ex, np.iinfo(np.int64).min)
    worst = np.unravel_index(ex.argmax(), ex.shape)
    assert ex[worst] == -case.tags["margin"]
    assert side[worst] == (0 if case.tags["side"] == "hi" else 1)
    if case.tags["margin"] == 0:
        assert (v["hi"][worst] == 0x7FFE) if case.tags["side"] == "hi" else (v["lo"][worst] == 0x8000)
    assert pb.falls_back(v) == (case.tags["margin"] < 0)
    # mid-lattice: a strip past Q0, a column well inside
    geo = v["geo"]
    strip, _, qs, c = geo.place(*worst)
    assert strip == qs > geo.Q0 and geo.LO + 8 <= c <= geo.HI - 8


def test_every_family_and_side_has_margin_zero_and_excess_one():
    have = {(c.family, c.s, c.tags["side"], c.tags["margin"]) for c in BOTH_SIDES}
    for fam, shifts in (("lookup", (1, 2, 3)), ("mu2", (1, 2, 3)), ("mu1", (1,))):
        for s in shifts:
            for side in ("hi", "lo"):
                assert {(fam, s, side, mg) for mg in (1, 0, -1)} <= have
    # one for one: the three spikes of a (family, shift, side) are consecutive integers
    for fam, s, side, _ in have:
        xs = sorted(abs(c.x) for c in BOTH_SIDES if (c.family, c.s, c.tags["side"]) == (fam, s, side))
        assert xs == [xs[0], xs[0] + 1, xs[0] + 2]


@pytest.mark.parametrize("case", GHOST_ROW, ids=repr)
def test_ghost_row_cases_sit_in_a_bottom_row_at_margin_zero(case):
    ref = reference(case)
    v, geo = ref["verdict"], ref["verdict"]["geo"]
    rec = case.tags["record"]
    ex, _ = excess(v)
    assert not pb.falls_back(v) and v["interior"][rec]
    assert ex[rec] == np.where(v["interior"], ex, np.iinfo(np.int64).min).max() == 0
    assert (v["hi"][rec] == 0x7FFE) if case.tags["side"] == "hi" else (v["lo"][rec] == 0x8000)
    strip, il, qs, _ = geo.place(*rec)
    assert il == geo.RR and strip == qs >= geo.Q0 and (strip + 1) * geo.RR <= case.n   # a full strip feeds on it
    i, j, a = rec
    marks = [(st, bb) for st in range(9) for bb in range(geo.W)
             if pb.pack_corner(geo.W, st, bb) and ref["layers"][st, i, j, a, bb] == NEG]
    assert marks == [tuple(x) for x in case.tags["marks"]]


def test_ghost_row_cases_cover_both_extremes_and_a_mark_at_either_shift():
    for s in (1, 2):
        mine = [c for c in GHOST_ROW if c.s == s]
        assert {c.tags["side"] for c in mine} == {"hi", "lo"} and any(c.tags["marks"] for c in mine)


@pytest.mark.parametrize("case", CONFINED, ids=repr)
def test_confined_cases_are_confined(case):
    v = reference(case)["verdict"]
    assert offenders(v) == [tuple(r) for r in case.tags["offenders"]]
    if not case.tags["offenders"]:   # the spike is oversize all the same -- in records of steps that are not interior
        ex, _ = excess(v)
        assert ((ex > 0) & ~v["interior"]).any() and abs(case.x) >= 40000


def test_confined_cases_lie_where_their_names_say():
    geo = Geometry(1, 110, 280)
    assert (geo.NS, geo.P, geo.RR, geo.Q0) == (6, 282, 20, 1)
    rec = lambda name: pb.CASES[name].tags["offenders"][0]
    at = lambda name: geo.place(*rec(name))
    assert at("b-first-interior-column")[2:] == (2, geo.LO) and at("b-last-interior-column")[2:] == (2, geo.HI)
    assert at("b-first-interior-strip")[0] == geo.Q0
    i, _, a = rec("b-row-n-of-partial-last-strip")
    assert i == geo.n and (geo.NS - 1) * geo.RR < geo.n < geo.NS * geo.RR - 1
    # the W lane records a LOOKUP spike at (i0, j0) touches are (i0, j0, a): all of them outside the interior phases
    for name in ("b-column-before-first-interior", "b-column-after-last-interior", "b-strip-before-first-interior"):
        i0, j0 = pb.CASES[name].pos
        assert not any(geo.interior(*geo.place(i0, j0, a)[2:]) for a in range(geo.W))
    assert pb.CASES["b-strip-before-first-interior"].pos[0] // geo.RR == geo.Q0 - 1
    i0, j0 = pb.CASES["b-column-before-first-interior"].pos
    assert geo.place(i0, j0, geo.W - 1)[3] == geo.LO - 1
    i0, j0 = pb.CASES["b-column-after-last-interior"].pos
    assert geo.place(i0, j0, 0)[3] == geo.HI + 1
    last = geo.NS - 1
    for team in (1, 3):
        # the check runs at the head of every step of a wave that is a multiple of 16, before that step's own records
        # count; the record lies in the second strip its wave sweeps, so the wave's step count differs between the teams
        step = lambda name: geo.local_step(*rec(f"{name}-team{team}"), team=team)
        assert step("c-step-before-a-check") % geo.CHECK == geo.CHECK - 1
        assert step("c-step-after-a-check") % geo.CHECK == 0
        assert at(f"c-step-before-a-check-team{team}")[0] // team >= 1
        # The lane row of this record lies beyond n in the NEXT strip its wave sweeps, the last one: the first interior step
        # there clears the lane's accumulator, and this record is the last the lane stores before.
        strip, il, qs, c = at(f"c-row-that-leaves-the-lattice-team{team}")
        assert (strip, qs, c) == (last - team, last - team, geo.HI) and last * geo.RR + il - 1 > geo.n
    assert at("c-last-interior-step-of-sweep")[2:] == (last, geo.HI)
    assert at("c-first-interior-step-of-last-strip")[2:] == (last, geo.LO)
    # After its last interior step (phase m - S of its last strip) a wave walks on to phase m + MAXOFF: MAXOFF + S steps
    # that are not interior, more than a check interval at every max_shift.  A periodic check always follows the last
    # packed record, so the check after the last step never decides alone -- no input can make it the only witness.
    for s in (1, 2, 3):
        g = Geometry(s, 110, 280)
        last_interior = (g.NS - 1) * g.P + g.HI          # the wave's step at lane 0's phase m - S (a team of one)
        assert g.wave_steps() - 1 - last_interior == g.MAXOFF + s >= g.CHECK + 8


@pytest.mark.parametrize("s", [1, 2, 3])
def test_a_check_falls_between_the_interior_runs_of_two_strips(s):
    """What the static_assert in the sweeps states (Pack<S>::check_in_every_gap), restated on the numbers."""
    geo = Geometry(s, 100, 100)
    gap = geo.P - (geo.HI - geo.LO + 1)          # Pack<S>::nbs
    assert gap >= geo.LO + s + 1 >= max(geo.CHECK, geo.BLK)
