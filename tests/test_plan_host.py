"""The batch planner (bialign_amd/csrc/bialign_plan.hpp) decides on the CPU what bialign_capi.hip then allocates and
uploads; tests/plan_check.hip is a stand-alone host program around the same functions.  Here, without a GPU:

  * the window mirror of window_edge.py is the code: every case is admitted at its scale and refused one above;
  * chunk plans are sound (partition, contiguous offsets, budget, maxima, launch order, the full-record re-plan), the
    wide-band affine sweep's ring included: a term of its own beside layers and tables, inside the budget;
  * the storage ladder takes the steps the GPU fallback tests expect, from their inputs;
  * nothing moved: team_shape, plan_chunks, sweep_geometry, lds_need* and cells_of answer tests/plan_expected.txt, the
    table the code gave before it moved into the header;
  * one mode, the rules as before: every combination of FIT / LOCAL with the storage flags, bands, gap opening costs and
    budgets answers tests/mode_expected.txt, the table the planner gave while it kept the two flags as two booleans
    (its max_shift 6 affine plans: since the ring is planned);
  * the same program under AddressSanitizer and UBSan prints the same; the header calls nothing of HIP."""
import os
import re

import numpy as np
import pytest

import plan_host as ph
import window_edge as we
from bialign_amd import synth

SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE = 1, 2, 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ph.build(tmp_path_factory.mktemp("plan"))


# ---- the window mirror is the code ---------------------------------------------------------------------------------

def window_request(problems, k, **kw):
    """The batch of ``problems`` (one form, cost pattern and max_shift) at scale k: costs, and the maxima the host takes."""
    first = problems[0]
    p = first.at(k)
    words = dict(s=first.s, k1=4, k2=3, beta=p["gap_opening_cost"], gamma=p["gap_cost"], delta=p["shift_cost"], quiet=1)
    amax, bmax = (max(x) for x in zip(*(q.maxima(k) for q in problems)))
    if first.form == "feature":
        (fa, fb), = [q.features for q in problems]
        words.update(form="feature", amax=amax, sw=p["structure_weight"], fa=",".join(repr(float(np.max(f))) for f in fa),
                     fb=",".join(repr(float(np.max(f))) for f in fb))
    elif first.form in ("mu1", "mu2", "mu12"):
        words.update(form=first.form, amax=0 if "1" in first.form else amax, bmax=0 if "2" in first.form else bmax, mu1=-amax, mu2=bmax)
    else:
        words.update(amax=-amax, bmax=bmax)
    words.update(kw)
    return ph.request(pairs=[(q.n, q.m) for q in problems], **words)


def test_every_window_edge_case_is_admitted_at_its_scale_and_refused_above(exe):
    solo = list(we.CASES.values())
    reqs = [window_request([p], k) for p in solo for k in (p.k, p.k + 1)]
    got = ph.plans(exe, reqs)
    assert len(got) == 2 * len(we.CASES) and len(solo) == len(we.MEASURED)
    for p, at, above in zip(solo, got[0::2], got[1::2]):
        assert at.rc == 0, (p, at.msg)
        assert at.colmax == p.window(p.k)[0], p                # (FEATURE form: score_bound's sqrt bound == feature_bound)
        assert above.rc == ph.E_RANGE and "int32 safety window" in above.msg, (p, above.msg)


def test_feature_cases_go_through_the_sqrt_bound(exe):
    feats = [p for p in we.CASES.values() if p.form == "feature"]
    assert len(feats) == 3
    for p in feats:
        at, = ph.plans(exe, [window_request([p], p.k)])
        amax, bmax = p.maxima(p.k)
        assert bmax == we.feature_bound(p.at(p.k)["structure_weight"], *p.features)
        assert at.colmax == we.window(p.n, p.m, amax, bmax, *(p.at(p.k)[c] for c in ("gap_opening_cost", "gap_cost", "shift_cost")))[0]


def test_ragged_batch_at_the_batch_scale(exe):
    k = we.batch_scale(we.RAGGED)
    at, above = ph.plans(exe, [window_request(we.RAGGED, k), window_request(we.RAGGED, k + 1)])
    assert at.rc == 0 and at.npairs == len(we.RAGGED)
    assert above.rc == ph.E_RANGE and "int32 safety window" in above.msg and above.msg.startswith("pair 6:")   # (100, 100)


@pytest.mark.parametrize("p", we.NULL, ids=[p.name for p in we.NULL])
def test_null_batch_sum_of_squares_on_both_sides(exe, p):
    bound = p.product(p.k)
    rmax = we.sumsq_max_replicas(bound)
    assert rmax * bound * bound <= we.INT64_MAX < (rmax + 1) * bound * bound
    at, above = ph.plans(exe, [window_request([p], p.k, replicas=r, seed=5) for r in (rmax, rmax + 1)])
    assert at.rc == 0 and at.npairs == rmax and at.storage == SCORE_ONLY
    assert above.rc == ph.E_RANGE and "sum of squares" in above.msg and f"{rmax + 1} replica scores" in above.msg


# ---- chunk plans are sound -------------------------------------------------------------------------------------------

def ragged(seed, count, lo, hi):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(*lo)), int(rng.integers(*hi))) for _ in range(count)]


LOOKUP = dict(k1=24, k2=4, amax=1100, bmax=800)
CHUNKED = {
    "lookup-s1-packed": dict(pairs=ragged(11, 16, (60, 130), (120, 300)), s=1, **LOOKUP),
    "lookup-s3-linear": dict(pairs=ragged(12, 14, (30, 120), (30, 120)), s=3, beta=0, **LOOKUP),
    "feature-s2": dict(pairs=ragged(13, 14, (60, 110), (120, 260)), s=2, form="feature", k1=4, k2=1, amax=100, sw=400,
                       fa="1.0,0.75,1.0", fb="0.5,1.0,1.0"),
    "dense-null-s1": dict(pairs=ragged(14, 5, (30, 80), (30, 80)), s=1, form="mu12", mu1=-11, mu2=700, replicas=4, seed=9),
    "wide-s6": dict(pairs=ragged(15, 12, (10, 40), (10, 40)), s=6, **LOOKUP),
    "wide-s7-level": dict(pairs=ragged(16, 12, (10, 40), (10, 40)), s=7, flags=LEVEL_TRACE, **LOOKUP),
    "wide-s8-score-only": dict(pairs=ragged(17, 12, (10, 40), (10, 40)), s=8, flags=SCORE_ONLY, **LOOKUP),
    "wide-s7-null": dict(pairs=ragged(18, 5, (10, 40), (10, 40)), s=7, replicas=4, seed=9, **LOOKUP),
}
RINGED = ("wide-s6", "wide-s8-score-only", "wide-s7-null")   # the affine wide-band sweep outside the LEVEL forms: a ring term



def check_layout(plan, budget_dw, wide, sizes=None, layer_cap=None, tab_cap=None):
    sizes = sizes or [(z["dwords"], z["tab_dwords"]) for z in plan.sizes]
    n = len(plan.pairs)
    assert len(plan.rings) in (0, n) and (len(plan.rings) == n) == ("max_chunk_ring_dwords" in plan.fields)
    rings = [z["ring_dwords"] for z in plan.rings] or [0] * n
    cb = plan.chunks
    assert cb[0] == 0 and cb[-1] == n and all(a < b for a, b in zip(cb, cb[1:]))          # a partition, in order
    tabs = any(t for _, t in sizes)
    max_lay = max_tab = max_ring = 0
    for a, b in zip(cb, cb[1:]):
        lay = tab = ring = 0
        for p in range(a, b):                                                              # contiguous from 0
            assert plan.pairs[p]["layer_off"] == lay and (not tabs or plan.pairs[p]["tab_off"] == tab), (p, plan.pairs[p])
            assert not plan.rings or plan.rings[p]["ring_off"] == ring == plan.pairs[p]["scratch_off"], (p, plan.rings[p])
            lay, tab, ring = lay + sizes[p][0], tab + sizes[p][1], ring + rings[p]
        assert lay + tab + ring <= budget_dw
        assert layer_cap is None or (lay <= layer_cap and tab <= tab_cap)
        max_lay, max_tab, max_ring = max(max_lay, lay), max(max_tab, tab), max(max_ring, ring)
        key = (lambda p: plan.shape[p][0] + plan.shape[p][1]) if wide else (lambda p: plan.pairs[p]["G"])
        assert plan.order[a:b] == sorted(range(a, b), key=key, reverse=True)              # (sorted() is stable; so is reverse=)
    assert plan.max_chunk_dwords == max_lay and plan.max_chunk_tab_dwords == max_tab
    assert plan.fields.get("max_chunk_ring_dwords", 0) == max_ring


@pytest.mark.parametrize("name", list(CHUNKED))
def test_chunk_plans_are_sound(exe, name):
    case = dict(CHUNKED[name])
    shapes = case.pop("pairs")
    R = case.get("replicas", 1)
    wide = case["s"] > 5
    one, = ph.plans(exe, [ph.request(pairs=shapes, replan=1, **case)])
    assert one.rc == 0 and one.nchunks == 1 and one.npairs == len(shapes) * R
    assert one.pack == (name in ("lookup-s1-packed", "feature-s2"))                      # (so the re-plan below is exercised)
    # the ring term is the formula's, for every pair of a plan that has one -- and only such plans print it
    vshapes = [s for s in shapes for _ in range(R)]
    assert [z["ring_dwords"] for z in one.rings] == ([ph.ring_dwords(n, case["s"]) for n, _ in vshapes] if name in RINGED else [])
    rings = [z["ring_dwords"] for z in one.rings] or [0] * len(vshapes)
    total = 4 * sum(z["dwords"] + z["tab_dwords"] + r for z, r in zip(one.sizes, rings))
    # the largest pair must still fit, with full records where packed ones have to be able to fall back to them
    largest = 4 * max((z["full_dwords"] if one.pack else z["dwords"]) + z["tab_dwords"] + r for z, r in zip(one.sizes, rings))
    # 3/4 of the total: two chunks wanted, the first closes once it holds half; a sixth: six wanted, no fewer than five
    budgets = {1: total, 2: total * 3 // 4, 5: max(total // 6, largest)}
    got = ph.plans(exe, [ph.request(pairs=shapes, replan=1, budget=b, **case) for b in budgets.values()])
    for (want, budget), plan in zip(budgets.items(), got):
        assert plan.rc == 0, plan.msg
        print(name, "budget", budget, "->", plan.nchunks, "chunks")
        assert (plan.pack, plan.storage) == (one.pack, one.storage)                         # the budget cut chunks, nothing else
        assert plan.nchunks == want if want < 5 else plan.nchunks >= 5
        plan.shape = vshapes
        check_layout(plan, budget // 4, wide)
        assert (plan.fields.get("max_chunk_ring_dwords", 0) > 0) == (name in RINGED) and plan.rings == [
            dict(z, ring_off=w["ring_off"]) for z, w in zip(one.rings, plan.rings)]      # (the term itself does not move)
        if name == "dense-null-s1" or name == "feature-s2":
            assert plan.max_chunk_tab_dwords > 0
        if one.pack:   # the re-plan at full-record sizes, inside the buffers of the first plan
            again = plan.replanned
            assert again is not None and again.rc == 0 and not again.packed_sizing
            again.shape = plan.shape
            layer_cap, tab_cap = int(plan.replan["layer_cap"]), int(plan.replan["tab_cap"])
            full = [(z["full_dwords"], z["tab_dwords"]) for z in plan.sizes]
            check_layout(again, layer_cap + (tab_cap if tab_cap else 0), wide, full, layer_cap, tab_cap if tab_cap else 0)
            assert [d["scratch_off"] - d["layer_off"] for d in again.pairs] == [d["scratch_off"] - d["layer_off"] for d in plan.pairs]
        else:
            assert plan.replanned is None


# ---- the storage ladder ------------------------------------------------------------------------------------------------

def test_fallback_to_lean_trace_and_the_refusal(exe):
    """The inputs of test_gpu_lean_trace.test_engine_falls_back_to_lean_traceback_when_a_pair_exceeds_the_budget."""
    pairs = [synth.protein_pair(1500 + t, 400, 380) for t in range(2)]
    shapes = [(400, 380)] * 2
    affine = ph.scoring_words(dict(synth.PROTEIN_PARAMS), pairs)
    linear = ph.scoring_words(dict(synth.PROTEIN_PARAMS, gap_opening_cost=0, gap_cost=-200, shift_cost=-250), pairs)
    full, lean, full_l, lean_l, refused = ph.plans(exe, [
        ph.request(pairs=shapes, **affine), ph.request(pairs=shapes, budget=12 << 20, **affine),
        ph.request(pairs=shapes, **linear), ph.request(pairs=shapes, budget=2 << 20, **linear),
        ph.request(pairs=shapes, budget=64 << 10, **affine)])
    assert full.rc == 0 and full.storage == 0 and full.pack == 1
    assert lean.rc == 0 and lean.storage == LEAN_TRACE and lean.pack == 0 and 4 * lean.max_chunk_dwords <= 12 << 20
    assert full_l.storage == 0 and lean_l.storage == LEAN_TRACE and 4 * lean_l.max_chunk_dwords <= 2 << 20
    assert refused.rc == ph.E_NOMEM and re.fullmatch(r"pair 0 needs \d+ bytes of layers, budget is 65536", refused.msg)


def test_fallback_to_level_trace_for_wide_bands(exe):
    """test_gpu_level_trace.test_memory_and_automatic_choice and the 1 MiB refusal of test_refusals_and_errors."""
    w = ph.scoring_words(dict(synth.PROTEIN_PARAMS, max_shift=6), [synth.protein_pair(5500, 300, 300)])
    full, asked, auto = ph.plans(exe, [ph.request(pairs=[(300, 300)], **w), ph.request(pairs=[(300, 300)], flags=LEVEL_TRACE, **w),
                                       ph.request(pairs=[(300, 300)], budget=400 << 20, **w)])
    assert full.storage == 0 and asked.storage == LEVEL_TRACE == auto.storage
    assert 4 * auto.max_chunk_dwords <= 400 << 20 and 4 * asked.max_chunk_dwords * 10 <= 4 * full.max_chunk_dwords * 4
    assert auto.wide_seg == asked.wide_seg >= 8
    w8 = ph.scoring_words(dict(synth.PROTEIN_PARAMS, max_shift=8), [synth.protein_pair(5601, 60, 60)])
    refused, = ph.plans(exe, [ph.request(pairs=[(60, 60)], budget=1 << 20, **w8)])
    assert refused.rc == ph.E_NOMEM and "budget is 1048576" in refused.msg


def test_wide_ring_is_cut_into_chunks_inside_the_budget(exe):
    """64 score-only pairs of 60 x 60 at max_shift 8 under 16 MiB: 16 dwords of layers each, and a ring of 5 levels =
    1 259 955 dwords = 5.04 MB each, 322.5 MB in all -- planned as one launch of 4 KiB while the ring was outside the plan.
    No chunk may hold more than the budget, so there are at least ceil(64 * 4 * (ring + 16) / 16 MiB) = 20 of them (three
    pairs fit a chunk: 22); a budget below one pair's ring is refused at creation, the ring's bytes in the message."""
    budget, shapes = 16 << 20, [(60, 60)] * 64
    ring = ph.ring_dwords(60, 8)
    assert ring == 1259955
    plan, = ph.plans(exe, [ph.request(pairs=shapes, s=8, flags=SCORE_ONLY, budget=budget, **LOOKUP)])
    assert plan.rc == 0 and plan.storage == SCORE_ONLY, plan.msg
    assert [z["ring_dwords"] for z in plan.rings] == [ring] * 64 and [z["dwords"] for z in plan.sizes] == [16] * 64
    plan.shape = shapes
    check_layout(plan, budget // 4, True)
    for a, b in zip(plan.chunks, plan.chunks[1:]):
        assert 4 * (b - a) * (ring + 16) <= budget
    print("64 x (60, 60), s=8, SCORE_ONLY, 16 MiB ->", plan.nchunks, "chunks")
    assert plan.nchunks >= -(-64 * 4 * (ring + 16) // budget) == 20
    refused, = ph.plans(exe, [ph.request(pairs=shapes, s=8, flags=SCORE_ONLY, budget=4 * ring, **LOOKUP)])
    assert refused.rc == ph.E_NOMEM, refused.msg
    assert refused.msg == f"pair 0 needs 64 bytes of layers and {4 * ring} of the wide-band ring, budget is {4 * ring}"


def test_wide_ring_counts_in_the_fallback_to_level_trace(exe):
    """A full-storage wide pair whose layers fit the budget and whose layers + ring do not is served from checkpointed
    levels; four bytes more and it keeps its full layers."""
    shapes = [(40, 44)]
    roomy, = ph.plans(exe, [ph.request(pairs=shapes, s=6, **LOOKUP)])
    assert roomy.rc == 0 and roomy.storage == 0
    layers, ring = 4 * roomy.sizes[0]["dwords"], 4 * roomy.rings[0]["ring_dwords"]
    assert ring == 4 * ph.ring_dwords(40, 6) and 0 < ring < layers
    fits, short, bare = ph.plans(exe, [ph.request(pairs=shapes, s=6, budget=b, **LOOKUP) for b in (layers + ring, layers + ring - 4, layers)])
    assert (fits.storage, fits.nchunks, fits.max_chunk_ring_dwords) == (0, 1, ring // 4)
    for plan in (short, bare):   # (the layers alone would have fitted)
        assert plan.rc == 0 and plan.storage == LEVEL_TRACE and not plan.rings and "max_chunk_ring_dwords" not in plan.fields
        assert 4 * plan.max_chunk_dwords <= layers


def test_packed_records_are_dropped_when_the_full_fallback_would_not_fit(exe):
    shapes = [(400, 380)] * 2
    roomy, = ph.plans(exe, [ph.request(pairs=shapes, s=1, **LOOKUP)])
    assert roomy.pack == 1 and roomy.packed_sizing == 1
    packed, full = 4 * roomy.sizes[0]["dwords"], 4 * roomy.sizes[0]["full_dwords"]
    assert packed < full
    fits, short = ph.plans(exe, [ph.request(pairs=shapes, s=1, budget=b, **LOOKUP) for b in (full, full - 4)])
    assert (fits.pack, fits.storage, fits.nchunks) == (1, 0, 2)
    assert short.pack == 0 and short.packed_sizing == 0 and short.storage == LEAN_TRACE   # (packed records alone would have fitted)


# ---- nothing moved -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def moved(exe):
    return ph.run(exe, "\n".join(ph.moved_requests()) + "\n")


def test_moved_functions_answer_as_before_the_split(moved):
    with open(ph.EXPECTED) as f:
        want = f.read().splitlines()
    got = moved.splitlines()
    for at, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, f"line {at}"
    assert len(got) == len(want)
    teams = {ln.split(" ", 2)[2] for ln in want if ln.startswith("team ")}
    assert len(teams) >= 15 and any("slim=1" in t for t in teams) and any("tw=8 gw=" in t and "gw=1 " not in t for t in teams)


def test_modes_answer_as_the_two_booleans_did(exe):
    got = ph.drop_mode_lines(ph.run(exe, "\n".join(ph.mode_requests()) + "\n")).splitlines()
    with open(ph.MODE_EXPECTED) as f:
        want = [ln for ln in f.read().splitlines() if not ln.startswith("#")]
    for at, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, f"line {at}"
    assert len(got) == len(want)
    refusals = {ln.split(" msg=")[1] for ln in want if ln.startswith("rc=-")}
    assert len(refusals) >= 12 and sum(ln == "rc=0 msg=" for ln in want) >= 40


def test_same_under_address_and_ub_sanitizers(moved, tmp_path):
    san = ph.build(tmp_path, name="plan_check_san", extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert ph.run(san, "\n".join(ph.moved_requests()) + "\n") == moved
    reqs = [window_request([p], p.k + d) for p in we.BOTH_SIDES for d in (0, 1)] + \
           [ph.request(pairs=c["pairs"], replan=1, **{k: v for k, v in c.items() if k != "pairs"}) for c in CHUNKED.values()]
    text = "\n".join(reqs) + "\n"
    assert ph.run(san, text) == ph.run(ph.build(tmp_path), text)


def test_planner_header_calls_nothing_of_hip():
    with open(os.path.join(ph.REPO, "bialign_amd", "csrc", "bialign_plan.hpp")) as f:
        assert not re.search(r"\bhip[A-Z]\w*\s*\(", f.read())
