"""Peak candidates and per-pair thresholds of the hit search (include/bialign.h, "Hit search") on the GPU against
tests/hits_peaks_expected.py: the profile is the oracle's bit for bit, and the walk log replays, step by step, as the greedy
loop the model prescribes from the profile's peaks and the pair's own threshold.

The inputs, ``search`` and ``same_results`` are those of tests/test_gpu_fit_hits.py.  The oracle runs of every case of this
module are made once, in one spawn pool (``ref``), and shared."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_expected as fe
import hits_expected as he
import hits_peaks_expected as hp
from free_ends_gpu import params_of
from test_gpu_fit_hits import (FORM_PAIR, FORM_PARAMS, TEAM_SHAPE, case_pairs, half_best, main_cases, pair_of,
                               same_results, search)

pytestmark = pytest.mark.gpu

EDGE_N = 4
EDGE_MS = (31, 32, 33, 63, 64, 65, 127)   # m + 1 ends: one bit short of a mask word, a full word, one bit into the next; two blocks of 64
EDGE_COSTS = ("affine", "one-layer")
RAGGED = [("protein", 1, 50, True), ("protein", 22, 50, True), ("protein", 50, 97, True), ("protein", 22, 50, True)]
# (rising cost in the input: a chunk is launched by falling cost, so the launch order is another)


@pytest.fixture(scope="module")
def ref():
    """{key: fit_expected's dict} for every pair of this module."""
    cases = {}
    for cost, s in main_cases():
        for kind, n, m, planted in case_pairs(cost, s):
            prm = params_of(kind, cost, s)
            cases[("main", cost, s, kind, n, m, planted)] = (n, m, prm, *fe.tables_of(pair_of(kind, n, m, planted), prm), False)
    for cost in EDGE_COSTS:
        prm = params_of("protein", cost, 1)
        for m in EDGE_MS:
            cases[("edge", cost, m)] = (EDGE_N, m, prm, *fe.tables_of(pair_of("protein", EDGE_N, m, True), prm), False)
    prm = params_of("protein", "affine", 1)
    for planted in (True, False):
        cases[("team", planted)] = (*TEAM_SHAPE, prm, *fe.tables_of(pair_of("protein", *TEAM_SHAPE, planted), prm), False)
    for cost in he.PLANTED_COSTS:
        cases[("planted", cost)] = he.planted_case(cost)[3]
    return fe.expected_many(cases)


def run(b):
    got = search(b)
    got["thresholds"] = b.hit_thresholds()
    return got


def check(got, spec, wants, peaks, thresholds=None, pairs=None, params=None, affine=None):
    """Every pair: the profile is the oracle's, the log replays under the peak rule and the pair's threshold, no walk
    starts from a non-peak, ``hit_thresholds()`` is the threshold, hit 0 is the batch's own alignment, and (``pairs``
    given) every hit's trace, re-scored on B[start:end], gives its score."""
    start, end = got["spans"]
    traces, complete = got["traces"]
    if pairs is not None:
        from bialign_amd.batch import encode_flat
        from bialign_amd.verify import rescore_trace
        model, fb = encode_flat(pairs, params)
        mols_a, mols_b = fb.molecules("a"), fb.molecules("b")
    for p, want in enumerate(wants):
        E = he.profile(want["glob"])
        T = spec[2] if thresholds is None else int(thresholds[p])
        np.testing.assert_array_equal(got["profiles"][p].astype(np.int64), E, err_msg=f"pair {p}")
        assert int(got["thresholds"][p]) == T, (p, got["thresholds"], T)
        hp.replay(want["glob"], spec, got["walks"][p], got["hits"][p], got["status"][p], peaks=peaks, threshold=T)
        if peaks:
            is_peak = hp.peaks(E)
            assert all(is_peak[w[0]] for w in got["walks"][p]), p
        hits = got["hits"][p]
        if want["score"] >= T:   # hit 0: the same span, score and trace bytes (the smallest best end is a peak)
            assert bool(complete[p]) and hits, p
            assert hits[0][:3] == (int(start[p]), int(end[p]), int(got["scores"][p])), p
            assert hits[0][3].tobytes() == traces[p].tobytes(), p
        else:
            assert not hits and not got["walks"][p] and got["status"][p] == "exhausted", p
        assert not any(he.meets(a[:2], b[:2]) for x, a in enumerate(hits) for b in hits[x + 1:]), p   # disjoint in B
        for s0, e0, score, trace in hits:
            assert want["glob"][s0, e0] == score, (p, s0, e0)
            if pairs is not None:
                n = len(pairs[p][0])
                total, idx, drift = rescore_trace(trace, mols_a[p][0], mols_a[p][1], mols_b[p][0][s0:e0], mols_b[p][1][s0:e0],
                                                  model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"],
                                                  params["shift_cost"], affine)
                assert total == score and idx == (n, e0 - s0, n, e0 - s0) and drift <= params["max_shift"], (p, s0, e0)


# ---- the peak mask ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", EDGE_COSTS)
def test_mask_word_edges(cost, ref):
    """A of 4 residues against B of 31 .. 127: the ends fill a mask word to its last bit, by one bit more, and two blocks
    of 64.  min_score 1 and a walk per end: the search ends only when every peak at or above 1 was walked."""
    from bialign_amd.batch import make_batch
    params = params_of("protein", cost, 1)
    for m in EDGE_MS:   # a batch each, so that the batch's mask has exactly this pair's words
        pair, want = pair_of("protein", EDGE_N, m, True), ref[("edge", cost, m)]
        spec = (m + 1, m + 1, 1)
        b = make_batch([pair], params, fit=True, hits=dict(max_hits=spec[0], min_score=1, max_walks=spec[1], peaks=True))
        assert b.hit_info()["peaks"] and b.hit_info()["flags"] == 1
        got = run(b)
        b.close()
        check(got, spec, [want], True, pairs=[pair], params=params, affine=cost == "affine")
        assert got["status"][0] == "exhausted"
    pairs = [pair_of("protein", EDGE_N, m, True) for m in EDGE_MS]   # and together: pairs with fewer words than the batch's mask
    spec = (EDGE_MS[-1] + 1, EDGE_MS[-1] + 1, 1)
    b = make_batch(pairs, params, fit=True, hits=dict(max_hits=spec[0], min_score=1, max_walks=spec[1], peaks=True))
    got = run(b)
    b.close()
    check(got, spec, [ref[("edge", cost, m)] for m in EDGE_MS], True, pairs=pairs, params=params, affine=cost == "affine")


@pytest.mark.parametrize("cost,s", main_cases(), ids=lambda v: str(v))
def test_peaks_against_the_oracle(cost, s, ref):
    from bialign_amd.batch import make_batch
    for kind in ("protein", "rna"):
        todo = [c for c in case_pairs(cost, s) if c[0] == kind]
        if not todo:
            continue
        pairs, params = [pair_of(*c) for c in todo], params_of(kind, cost, s)
        wants = [ref[("main", cost, s, *c)] for c in todo]
        spec = (max(c[2] for c in todo) + 1, max(c[2] for c in todo) + 1, half_best(wants))
        b = make_batch(pairs, params, fit=True, hits=dict(max_hits=spec[0], min_score=spec[2], max_walks=spec[1], peaks=True))
        got = run(b)
        check(got, spec, wants, True, pairs=pairs, params=params, affine=b.affine)
        same_results(run(b), got)   # a second run repeats the results
        b.close()


@pytest.mark.parametrize("cost", he.PLANTED_COSTS)
def test_planted_copies_within_the_default_walks(cost, ref):
    """A 22 against B 150 with three copies of A, max_hits 3 and the default max_walks (12): from the peaks, three hits
    that meet the three windows (the condition: tests/test_hit_peaks_host.py); without the flag, what the search gave
    before the flag existed, by replay under the old rule."""
    from bialign_amd.batch import make_batch
    pair, windows, params, _ = he.planted_case(cost)
    want = ref[("planted", cost)]
    n = he.PLANTED["n"]
    spec = he.resolve((3, int(min(want["glob"][w, w + n] for w in windows))))
    b = make_batch([pair], params, fit=True, hits=dict(max_hits=3, min_score=spec[2], peaks=True))
    assert b.hit_info()["max_walks"] == 12
    got = run(b)
    check(got, spec, [want], True, pairs=[pair], params=params, affine=b.affine)
    hits = got["hits"][0]
    assert len(hits) == 3 and got["status"][0] == "max_hits" and len(got["walks"][0]) <= 12
    for w in windows:
        assert sum(he.meets((w, w + n), h[:2]) for h in hits) == 1, (w, hits)
    b.set_hits(3, spec[2], peaks=False)
    assert not b.hit_info()["peaks"] and b.hit_info()["flags"] == 0
    old = run(b)
    b.close()
    he.replay(want["glob"], spec, old["walks"][0], old["hits"][0], old["status"][0])
    check(old, spec, [want], False, pairs=[pair], params=params, affine=b.affine)
    assert old["status"][0] == "max_walks" and len(old["hits"][0]) == 1   # what the peak rule exists for


def test_every_record_form(ref, monkeypatch):
    """The two 101 x 278 pairs of tests/test_gpu_fit_hits.py with the peak rule: packed records on and forced off under
    the forced team shapes.  One set of results, and the oracle's."""
    from bialign_amd.batch import make_batch
    params = params_of("protein", "affine", 1)
    pairs = [pair_of("protein", *TEAM_SHAPE, planted) for planted in (True, False)]
    wants = [ref[("team", planted)] for planted in (True, False)]
    spec = (8, TEAM_SHAPE[1] + 1, half_best(wants))
    base = None
    for pack in ("1", "0"):
        for team in ("1", "3", "x3"):
            monkeypatch.setenv("BIALIGN_TEAM", team)
            monkeypatch.setenv("BIALIGN_PACK", pack)
            b = make_batch(pairs, params, fit=True, hits=dict(max_hits=spec[0], min_score=spec[2], max_walks=spec[1], peaks=True))
            got = run(b)
            b.close()
            t = got["timing"]
            assert t["cross_cu"] == (team == "x3") and t["packed_records"] == (pack == "1"), t
            if base is None:
                base = got
                check(got, spec, wants, True, pairs=pairs, params=params, affine=True)
            same_results(got, base)
            np.testing.assert_array_equal(got["thresholds"], base["thresholds"])


# ---- thresholds -------------------------------------------------------------------------------------------------------

def ragged(ref):
    pairs = [pair_of(*c) for c in RAGGED]
    wants = [ref[("main", "affine", 1, *c)] for c in RAGGED]
    return pairs, wants, params_of("protein", "affine", 1)


def formula(wants, base, permille):
    return [hp.threshold(he.profile(w["glob"]), base[p], permille) for p, w in enumerate(wants)]


@pytest.mark.parametrize("peaks", [False, True])
def test_thresholds_per_pair(peaks, ref):
    """A ragged batch launched in another order than it was given, in one chunk and in several: every pair is searched
    with its own T_p, one of them above its Emax (no walk, EXHAUSTED)."""
    from bialign_amd.batch import make_batch
    pairs, wants, params = ragged(ref)
    emax = [w["score"] for w in wants]
    assert all(e > 3 for e in emax[1:])
    base = [1, emax[1] + 1, emax[2] // 2, emax[3] // 3]
    spec = (98, 98, 7)   # (min_score 7: the array stands in its place)
    hits = dict(max_hits=spec[0], min_score=spec[2], max_walks=spec[1], peaks=peaks)
    roomy = make_batch(pairs, params, fit=True, hits=dict(hits, min_scores=base))
    array_bytes = roomy.hit_info()["buffer_bytes"]
    np.testing.assert_array_equal(roomy.hit_thresholds(), [-1] * 4)   # no run yet
    one = run(roomy)
    one_chunk = roomy.info["hbm_layer_bytes"]
    check(one, spec, wants, peaks, formula(wants, base, 0), pairs, params, True)
    assert one["status"][1] == "exhausted" and not one["walks"][1] and len(one["hits"][3]) >= 1

    # min_permille together with the array, and alone; a re-run keeps them
    roomy.set_hits(**hits, min_scores=base, min_permille=600)
    both = run(roomy)
    T = formula(wants, base, 600)
    assert T[1] == base[1] and T[2] == -(-600 * emax[2] // 1000) and T != formula(wants, base, 0)
    check(both, spec, wants, peaks, T, pairs, params, True)
    same_results(run(roomy), both)
    np.testing.assert_array_equal(roomy.hit_thresholds(), T)
    roomy.set_hits(**hits, min_permille=1000)
    alone = run(roomy)
    check(alone, spec, wants, peaks, formula(wants, [spec[2]] * 4, 1000), pairs, params, True)
    assert all(h and h[0][2] == e for h, e in zip(alone["hits"], emax) if e >= spec[2])

    # the array's bytes count; a second set_hits clears the thresholds
    no_array = make_batch(pairs, params, fit=True, hits=hits)
    assert array_bytes == no_array.hit_info()["buffer_bytes"] + 4 * len(pairs)
    no_array.close()
    roomy.set_hits(**hits)
    cleared = run(roomy)
    check(cleared, spec, wants, peaks, [spec[2]] * 4, pairs, params, True)

    # a fill-only run: the profile, NOT_SEARCHED, thresholds -1
    roomy.set_hits(**hits, min_scores=base, min_permille=600)
    roomy.run(fill_only=True)
    np.testing.assert_array_equal(roomy.hit_thresholds(), [-1] * 4)
    assert roomy.fit_hits() == ([[]] * 4, ["not_searched"] * 4) and roomy.fit_hit_walks() == [[]] * 4
    for p, w in enumerate(wants):
        np.testing.assert_array_equal(roomy.hit_profile(p).astype(np.int64), he.profile(w["glob"]))
    roomy.close()

    b = make_batch(pairs, params, fit=True, hbm_budget_bytes=int(one_chunk * 0.6), hits=dict(hits, min_scores=base))
    assert b.current_info()["nchunks"] > 1
    several = run(b)
    b.close()
    same_results(several, one)
    np.testing.assert_array_equal(several["thresholds"], one["thresholds"])


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_batch_usable(monkeypatch):
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch
    lib = _lib.lib
    b = make_batch([FORM_PAIR], FORM_PARAMS, fit=True)
    b.run()
    score = int(b.scores()[0])
    one = np.array([5], dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib.c_i32p)
    assert lib.bialign_batch_set_hit_thresholds(b._h, ptr(one), 0) == _lib.E_INVALID       # no search set
    assert lib.bialign_batch_get_hit_thresholds(b._h, ptr(one)) == _lib.E_INVALID
    b.run()
    assert int(b.scores()[0]) == score
    for flags in (2, 3, 1 << 31 - 1, -2):   # past Python's own check: the library's
        spec = _lib.HitSpec(3, 0, 100, flags)
        assert lib.bialign_batch_set_hits(b._h, ctypes.byref(spec)) == _lib.E_INVALID, flags
        b.run()
        assert int(b.scores()[0]) == score
    b.set_hits(3, 100, peaks=True)
    b.run()
    before = (b.fit_hits(), b.hit_thresholds().tolist())
    assert before[1] == [100]
    for arr, permille in ((None, 1001), (None, -1), (np.array([0], dtype=np.int32), 0), (np.array([-7], dtype=np.int32), 500)):
        rc = lib.bialign_batch_set_hit_thresholds(b._h, None if arr is None else ptr(arr), permille)
        assert rc == _lib.E_INVALID, (arr, permille)
        b.run()   # the search it had, with the thresholds it had
        after = (b.fit_hits(), b.hit_thresholds().tolist())
        assert after[1] == before[1] and after[0][1] == before[0][1]
        assert [h[:3] for h in after[0][0][0]] == [h[:3] for h in before[0][0][0]]
    monkeypatch.setenv("BIALIGN_TEST_FAIL_HITS_ALLOC", "1")
    assert lib.bialign_batch_set_hit_thresholds(b._h, ptr(one), 0) == _lib.E_NOMEM
    monkeypatch.delenv("BIALIGN_TEST_FAIL_HITS_ALLOC")
    b.run()
    assert b.hit_thresholds().tolist() == [100]
    assert lib.bialign_batch_set_hit_thresholds(b._h, ptr(one), 0) == 0
    b.run()
    assert b.hit_thresholds().tolist() == [5]
    b.close()


# ---- significance -----------------------------------------------------------------------------------------------------

def test_hit_significance(ref):
    from bialign_amd import significance as sg
    from bialign_amd.batch import make_batch
    pair, windows, params, _ = he.planted_case("affine")
    want = ref[("planted", "affine")]
    spec = he.resolve((3, int(min(want["glob"][w, w + he.PLANTED["n"]] for w in windows))))
    b = make_batch([pair], params, fit=True, hits=dict(max_hits=3, min_score=spec[2], peaks=True))
    b.run()
    hits = b.fit_hits()[0]
    got = sg.hit_significance(b, [pair], params, replicas=16, seed=11)
    b.close()
    assert len(got) == 1 and len(got[0]) == len(hits[0]) == 3
    z = sg.zscores([pair], params, replicas=16, seed=11, fit=True)
    assert got[0][0]["score"] == int(z["score"][0]) == want["score"]
    assert got[0][0]["z"] == z["z"][0] and got[0][0]["p_emp"] == z["p_emp"][0]
    nb = sg.null_batch([pair], params, 16, seed=11, fit=True)
    nb.run()
    replica = nb.null_scores()[0].astype(np.int64)
    stats = nb.null_stats()
    nb.close()
    zs = sg.hit_zscores(hits, stats)[0]
    for h, (hit, sig) in enumerate(zip(hits[0], got[0])):
        assert sig["score"] == hit[2] and sig["replicas"] == 16
        assert sig["n_ge"] == int((replica >= hit[2]).sum()) and sig["p_emp"] == (sig["n_ge"] + 1) / 17, h
        assert sig["z"] == zs[h] and abs(zs[h] - (hit[2] - replica.mean()) / replica.std(ddof=1)) < 1e-9, h
