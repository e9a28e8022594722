"""The hit search of FIT batches (include/bialign.h, "Hit search") on the GPU against tests/hits_expected.py: the profile
is the oracle's bit for bit, and the walk log replays, step by step, as the greedy loop the model prescribes.

The oracle runs of every case of this module are made once, in one spawn pool (``ref``), and shared."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_expected as fe
import free_ends_gpu as fg
import hits_expected as he
from bialign_amd import synth
from free_ends_gpu import feature_mu2, pad, params_of, seq_mu1

pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 2, 3, 5)
SHAPES = [(22, 50), (50, 97), (1, 50)]   # FIT's own: one strip and three at max_shift 1, and a one-residue A
TEAM_SHAPE = (101, 278)                  # the smallest shape that admits a team of three waves (tests/test_gpu_fit.py)
pair_of = fg.pair_of(fe.make_pair, 9000)

FORM_PARAMS = dict(synth.PROTEIN_PARAMS)
FORM_PAIR = fe.make_pair("protein", 4242, 22, 50, True)
feature_molecules = lambda: fg.feature_molecules(77, (20, 47))
form_tables = lambda: fg.form_tables(FORM_PAIR, FORM_PARAMS)


def main_cases():
    return [(cost, s) for cost in ("affine", "one-layer") for s in SHIFTS] + [("beta>0", 1)]


def case_pairs(cost, s):
    """[(kind, n, m, planted)]: per shape a planted protein pair, and up to max_shift 2 (where the oracle is cheap for RNA,
    as in tests/test_gpu_fit.py) a plain RNA pair."""
    out = [("protein", n, m, True) for n, m in SHAPES]
    if s <= 2 and cost != "beta>0":
        out += [("rna", n, m, False) for n, m in SHAPES]
    return out


@pytest.fixture(scope="module")
def ref():
    """{key: fit_expected's dict} for every pair of this module."""
    cases = {}
    for cost, s in main_cases():
        for kind, n, m, planted in case_pairs(cost, s):
            prm = params_of(kind, cost, s)
            cases[("main", cost, s, kind, n, m, planted)] = (n, m, prm, *fe.tables_of(pair_of(kind, n, m, planted), prm), False)
    prm = params_of("protein", "affine", 1)
    for planted in (True, False):
        cases[("team", planted)] = (*TEAM_SHAPE, prm, *fe.tables_of(pair_of("protein", *TEAM_SHAPE, planted), prm), False)
    for cost in he.PLANTED_COSTS:
        cases[("planted", cost)] = he.planted_case(cost)[3]
    mu1, mu2, d1, d2 = form_tables()
    cases[("form", "mu1")] = (22, 50, FORM_PARAMS, pad(d1), mu2, False)
    cases[("form", "mu2")] = (22, 50, FORM_PARAMS, mu1, pad(d2), False)
    mols = feature_molecules()
    fprm = dict(synth.RNA_PARAMS)
    cases[("form", "feature")] = (20, 47, fprm, seq_mu1(mols[0][0], mols[1][0], fprm),
                                  feature_mu2(mols[0][1], mols[1][1], fprm["structure_weight"]), False)
    return fe.expected_many(cases)


def half_best(wants):
    """A min_score from the oracle alone: half the smallest fit score of the batch's pairs (at least 1)."""
    return max(1, min(w["score"] for w in wants) // 2)


def search(b):
    """One run of a batch with a search set -> dict of everything the run left."""
    b.run()
    hits, status = b.fit_hits()
    return dict(scores=b.scores().copy(), spans=b.fit_spans(), traces=b.traces(), hits=hits, status=status,
                walks=b.fit_hit_walks(), profiles=[b.hit_profile(p) for p in range(b.npairs)], timing=b.timing(),
                info=b.hit_info())


def same_results(got, base):
    assert got["status"] == base["status"] and got["walks"] == base["walks"]
    for gp, bp in zip(got["profiles"], base["profiles"]):
        np.testing.assert_array_equal(gp, bp)
    for gh, bh in zip(got["hits"], base["hits"]):
        assert [h[:3] for h in gh] == [h[:3] for h in bh]
        for x, y in zip(gh, bh):
            np.testing.assert_array_equal(x[3], y[3])


def check_against_oracle(got, spec, wants, pairs=None, params=None, affine=None):
    """Every pair: the profile is the oracle's, the log replays, hit 0 is the batch's own alignment, and (``pairs`` given:
    LOOKUP scores) every hit's trace, re-scored on B[start:end], gives its score.  (Affine: search and traceback kernel
    call one walk, walk_affine, so hit 0's comparison holds the search's end choice and start state to the kernel's.
    One-layer: traceback_linear_kernel keeps a copy of walk_linear's column loop, and hit 0 == the batch's trace is what
    ties that copy to the function the search calls.  The walks' rules themselves are held to the oracle by the traces of
    tests/test_gpu_fit.py and the other modes' tests.)"""
    start, end = got["spans"]
    traces, complete = got["traces"]
    if pairs is not None:
        from bialign_amd.batch import encode_flat
        from bialign_amd.verify import rescore_trace
        model, fb = encode_flat(pairs, params)
        mols_a, mols_b = fb.molecules("a"), fb.molecules("b")
    for p, want in enumerate(wants):
        np.testing.assert_array_equal(got["profiles"][p].astype(np.int64), he.profile(want["glob"]), err_msg=f"pair {p}")
        he.replay(want["glob"], spec, got["walks"][p], got["hits"][p], got["status"][p])
        hits = got["hits"][p]
        if want["score"] >= spec[2]:   # hit 0: the same span, score and trace bytes
            assert bool(complete[p]) and hits, p
            assert hits[0][:3] == (int(start[p]), int(end[p]), int(got["scores"][p])), p
            assert hits[0][3].tobytes() == traces[p].tobytes(), p
        else:
            assert not hits and not got["walks"][p], p
        assert all(a[2] >= b[2] for a, b in zip(hits, hits[1:])), p      # scores do not increase
        assert not any(he.meets(a[:2], b[:2]) for x, a in enumerate(hits) for b in hits[x + 1:]), p   # disjoint in B
        for s0, e0, score, trace in hits:
            assert want["glob"][s0, e0] == score, (p, s0, e0)
            if pairs is not None:
                n = len(pairs[p][0])
                total, idx, drift = rescore_trace(trace, mols_a[p][0], mols_a[p][1], mols_b[p][0][s0:e0], mols_b[p][1][s0:e0],
                                                  model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"],
                                                  params["shift_cost"], affine)
                assert total == score and idx == (n, e0 - s0, n, e0 - s0) and drift <= params["max_shift"], (p, s0, e0)


# ---- profile, log and hits against the oracle -------------------------------------------------------------------------

@pytest.mark.parametrize("cost,s", main_cases(), ids=lambda v: str(v))
def test_search_against_the_oracle(cost, s, ref):
    """max_hits = max_walks = m + 1 of the longest B, a walk per end: a search ends exhausted unless every end was walked.
    min_score: half the smallest fit score of the batch."""
    from bialign_amd.batch import make_batch
    for kind in ("protein", "rna"):
        todo = [c for c in case_pairs(cost, s) if c[0] == kind]
        if not todo:
            continue
        pairs, params = [pair_of(*c) for c in todo], params_of(kind, cost, s)
        wants = [ref[("main", cost, s, *c)] for c in todo]
        spec = (max(c[2] for c in todo) + 1, max(c[2] for c in todo) + 1, half_best(wants))
        b = make_batch(pairs, params, fit=True, hits=(spec[0], spec[2], spec[1]))
        got = search(b)
        assert got["info"]["max_walks"] == spec[1] and got["info"]["buffer_bytes"] > 0 and got["info"]["search_ms"] > 0
        check_against_oracle(got, spec, wants, pairs, params, b.affine)
        assert "exhausted" in got["status"]
        same_results(search(b), got)   # a second run repeats the results
        b.close()


@pytest.mark.parametrize("cost", he.PLANTED_COSTS)
def test_planted_copies_are_found(cost, ref):
    """A 22 against B 150 with three copies of A (the inputs' condition: tests/test_fit_hits_host.py): exactly three
    hits, one per planted window."""
    from bialign_amd.batch import make_batch
    pair, windows, params, _ = he.planted_case(cost)
    want = ref[("planted", cost)]
    spec = he.planted_spec(want["glob"], windows)
    b = make_batch([pair], params, fit=True, hits=(spec[0], spec[2], spec[1]))
    got = search(b)
    check_against_oracle(got, spec, [want], [pair], params, b.affine)
    b.close()
    hits = got["hits"][0]
    assert len(hits) == he.PLANTED["copies"] and got["status"][0] == "exhausted"
    for w in windows:
        assert sum(he.meets((w, w + he.PLANTED["n"]), h[:2]) for h in hits) == 1, (w, hits)


def test_stop_reasons(ref):
    """max_hits = 1: MAX_HITS with hit 0 alone.  max_walks = max_hits = 2 on the pairs for which the oracle says, under
    either start rule, that the second walk runs into the first hit: MAX_WALKS.  A min_score above the best score:
    EXHAUSTED without a walk."""
    from bialign_amd.batch import make_batch
    todo = [c for c in case_pairs("affine", 1) if c[0] == "protein"] + [c for c in case_pairs("one-layer", 1) if c[0] == "protein"]
    keys = [("main", "affine", 1, *c) for c in todo[:3]] + [("main", "one-layer", 1, *c) for c in todo[3:]]
    seen = set()
    for cost in ("affine", "one-layer"):
        part = [(c, k) for c, k in zip(todo, keys) if k[1] == cost]
        pairs, params = [pair_of(*c) for c, _ in part], params_of("protein", cost, 1)
        wants = [ref[k] for _, k in part]
        b = make_batch(pairs, params, fit=True)
        for spec in ((1, 1, half_best(wants)), (2, 2, half_best(wants)), (3, 12, max(w["score"] for w in wants) + 1)):
            b.set_hits(spec[0], spec[2], spec[1] if spec[1] != 12 else 0)   # (0: 4 * max_hits)
            got = search(b)
            check_against_oracle(got, spec, wants, pairs, params, b.affine)
            for p, want in enumerate(wants):
                if spec[0] == 1:
                    assert got["status"][p] == "max_hits" and len(got["hits"][p]) == 1
                elif spec[0] == 3:
                    assert got["status"][p] == "exhausted" and not got["hits"][p] and not got["walks"][p]
                elif all(he.greedy(want["glob"], spec, rule)[2] == "max_walks" for rule in (min, max)):
                    assert got["status"][p] == "max_walks" and len(got["hits"][p]) == 1
                    seen.add(cost)
        b.close()
    assert seen, "no input whose second walk is discarded: MAX_WALKS was not reached"


# ---- every record form, chunks, forms of the scores ------------------------------------------------------------------

def test_every_record_form(ref, monkeypatch):
    """Two pairs long enough for a team of three, max_shift 1, affine: packed records on and forced off under the forced
    team shapes; timing() says which sweep ran.  One set of results, and the oracle's."""
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
            b = make_batch(pairs, params, fit=True, hits=(spec[0], spec[2], spec[1]))
            got = search(b)
            b.close()
            t = got["timing"]
            slim = team == "3" and pack == "1"
            assert t["waves_per_pair"] == (1 if team == "1" else (3 if slim or team == "x3" else 2)), t
            assert t["cross_cu"] == (team == "x3") and t["packed_records"] == (pack == "1"), t
            if base is None:
                base = got
                check_against_oracle(got, spec, wants, pairs, params, True)
            same_results(got, base)


def test_replanned_run_after_a_packed_overflow(monkeypatch):
    """Costs under which the packed records' 16-bit offsets overflow: the run is repeated with full records, re-planned
    into other chunks, and the search with it.  The results are those of a batch that never packed."""
    from bialign_amd.batch import make_batch
    params = dict(synth.PROTEIN_PARAMS, simmatrix=None, sequence_match_similarity=5000, sequence_mismatch_similarity=-5000,
                  structure_weight=100, gap_opening_cost=-5000, gap_cost=-5000, shift_cost=-5000)
    pairs = [fe.make_pair("protein", 4800 + t, 60 + 9 * t, 170 - 3 * t, True) for t in range(4)]   # planted: placements exist
    monkeypatch.setenv("BIALIGN_PACK", "0")
    plain = make_batch(pairs, params, fit=True, hits=(4, 1, 40))
    base = search(plain)
    plain.close()
    monkeypatch.setenv("BIALIGN_PACK", "1")
    probe = make_batch(pairs, params, fit=True)
    one_chunk = probe.info["hbm_layer_bytes"]
    probe.close()
    b = make_batch(pairs, params, fit=True, hbm_budget_bytes=int(one_chunk * 0.6), hits=(4, 1, 40))
    assert b.info["nchunks"] >= 2
    got = search(b)
    b.close()
    assert got["timing"]["recovered_runs"] == 1 and not got["timing"]["packed_records"], got["timing"]
    assert not base["timing"]["packed_records"]
    same_results(got, base)
    assert any(len(h) >= 1 for h in got["hits"])


def test_chunks(ref):
    """Four pairs under a budget that cuts the batch into chunks: every chunk is searched while its layers are resident."""
    from bialign_amd.batch import make_batch
    todo = [c for c in case_pairs("affine", 1) if c[0] == "protein"]
    pairs = [pair_of(*c) for c in todo] + [pair_of(*todo[1])]
    wants = [ref[("main", "affine", 1, *c)] for c in todo] + [ref[("main", "affine", 1, *todo[1])]]
    params = params_of("protein", "affine", 1)
    spec = (98, 98, half_best(wants))
    roomy = make_batch(pairs, params, fit=True, hits=(spec[0], spec[2], spec[1]))
    base = search(roomy)
    one_chunk = roomy.info["hbm_layer_bytes"]
    roomy.close()
    check_against_oracle(base, spec, wants, pairs, params, True)
    b = make_batch(pairs, params, fit=True, hbm_budget_bytes=int(one_chunk * 0.45), hits=(spec[0], spec[2], spec[1]))
    assert b.current_info()["nchunks"] > 1
    same_results(search(b), base)
    b.close()


@pytest.mark.parametrize("form", ["mu1", "mu2", "feature"])
def test_forms_of_the_scores(form, ref):
    from bialign_amd.batch import make_batch, make_feature_batch
    want = ref[("form", form)]
    spec = (51, 51, half_best([want]))
    if form == "feature":
        b = make_feature_batch(feature_molecules(), [(0, 1)], dict(synth.RNA_PARAMS), fit=True)
    else:
        _, _, d1, d2 = form_tables()
        b = make_batch([FORM_PAIR], FORM_PARAMS, fit=True, **(dict(mu1_dense=[d1]) if form == "mu1" else dict(mu2_dense=[d2])))
    b.set_hits(spec[0], spec[2], spec[1])
    got = search(b)
    b.close()
    check_against_oracle(got, spec, [want])


# ---- refusals and state -----------------------------------------------------------------------------------------------

def test_set_hits_refusals():
    from bialign_amd import _lib
    from bialign_amd import significance as sg
    from bialign_amd.batch import make_batch
    for make in (lambda: make_batch([FORM_PAIR], FORM_PARAMS), lambda: make_batch([FORM_PAIR], FORM_PARAMS, local=True),
                 lambda: make_batch([FORM_PAIR], FORM_PARAMS, fit=True, score_only=True),
                 lambda: sg.null_batch([FORM_PAIR], FORM_PARAMS, 4, seed=5, fit=True)):
        b = make()
        with pytest.raises(_lib.BialignError) as err:
            b.set_hits(3, 100)
        assert err.value.code == _lib.E_UNSUPPORTED and "FIT" in err.value.message and "full storage" in err.value.message
        b.run()   # the batch is what it was
        b.close()
    b = make_batch([FORM_PAIR], FORM_PARAMS, fit=True)
    for bad in ((0, 0, 100), (257, 0, 100), (3, 0, 0), (4, 3, 100)):   # past Python's own check: the library's
        spec = _lib.HitSpec(bad[0], bad[1], bad[2], 0)
        assert _lib.lib.bialign_batch_set_hits(b._h, ctypes.byref(spec)) == _lib.E_INVALID, bad
    with pytest.raises(ValueError, match="no hit search"):
        b.fit_hits()
    b.close()


def test_allocation_failure_leaves_the_batch_usable(monkeypatch):
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch
    b = make_batch([FORM_PAIR], FORM_PARAMS, fit=True)
    b.run()
    score = int(b.scores()[0])
    monkeypatch.setenv("BIALIGN_TEST_FAIL_HITS_ALLOC", "1")
    with pytest.raises(_lib.BialignError) as err:
        b.set_hits(3, 100)
    assert err.value.code == _lib.E_NOMEM
    monkeypatch.delenv("BIALIGN_TEST_FAIL_HITS_ALLOC")
    b.run()
    assert int(b.scores()[0]) == score
    info = _lib.HitInfo()
    assert _lib.lib.bialign_batch_get_hit_info(b._h, ctypes.byref(info)) == _lib.E_INVALID   # no search is set
    b.set_hits(3, 100)
    b.run()
    assert b.fit_hits()[1][0] in ("exhausted", "max_hits", "max_walks")
    b.close()


def test_run_rules(ref):
    """Getters ahead of a run; a fill-only run; an async run; taking the search away again."""
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch
    c = ("protein", 22, 50, True)
    pair, params, want = pair_of(*c), params_of("protein", "affine", 1), ref[("main", "affine", 1, *c)]
    spec = (4, 16, half_best([want]))
    plain = make_batch([pair], params, fit=True)
    plain.run()
    plain_results = (plain.scores().copy(), plain.fit_spans(), plain.traces())
    b = make_batch([pair], params, fit=True, hits=(spec[0], spec[2]))
    assert b.hit_info()["max_walks"] == 16 and b.hit_info()["search_ms"] == 0
    with pytest.raises(_lib.BialignError) as err:
        b.fit_hits()
    assert err.value.code == _lib.E_INVALID
    b.run(fill_only=True)   # the profile, and nothing searched
    np.testing.assert_array_equal(b.hit_profile(0).astype(np.int64), he.profile(want["glob"]))
    assert b.fit_hits() == ([[]], ["not_searched"]) and b.fit_hit_walks() == [[]]
    b.run(wait=False)       # a getter completes an async run
    hits, status = b.fit_hits()
    got = dict(scores=b.scores().copy(), spans=b.fit_spans(), traces=b.traces(), hits=hits, status=status,
               walks=b.fit_hit_walks(), profiles=[b.hit_profile(0)])
    check_against_oracle(got, spec, [want], [pair], params, True)
    for x, y in zip((got["scores"], *got["spans"]), (plain_results[0], *plain_results[1])):   # the batch's own results: untouched
        np.testing.assert_array_equal(x, y)
    assert got["traces"][0][0].tobytes() == plain_results[2][0][0].tobytes()
    b.set_hits(None)        # the plain run again
    b.run()
    np.testing.assert_array_equal(b.scores(), plain_results[0])
    assert b.traces()[0][0].tobytes() == plain_results[2][0][0].tobytes()
    with pytest.raises(ValueError, match="no hit search"):
        b.hit_profile(0)
    out = np.empty(51, dtype=np.int32)
    assert _lib.lib.bialign_batch_get_hit_profile(b._h, 0, out.ctypes.data_as(_lib.c_i32p)) == _lib.E_INVALID
    b.close()
    plain.close()
