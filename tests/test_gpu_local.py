"""Local alignments (BIALIGN_BATCH_LOCAL) on the GPU against tests/local_expected.py: one oracle fill per start
(i0, j0) gives every window's global score, hence the local score, the smallest best end, and the LOCAL layers.

The oracle runs of every case of this module are made once, in one spawn pool (``ref``), and shared.

Shapes: per max_shift the rows span three strips (n = 2 RR + 4: 130, 44, 26, 20, 12 at max_shift 0, 1, 2, 3, 5), m = 41
is five 8-column ghost blocks with interior and boundary steps; beside them n = 1 and m = 7 < n.

Oracle cost: one expectation is about W^2 n^2 m^2 / 4 band cells -- 5 to 7.4 M at every max_shift's large shape -- at
about 0.6 M cells per second and core in the affine recurrence, a fifteenth of that in the one-layer one.  Two pairs per
large shape, five bands: 10 affine expectations of 8..12 s, 10 one-layer ones of under 1 s, the small shapes, forms and
null replicas another 20 s: about 150 core-seconds, 10 to 20 s of wall time in a pool of 16.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_expected as le
import free_ends_gpu as fg
from bialign_amd import significance as sg
from bialign_amd import synth
from free_ends_gpu import feature_mu2, pad, params_of, seq_mu1, stats_of

pytestmark = pytest.mark.gpu

SHIFTS, M_LONG, M_SHORT = (0, 1, 2, 3, 5), 41, 7
# max_shift 2: a team of four waves needs eight strips and a column period of 280 -- the smallest such shape
TEAM_SHAPE, TEAM_SHIFT, TEAM_SIZES = (101, 278), 2, (1, 4)
NULL_R, NULL_SEED = 3, 5


def rows_of(s):
    """Rows that span three strips: a strip has RR = 64 // (2 s + 1) - 1 rows."""
    return 2 * (64 // (2 * s + 1) - 1) + 4


def shapes_of(s):
    return [(rows_of(s), M_LONG), (1, M_LONG), (rows_of(s), M_SHORT)]


pair_of = fg.pair_of(le.make_pair, 9000)


def case_pairs(s):
    """[(kind, n, m, planted)] of one max_shift: per shape a planted protein pair (whose layers are compared; n = 1 has no
    room for flanks: a plain one) and a plain RNA pair."""
    return [c for n, m in shapes_of(s) for c in (("protein", n, m, True), ("rna", n, m, False))]


def main_cases():
    return [(cost, s) for cost in ("affine", "one-layer") for s in SHIFTS]


FORM_PARAMS = dict(synth.PROTEIN_PARAMS)
FORM_SHAPE = (22, 30)
FORM_PAIR = le.make_pair("protein", 4242, *FORM_SHAPE, True)
NULL_PAIRS = [le.make_pair("protein", 4300, 14, 24, True), le.make_pair("protein", 4301, 11, 19, False)]
feature_molecules = lambda: fg.feature_molecules(78, (16, 30))
form_tables = lambda: fg.form_tables(FORM_PAIR, FORM_PARAMS)


@pytest.fixture(scope="module")
def ref():
    """{key: local_expected's dict} for every pair of this module, and under ``("tables", key)`` the case's tables."""
    cases = {}
    for cost, s in main_cases():
        for kind, n, m, planted in case_pairs(s):
            prm = params_of(kind, cost, s)
            mu1, mu2 = le.tables_of(pair_of(kind, n, m, planted), prm)
            cases[("main", cost, s, kind, n, m, planted)] = (n, m, prm, mu1, mu2, planted)
    mu1, mu2, d1, d2 = form_tables()
    cases[("form", "mu1")] = (*FORM_SHAPE, FORM_PARAMS, pad(d1), mu2, False)
    cases[("form", "mu2")] = (*FORM_SHAPE, FORM_PARAMS, mu1, pad(d2), False)
    mols = feature_molecules()
    fprm = dict(synth.RNA_PARAMS)
    nf, mf = len(mols[0][0]), len(mols[1][0])
    cases[("form", "feature")] = (nf, mf, fprm, seq_mu1(mols[0][0], mols[1][0], fprm),
                                  feature_mu2(mols[0][1], mols[1][1], fprm["structure_weight"]), False)
    for p, pair in enumerate(NULL_PAIRS):   # observed pairs and their replicas, as the host shuffles them
        cases[("null", p, None)] = (len(pair[0]), len(pair[1]), FORM_PARAMS, *le.tables_of(pair, FORM_PARAMS), False)
        for r in range(NULL_R):
            cases[("null", p, r)] = (len(pair[0]), len(pair[1]), FORM_PARAMS,
                                     *le.tables_of(sg.shuffle_b(pair, NULL_SEED, p, r), FORM_PARAMS), False)
    for r in range(NULL_R):
        seq_b, feats_b = sg.shuffle_features(mols[1][0], mols[1][1], NULL_SEED, 0, r)
        cases[("null-feature", r)] = (nf, mf, fprm, seq_mu1(mols[0][0], seq_b, fprm),
                                      feature_mu2(mols[0][1], feats_b, fprm["structure_weight"]), False)
        cases[("null-dense", r)] = (*FORM_SHAPE, FORM_PARAMS, pad(sg.shuffle_tables(d1, NULL_SEED, 0, r)),
                                    pad(sg.shuffle_tables(d2, NULL_SEED, 0, r)), False)
    out = le.expected_many(cases)
    out.update({("tables", key): (c[2], c[3], c[4]) for key, c in cases.items()})
    return out


def run_local(pairs, params, **kw):
    """A LOCAL batch of ``pairs`` -> dict of its results (full storage: traces and spans of the walk too)."""
    from bialign_amd.batch import make_batch
    b = make_batch(pairs, params, local=True, **kw)
    b.run()
    out = dict(scores=b.scores().copy(), spans=b.local_spans(), timing=b.timing(), affine=b.affine, batch=b)
    if not kw.get("score_only"):
        out["traces"], out["complete"] = b.traces()
    return out


def check_ends(got, wants):
    assert [int(x) for x in got["scores"]] == [w["score"] for w in wants]
    assert [(int(a), int(b)) for a, b in zip(got["spans"][1], got["spans"][3])] == [w["end"] for w in wants]


def check_walks(got, pairs, params, wants, tables):
    """Every pair of a full-storage LOCAL batch: score, smallest best end, and the walk -- complete, its window one that
    attains the maximum, its columns re-scored on the two windows give the score."""
    from bialign_amd.batch import encode_flat
    from bialign_amd.verify import rescore_trace
    model, fb = encode_flat(pairs, params)
    mols_a, mols_b = fb.molecules("a"), fb.molecules("b")
    check_ends(got, wants)
    for p, want in enumerate(wants):
        n, m = len(pairs[p][0]), len(pairs[p][1])
        assert bool(got["complete"][p]), p
        sa, ea, sb, eb = span = tuple(int(x[p]) for x in got["spans"])
        assert 0 <= sa <= ea <= n and 0 <= sb <= eb <= m, (p, span)
        assert le.span_score(want, *tables[p], span) == want["score"], (p, span)
        total, idx, drift = rescore_trace(got["traces"][p], mols_a[p][0][sa:ea], mols_a[p][1][sa:ea], mols_b[p][0][sb:eb], mols_b[p][1][sb:eb],
                                          model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"], params["shift_cost"],
                                          got["affine"])
        assert total == want["score"] and idx == (ea - sa, eb - sb, ea - sa, eb - sb) and drift <= params["max_shift"], p


# ---- the inputs: windows inside both molecules occur -------------------------------------------------------------------

def test_planted_pairs_have_inner_windows(ref):
    """A condition on the inputs, from the helper alone: for at least half of the planted pairs (all of them but n = 1,
    which has no room for flanks) the best window ends before both molecules' ends and no window that starts at a first
    residue attains the score there -- start_a > 0, end_a < n, start_b > 0, end_b < m.  Otherwise the mode could not be
    told from FIT or global."""
    for cost, s in main_cases():
        planted = [c for c in case_pairs(s) if c[3]]
        inner = [ref[("main", cost, s, *c)]["inner"] for c in planted]
        assert 2 * sum(inner) >= len(planted), (cost, s, inner)
        assert all(inner[x] for x, c in enumerate(planted) if c[1] > 1), (cost, s, inner)
        assert all(ref[("main", cost, s, *c)]["score"] >= 0 for c in case_pairs(s))


# ---- scores, spans, walks and layers -----------------------------------------------------------------------------------

@pytest.mark.parametrize("cost,s", main_cases(), ids=lambda v: str(v))
def test_full_storage_against_the_oracle(cost, s, ref):
    for kind in ("protein", "rna"):
        todo = [c for c in case_pairs(s) if c[0] == kind]
        pairs = [pair_of(*c) for c in todo]
        params = params_of(kind, cost, s)
        wants = [ref[("main", cost, s, *c)] for c in todo]
        got = run_local(pairs, params)
        check_walks(got, pairs, params, wants, [ref[("tables", ("main", cost, s, *c))] for c in todo])
        for p, (c, want) in enumerate(zip(todo, wants)):   # the planted pairs: the LOCAL layers
            if want["layers"] is not None:
                le.compare_layers(got["batch"].dump_layers(p).astype(np.int64), want["layers"], c[1], c[2], s)
        # the dump re-ran a sweep: scores and spans stay; a fill-only run leaves the scores and the ends, and no start
        np.testing.assert_array_equal(got["batch"].scores(), got["scores"])
        for x, y in zip(got["batch"].local_spans(), got["spans"]):
            np.testing.assert_array_equal(x, y)
        got["batch"].run(fill_only=True)
        np.testing.assert_array_equal(got["batch"].scores(), got["scores"])
        start_a, end_a, start_b, end_b = got["batch"].local_spans()
        assert (start_a == -1).all() and (start_b == -1).all()
        np.testing.assert_array_equal(end_a, got["spans"][1])
        np.testing.assert_array_equal(end_b, got["spans"][3])
        got["batch"].close()


@pytest.mark.parametrize("cost,s", main_cases(), ids=lambda v: str(v))
def test_score_only_against_the_oracle_and_full_storage(cost, s, ref):
    """The LEAN sweeps fold the same keys: scores and ends as the oracle's, hence as full storage's; no starts."""
    for kind in ("protein", "rna"):
        todo = [c for c in case_pairs(s) if c[0] == kind]
        got = run_local([pair_of(*c) for c in todo], params_of(kind, cost, s), score_only=True)
        got["batch"].close()
        check_ends(got, [ref[("main", cost, s, *c)] for c in todo])
        assert (got["spans"][0] == -1).all() and (got["spans"][2] == -1).all()


# ---- teams ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", ["affine", "one-layer"])
def test_teams_agree_with_the_one_wave_sweep(cost, monkeypatch):
    """Two pairs of a team's smallest shape under every team size of the LOCAL plan, full storage and score-only: scores,
    spans and one pair's dumped layers bit for bit those of the one-wave launch.  An exact expectation is out of reach at
    this shape (about 10^9 band cells); each score is bounded from below by one oracle run of the returned windows, which
    must equal it.  That no better window exists at this shape rests on the one-wave kernel's oracle checks at the small
    shapes above."""
    from bialign_amd.batch import make_batch
    params = params_of("protein", cost, TEAM_SHIFT)
    pairs = [pair_of("protein", *TEAM_SHAPE, planted) for planted in (True, False)]
    base = None
    for team in TEAM_SIZES:
        monkeypatch.setenv("BIALIGN_TEAM", str(team))
        got = run_local(pairs, params)
        assert got["timing"]["waves_per_pair"] == team and not got["timing"]["cross_cu"] and not got["timing"]["packed_records"]
        assert all(got["complete"])
        cur = dict(scores=got["scores"].tolist(), spans=[x.tolist() for x in got["spans"]], layers=got["batch"].dump_layers(0))
        got["batch"].close()
        lean = run_local(pairs, params, score_only=True)
        lean["batch"].close()
        assert lean["timing"]["waves_per_pair"] == team
        assert lean["scores"].tolist() == cur["scores"] and [x.tolist() for x in lean["spans"]][1::2] == cur["spans"][1::2]
        if base is None:
            base = cur
            for p, pair in enumerate(pairs):
                sa, ea, sb, eb = (x[p] for x in cur["spans"])
                assert cur["scores"][p] > 0 and sa < ea and sb < eb
                mu1, mu2 = le.tables_of(pair, params)
                assert le.window_global(params, mu1, mu2, sa, ea, sb, eb) == cur["scores"][p]
            b = make_batch(pairs, params)   # without the flag: other scores
            b.run()
            assert b.scores().tolist() != cur["scores"]
            b.close()
        else:
            assert cur["scores"] == base["scores"] and cur["spans"] == base["spans"]
            np.testing.assert_array_equal(cur["layers"], base["layers"])


# ---- the forms of mu1 and mu2 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["mu1", "mu2"])
def test_dense_forms(form, ref):
    _, _, d1, d2 = form_tables()
    want = ref[("form", form)]
    kw = dict(mu1_dense=[d1]) if form == "mu1" else dict(mu2_dense=[d2])
    for score_only in (False, True):
        got = run_local([FORM_PAIR], FORM_PARAMS, score_only=score_only, **kw)
        got["batch"].close()
        check_ends(got, [want])
        if not score_only:
            span = tuple(int(x[0]) for x in got["spans"])
            assert bool(got["complete"][0]) and le.span_score(want, *ref[("tables", ("form", form))], span) == want["score"]


def test_feature_form(ref):
    from bialign_amd.batch import make_feature_batch
    want = ref[("form", "feature")]
    for score_only in (False, True):
        b = make_feature_batch(feature_molecules(), [(0, 1)], dict(synth.RNA_PARAMS), local=True, score_only=score_only)
        b.run()
        spans = b.local_spans()
        assert int(b.scores()[0]) == want["score"] and (int(spans[1][0]), int(spans[3][0])) == want["end"]
        if not score_only:
            _, ok = b.traces()
            assert bool(ok[0])
            assert le.span_score(want, *ref[("tables", ("form", "feature"))], tuple(int(x[0]) for x in spans)) == want["score"]
        b.close()


# ---- null batches ---------------------------------------------------------------------------------------------------

def test_null_batch_scores_the_shuffles_in_local_mode(ref):
    want = [[ref[("null", p, r)]["score"] for r in range(NULL_R)] for p in range(len(NULL_PAIRS))]
    observed = [ref[("null", p, None)]["score"] for p in range(len(NULL_PAIRS))]
    nb = sg.null_batch(NULL_PAIRS, FORM_PARAMS, NULL_R, seed=NULL_SEED, local=True)
    nb.run()
    got = nb.null_scores()
    nb.close()
    assert got.tolist() == want
    z = sg.zscores(NULL_PAIRS, FORM_PARAMS, replicas=NULL_R, seed=NULL_SEED, local=True)
    exp = sg.zscores_from_stats(observed, stats_of(want, observed))
    for k in exp:
        np.testing.assert_array_equal(z[k], exp[k], err_msg=k)
    # without the flag the replicas are scored globally: other numbers
    nb = sg.null_batch(NULL_PAIRS, FORM_PARAMS, NULL_R, seed=NULL_SEED)
    nb.run()
    assert nb.null_scores().tolist() != want
    nb.close()


def test_null_feature_and_dense_batches(ref):
    mols = feature_molecules()
    nb = sg.null_feature_batch(mols, [(0, 1)], dict(synth.RNA_PARAMS), NULL_R, seed=NULL_SEED, local=True)
    nb.run()
    assert nb.null_scores()[0].tolist() == [ref[("null-feature", r)]["score"] for r in range(NULL_R)]
    nb.close()
    _, _, d1, d2 = form_tables()
    nb = sg.null_dense_batch([FORM_PAIR], FORM_PARAMS, NULL_R, seed=NULL_SEED, mu1_dense=[d1], mu2_dense=[d2], local=True)
    nb.run()
    assert nb.null_scores()[0].tolist() == [ref[("null-dense", r)]["score"] for r in range(NULL_R)]
    nb.close()


# ---- ABI error paths --------------------------------------------------------------------------------------------------

def test_spans_of_other_batches_are_refused():
    from bialign_amd._lib import BialignError, E_INVALID
    from bialign_amd.batch import make_batch
    for kw in (dict(), dict(fit=True)):   # without the flag, and a FIT batch: no local spans
        b = make_batch([FORM_PAIR], FORM_PARAMS, **kw)
        b.run()
        with pytest.raises(BialignError) as err:
            b.local_spans()
        assert err.value.code == E_INVALID
        b.close()
    b = make_batch([FORM_PAIR], FORM_PARAMS, local=True)   # a LOCAL batch: no fit spans, and no spans before a run
    with pytest.raises(BialignError) as err:
        b.local_spans()
    assert err.value.code == E_INVALID
    b.run()
    with pytest.raises(BialignError) as err:
        b.fit_spans()
    assert err.value.code == E_INVALID
    b.close()
    nb = sg.null_batch(NULL_PAIRS, FORM_PARAMS, NULL_R, seed=NULL_SEED, local=True)   # a null batch: no observed alignments
    nb.run()
    with pytest.raises(BialignError) as err:
        nb.local_spans()
    assert err.value.code == E_INVALID
    nb.close()


@pytest.mark.parametrize("kw,s,code", [(dict(fit=True), 1, "E_INVALID"), (dict(lean_trace=True), 1, "E_UNSUPPORTED"),
                                       (dict(level_trace=True), 1, "E_UNSUPPORTED"), (dict(), 6, "E_UNSUPPORTED"),
                                       (dict(beta=100), 1, "E_UNSUPPORTED"), (dict(hbm_budget_bytes=64 << 10), 1, "E_NOMEM")],
                         ids=["fit", "lean_trace", "level_trace", "max_shift 6", "beta > 0", "budget"])
def test_refusals(kw, s, code):
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch
    kw = dict(kw)
    params = dict(FORM_PARAMS, max_shift=s)
    if "beta" in kw:
        params["gap_opening_cost"] = kw.pop("beta")
    with pytest.raises(_lib.BialignError) as err:
        make_batch([FORM_PAIR], params, local=True, **kw)
    assert err.value.code == getattr(_lib, code) and "LOCAL" in err.value.message
