"""Fit alignments (BIALIGN_BATCH_FIT) on the GPU against tests/fit_expected.py: one oracle fill per start of the
substring gives every substring's global score, hence the fit score, the smallest best end, and the FIT layers.

The oracle runs of every case of this module are made once, in one spawn pool (``ref``), and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_expected as fe
import free_ends_gpu as fg
from bialign_amd import significance as sg
from bialign_amd import synth
from free_ends_gpu import feature_mu2, pad, params_of, seq_mu1, stats_of

pytestmark = pytest.mark.gpu

SHIFTS, NS, MS = (0, 1, 2, 3, 5), (1, 22, 50), (50, 97)
SHAPES = [(n, m) for n in NS for m in MS]
# max_shift 1: n = 50 spans three strips of 21 rows, m = 97 a dozen 8-column ghost blocks and six range-check intervals.
# A team of three waves needs six strips and a column period of 280: the smallest such shape, for the forced team shapes.
TEAM_SHAPE = (101, 278)
NULL_R, NULL_SEED = 8, 5
pair_of = fg.pair_of(fe.make_pair, 7000)


def case_pairs(cost, s):
    """[(kind, n, m, planted)] of one (costs, max_shift): per shape a planted protein pair (whose layers are compared)
    and a plain RNA pair; at the narrow bands, where the oracle is cheap, a plain protein and a planted RNA pair too."""
    if cost == "beta>0":   # the one case of a rewarded gap opening: protein pairs of the three-strip shapes
        return [("protein", n, m, planted) for n, m in SHAPES if n == 50 for planted in (True, False)]
    out = []
    for n, m in SHAPES:
        out += [("protein", n, m, True), ("rna", n, m, False)]
        if s <= 2:
            out += [("protein", n, m, False), ("rna", n, m, True)]
    return out


def main_cases():
    return [(cost, s) for cost in ("affine", "one-layer") for s in SHIFTS] + [("beta>0", 1)]


FORM_PARAMS = dict(synth.PROTEIN_PARAMS)
FORM_PAIR = fe.make_pair("protein", 4242, 22, 50, True)
NULL_PAIRS = [fe.make_pair("protein", 4300, 22, 50, True), fe.make_pair("protein", 4301, 15, 41, False)]
feature_molecules = lambda: fg.feature_molecules(77, (20, 47))
form_tables = lambda: fg.form_tables(FORM_PAIR, FORM_PARAMS)


@pytest.fixture(scope="module")
def ref():
    """{key: fit_expected's dict} for every pair of this module."""
    cases = {}
    for cost, s in main_cases():
        for kind, n, m, planted in case_pairs(cost, s):
            prm = params_of(kind, cost, s)
            mu1, mu2 = fe.tables_of(pair_of(kind, n, m, planted), prm)
            cases[("main", cost, s, kind, n, m, planted)] = (n, m, prm, mu1, mu2, kind == "protein" and planted)
    for planted in (True, False):   # the forced team shapes: two long pairs, scores / spans / walks only
        prm = params_of("protein", "affine", 1)
        mu1, mu2 = fe.tables_of(pair_of("protein", *TEAM_SHAPE, planted), prm)
        cases[("team", planted)] = (*TEAM_SHAPE, prm, mu1, mu2, False)
        lprm = params_of("protein", "one-layer", 1)
        cases[("team-one-layer", planted)] = (*TEAM_SHAPE, lprm, *fe.tables_of(pair_of("protein", *TEAM_SHAPE, planted), lprm), False)
    mu1, mu2, d1, d2 = form_tables()
    cases[("form", "mu1")] = (22, 50, FORM_PARAMS, pad(d1), mu2, False)
    cases[("form", "mu2")] = (22, 50, FORM_PARAMS, mu1, pad(d2), False)
    mols = feature_molecules()
    fprm = dict(synth.RNA_PARAMS)
    cases[("form", "feature")] = (20, 47, fprm, seq_mu1(mols[0][0], mols[1][0], fprm),
                                  feature_mu2(mols[0][1], mols[1][1], fprm["structure_weight"]), False)
    for p, pair in enumerate(NULL_PAIRS):   # observed pairs and their replicas, as the host shuffles them
        cases[("null", p, None)] = (len(pair[0]), len(pair[1]), FORM_PARAMS, *fe.tables_of(pair, FORM_PARAMS), False)
        for r in range(NULL_R):
            cases[("null", p, r)] = (len(pair[0]), len(pair[1]), FORM_PARAMS,
                                     *fe.tables_of(sg.shuffle_b(pair, NULL_SEED, p, r), FORM_PARAMS), False)
    for r in range(4):
        seq_b, feats_b = sg.shuffle_features(mols[1][0], mols[1][1], NULL_SEED, 0, r)
        cases[("null-feature", r)] = (20, 47, fprm, seq_mu1(mols[0][0], seq_b, fprm),
                                      feature_mu2(mols[0][1], feats_b, fprm["structure_weight"]), False)
        cases[("null-dense", r)] = (22, 50, FORM_PARAMS, pad(sg.shuffle_tables(d1, NULL_SEED, 0, r)),
                                    pad(sg.shuffle_tables(d2, NULL_SEED, 0, r)), False)
    return fe.expected_many(cases)


def run_fit(pairs, params, **kw):
    """A FIT batch of ``pairs`` -> dict of its results (full storage: traces and spans of the walk too)."""
    from bialign_amd.batch import make_batch
    b = make_batch(pairs, params, fit=True, **kw)
    b.run()
    out = dict(scores=b.scores().copy(), spans=b.fit_spans(), timing=b.timing(), affine=b.affine, batch=b)
    if not kw.get("score_only"):
        out["traces"], out["complete"] = b.traces()
    return out


def check_walks(got, pairs, params, wants):
    """Every pair of a full-storage FIT batch: score, smallest best end, and the walk -- complete, its columns re-scored
    on B[start_b:end_b] give the score, and that substring's global score is the score."""
    from bialign_amd.batch import encode_flat
    from bialign_amd.verify import rescore_trace
    model, fb = encode_flat(pairs, params)
    mols_a, mols_b = fb.molecules("a"), fb.molecules("b")
    start, end = got["spans"]
    for p, want in enumerate(wants):
        n, m = len(pairs[p][0]), len(pairs[p][1])
        assert int(got["scores"][p]) == want["score"], p
        assert int(end[p]) == want["end_b"], p
        assert bool(got["complete"][p]), p
        s0, e0 = int(start[p]), int(end[p])
        assert 0 <= s0 <= e0 <= m, p
        assert want["glob"][s0, e0] == want["score"], (p, s0, e0)
        total, idx, drift = rescore_trace(got["traces"][p], mols_a[p][0], mols_a[p][1], mols_b[p][0][s0:e0], mols_b[p][1][s0:e0],
                                          model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"], params["shift_cost"],
                                          got["affine"])
        assert total == want["score"] and idx == (n, e0 - s0, n, e0 - s0) and drift <= params["max_shift"], p


# ---- the inputs: windows inside B occur --------------------------------------------------------------------------------

def test_inputs_have_inner_windows(ref):
    """A condition on the inputs, from the helper alone: in every shape some pair's best substring ends before B's end
    and cannot start at B's first residue.  (Not asked of beta > 0: where every gap opening is rewarded, the best
    substring is as long as B.)"""
    for cost, s in main_cases():
        for n, m in SHAPES if cost != "beta>0" else []:
            inner = []
            for kind, n2, m2, planted in case_pairs(cost, s):
                if (n2, m2) == (n, m):
                    want = ref[("main", cost, s, kind, n, m, planted)]
                    inner.append(want["end_b"] < m and want["glob"][0, want["end_b"]] < want["score"])
            assert any(inner), (cost, s, n, m)


# ---- scores, spans, walks and layers -----------------------------------------------------------------------------------

@pytest.mark.parametrize("cost,s", main_cases(), ids=lambda v: str(v))
def test_full_storage_against_the_oracle(cost, s, ref):
    for kind in ("protein", "rna"):
        todo = [c for c in case_pairs(cost, s) if c[0] == kind]
        if not todo:
            continue
        pairs = [pair_of(*c) for c in todo]
        params = params_of(kind, cost, s)
        wants = [ref[("main", cost, s, *c)] for c in todo]
        got = run_fit(pairs, params)
        check_walks(got, pairs, params, wants)
        for p, (c, want) in enumerate(zip(todo, wants)):   # one pair per shape: the FIT layers
            if want["layers"] is not None:
                fe.compare_layers(got["batch"].dump_layers(p).astype(np.int64), want["layers"], c[1], c[2], s)
        # a fill-only run leaves the fit scores and the ends, and no start
        got["batch"].run(fill_only=True)
        np.testing.assert_array_equal(got["batch"].scores(), got["scores"])
        start, end = got["batch"].fit_spans()
        assert (start == -1).all()
        np.testing.assert_array_equal(end, got["spans"][1])
        got["batch"].close()


@pytest.mark.parametrize("cost,s", main_cases(), ids=lambda v: str(v))
def test_score_only_against_the_oracle(cost, s, ref):
    """The lean sweeps keep the best end cell of row n themselves (fill_linear_kernel, fill_affine_kernel; the affine
    max_shift 1 sweep: see test_kernels_see_fit)."""
    for kind in ("protein", "rna"):
        todo = [c for c in case_pairs(cost, s) if c[0] == kind]
        if not todo:
            continue
        wants = [ref[("main", cost, s, *c)] for c in todo]
        got = run_fit([pair_of(*c) for c in todo], params_of(kind, cost, s), score_only=True)
        got["batch"].close()
        assert [int(x) for x in got["scores"]] == [w["score"] for w in wants]
        assert [int(x) for x in got["spans"][1]] == [w["end_b"] for w in wants]
        assert (got["spans"][0] == -1).all()


# ---- every kernel sees FIT ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pack", ["1", "0"])
@pytest.mark.parametrize("team", ["1", "3", "x3"])
def test_kernels_see_fit(team, pack, ref, monkeypatch):
    """max_shift 1, affine, under the forced team shapes, packed records on and forced off, full storage and score-only:
    the issue's shapes (whose short periods admit one wave per pair whatever is asked), and two pairs long enough for a
    team of three, where timing() says which sweep ran: the three-waves-per-SIMD kernel (teams of 3: packed or LEAN
    records), fill_affine_kernel with packed, full and LEAN records, one wave, two, and as a cross-CU team."""
    monkeypatch.setenv("BIALIGN_TEAM", team)
    monkeypatch.setenv("BIALIGN_PACK", pack)
    params = params_of("protein", "affine", 1)
    small = [c for c in case_pairs("affine", 1) if c[0] == "protein"]
    long_pairs = [pair_of("protein", *TEAM_SHAPE, planted) for planted in (True, False)]
    long_wants = [ref[("team", planted)] for planted in (True, False)]
    for score_only in (False, True):
        for pairs, wants, is_long in (([pair_of(*c) for c in small], [ref[("main", "affine", 1, *c)] for c in small], False),
                                      (long_pairs, long_wants, True)):
            got = run_fit(pairs, params, score_only=score_only)
            got["batch"].close()
            t = got["timing"]
            if is_long:
                slim = team == "3" and (score_only or pack == "1")
                assert t["waves_per_pair"] == (1 if team == "1" else (3 if slim or team == "x3" else 2)), t
                assert t["cross_cu"] == (team == "x3"), t
            assert t["packed_records"] == (pack == "1" and not score_only), t
            if score_only:
                assert [int(x) for x in got["scores"]] == [w["score"] for w in wants]
                assert [int(x) for x in got["spans"][1]] == [w["end_b"] for w in wants]
                assert (got["spans"][0] == -1).all()
            else:
                check_walks(got, pairs, params, wants)


def test_one_layer_teams_see_fit(ref, monkeypatch):
    """fill_linear_kernel alone and as a team (two waves, and a cross-CU team) on the long pairs' shape, score-only and
    full."""
    params = params_of("protein", "one-layer", 1)
    pairs = [pair_of("protein", *TEAM_SHAPE, planted) for planted in (True, False)]
    base = tuple(tuple(ref[("team-one-layer", planted)][k] for planted in (True, False)) for k in ("score", "end_b"))
    for team in ("1", "2", "x3"):
        monkeypatch.setenv("BIALIGN_TEAM", team)
        for score_only in (False, True):
            got = run_fit(pairs, params, score_only=score_only)
            got["batch"].close()
            assert got["timing"]["waves_per_pair"] == int(team.lstrip("x")) and got["timing"]["cross_cu"] == (team == "x3")
            key = (tuple(int(x) for x in got["scores"]), tuple(int(x) for x in got["spans"][1]))
            assert key == base
            if not score_only:
                assert (got["spans"][0] >= 0).all() and all(got["complete"])


# ---- the forms of mu1 and mu2 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["mu1", "mu2"])
def test_dense_forms(form, ref):
    _, _, d1, d2 = form_tables()
    want = ref[("form", form)]
    kw = dict(mu1_dense=[d1]) if form == "mu1" else dict(mu2_dense=[d2])
    for score_only in (False, True):
        got = run_fit([FORM_PAIR], FORM_PARAMS, score_only=score_only, **kw)
        got["batch"].close()
        assert int(got["scores"][0]) == want["score"] and int(got["spans"][1][0]) == want["end_b"]
        if not score_only:
            s0, e0 = int(got["spans"][0][0]), int(got["spans"][1][0])
            assert bool(got["complete"][0]) and want["glob"][s0, e0] == want["score"]


def test_feature_form(ref):
    from bialign_amd.batch import make_feature_batch
    want = ref[("form", "feature")]
    for score_only in (False, True):
        b = make_feature_batch(feature_molecules(), [(0, 1)], dict(synth.RNA_PARAMS), fit=True, score_only=score_only)
        b.run()
        start, end = b.fit_spans()
        assert int(b.scores()[0]) == want["score"] and int(end[0]) == want["end_b"]
        if not score_only:
            _, ok = b.traces()
            assert bool(ok[0]) and want["glob"][int(start[0]), int(end[0])] == want["score"]
        b.close()


# ---- null batches ---------------------------------------------------------------------------------------------------

def test_null_batch_scores_the_shuffles_in_fit_mode(ref):
    want = [[ref[("null", p, r)]["score"] for r in range(NULL_R)] for p in range(len(NULL_PAIRS))]
    observed = [ref[("null", p, None)]["score"] for p in range(len(NULL_PAIRS))]
    nb = sg.null_batch(NULL_PAIRS, FORM_PARAMS, NULL_R, seed=NULL_SEED, fit=True)
    nb.run()
    got = nb.null_scores()
    nb.close()
    assert got.tolist() == want
    z = sg.zscores(NULL_PAIRS, FORM_PARAMS, replicas=NULL_R, seed=NULL_SEED, fit=True)
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
    nb = sg.null_feature_batch(mols, [(0, 1)], dict(synth.RNA_PARAMS), 4, seed=NULL_SEED, fit=True)
    nb.run()
    assert nb.null_scores()[0].tolist() == [ref[("null-feature", r)]["score"] for r in range(4)]
    nb.close()
    _, _, d1, d2 = form_tables()
    nb = sg.null_dense_batch([FORM_PAIR], FORM_PARAMS, 4, seed=NULL_SEED, mu1_dense=[d1], mu2_dense=[d2], fit=True)
    nb.run()
    assert nb.null_scores()[0].tolist() == [ref[("null-dense", r)]["score"] for r in range(4)]
    nb.close()


# ---- without the flag; refusals ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", ["affine", "one-layer"])
def test_unchanged_without_the_flag(cost):
    from bialign_amd._lib import BialignError, E_INVALID
    from bialign_amd.batch import make_batch
    from bialign_amd.engine import trace_codes_to_columns
    from oracle import oracle
    params = params_of("protein", cost, 1)
    pairs = [pair_of("protein", n, 50, planted) for n in (1, 22, 50) for planted in (True, False)]
    b = make_batch(pairs, params)
    b.run()
    traces, ok = b.traces()
    for p, pair in enumerate(pairs):
        want = oracle.solve(*pair, params)
        assert int(b.scores()[p]) == want["score"] and bool(ok[p]) == want["complete"]
        assert trace_codes_to_columns(traces[p]) == oracle.trace_to_lists(want["trace"])
    with pytest.raises(BialignError) as err:
        b.fit_spans()
    assert err.value.code == E_INVALID
    b.close()


@pytest.mark.parametrize("kw,s", [(dict(lean_trace=True), 1), (dict(level_trace=True), 1), (dict(), 6)],
                         ids=["lean_trace", "level_trace", "max_shift 6"])
def test_refusals(kw, s):
    from bialign_amd._lib import BialignError, E_UNSUPPORTED
    from bialign_amd.batch import make_batch
    with pytest.raises(BialignError) as err:
        make_batch([FORM_PAIR], dict(FORM_PARAMS, max_shift=s), fit=True, **kw)
    assert err.value.code == E_UNSUPPORTED and "FIT" in err.value.message
