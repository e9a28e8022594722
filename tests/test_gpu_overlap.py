"""Overlap alignments (BIALIGN_BATCH_OVERLAP) on the GPU against tests/overlap_expected.py: one oracle fill per free start
-- (i0, 0) and (0, j0), n + m + 1 of them -- gives every admissible window's global score, hence the overlap score, the
smallest best end cell, and the OVERLAP layers.

The oracle runs of every case of this module are made once, in one spawn pool (``ref``), and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import free_ends_gpu as fg
import overlap_expected as oe
from bialign_amd import significance as sg
from bialign_amd import synth
from free_ends_gpu import feature_mu2, pad, params_of, seq_mu1, stats_of

pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 2, 3, 5)
# max_shift 1: n = 50 spans three strips of 21 rows, m = 97 a dozen 8-column ghost blocks and six range-check intervals; the
# transposed shapes matter because both molecules' ends are free.  The planted kind a shape carries (None: too short), and
# the second one the narrow bands add.
SHAPES = {(1, 50): None, (22, 50): "a_in_b", (50, 97): "a_suffix_b_prefix", (97, 50): "b_suffix_a_prefix", (50, 22): "b_in_a",
          (50, 1): None}
SECOND = {(50, 97): "b_suffix_a_prefix", (97, 50): "a_suffix_b_prefix"}
# A team of three waves needs six strips and a column period of 280: the smallest such shape, for the forced team shapes.
TEAM_SHAPE = (101, 278)
TEAM_KINDS = ("a_suffix_b_prefix", "b_suffix_a_prefix")
NULL_R, NULL_SEED = 8, 5
pair_of = lambda kind, n, m, planted: oe.make_pair(kind, 9000 + 31 * n + m + 97 * (oe.KINDS.index(planted) + 1 if planted else 0), n, m, planted)


def case_pairs(cost, s):
    """[(kind, n, m, planted)] of one (costs, max_shift): per shape the protein pair of its planted kind (a plain one where
    the shape is too short), whose layers are compared, and -- but for beta > 0 -- a plain RNA pair; at max_shift <= 1 the
    long shapes' second planted kind too."""
    out = []
    for (n, m), planted in SHAPES.items():
        out.append(("protein", n, m, planted))
        if cost != "beta>0":
            out.append(("rna", n, m, None))
            if s <= 1 and (n, m) in SECOND:
                out.append(("protein", n, m, SECOND[(n, m)]))
    return out


def main_cases():
    return [(cost, s) for cost in ("affine", "one-layer") for s in SHIFTS] + [("beta>0", 1)]


FORM_PARAMS = dict(synth.PROTEIN_PARAMS)
FORM_PAIR = oe.make_pair("protein", 4242, 22, 50, "a_in_b")
NULL_PAIRS = [oe.make_pair("protein", 4300, 22, 50, "a_suffix_b_prefix"), oe.make_pair("protein", 4301, 15, 41, None)]
feature_molecules = lambda: fg.feature_molecules(77, (20, 47))
form_tables = lambda: fg.form_tables(FORM_PAIR, FORM_PARAMS)


@pytest.fixture(scope="module")
def ref():
    """{key: overlap_combine's dict} for every pair of this module."""
    cases = {}
    for cost, s in main_cases():
        for kind, n, m, planted in case_pairs(cost, s):
            prm = params_of(kind, cost, s)
            mu1, mu2 = oe.tables_of(pair_of(kind, n, m, planted), prm)
            cases[("main", cost, s, kind, n, m, planted)] = (n, m, prm, mu1, mu2, kind == "protein" and planted == SHAPES[(n, m)])
    for planted in TEAM_KINDS:   # the forced team shapes: two long pairs, scores / spans / walks only
        for name, cost in (("team", "affine"), ("team-one-layer", "one-layer")):
            prm = params_of("protein", cost, 1)
            cases[(name, planted)] = (*TEAM_SHAPE, prm, *oe.tables_of(pair_of("protein", *TEAM_SHAPE, planted), prm), False)
    mu1, mu2, d1, d2 = form_tables()
    cases[("form", "mu1")] = (22, 50, FORM_PARAMS, pad(d1), mu2, False)
    cases[("form", "mu2")] = (22, 50, FORM_PARAMS, mu1, pad(d2), False)
    mols = feature_molecules()
    fprm = dict(synth.RNA_PARAMS)
    cases[("form", "feature")] = (20, 47, fprm, seq_mu1(mols[0][0], mols[1][0], fprm),
                                  feature_mu2(mols[0][1], mols[1][1], fprm["structure_weight"]), False)
    for p, pair in enumerate(NULL_PAIRS):   # observed pairs and their replicas, as the host shuffles them
        cases[("null", p, None)] = (len(pair[0]), len(pair[1]), FORM_PARAMS, *oe.tables_of(pair, FORM_PARAMS), False)
        for r in range(NULL_R):
            cases[("null", p, r)] = (len(pair[0]), len(pair[1]), FORM_PARAMS,
                                     *oe.tables_of(sg.shuffle_b(pair, NULL_SEED, p, r), FORM_PARAMS), False)
    for r in range(4):
        seq_b, feats_b = sg.shuffle_features(mols[1][0], mols[1][1], NULL_SEED, 0, r)
        cases[("null-feature", r)] = (20, 47, fprm, seq_mu1(mols[0][0], seq_b, fprm),
                                      feature_mu2(mols[0][1], feats_b, fprm["structure_weight"]), False)
        cases[("null-dense", r)] = (22, 50, FORM_PARAMS, pad(sg.shuffle_tables(d1, NULL_SEED, 0, r)),
                                    pad(sg.shuffle_tables(d2, NULL_SEED, 0, r)), False)
    return oe.expected_many(cases)


def run_overlap(pairs, params, **kw):
    """An OVERLAP batch of ``pairs`` -> dict of its results (full storage: traces and spans of the walk too)."""
    from bialign_amd.batch import make_batch
    b = make_batch(pairs, params, overlap=True, **kw)
    b.run()
    out = dict(scores=b.scores().copy(), spans=b.overlap_spans(), timing=b.timing(), affine=b.affine, batch=b)
    if not kw.get("score_only"):
        out["traces"], out["complete"] = b.traces()
    return out


def check_ends(got, wants):
    assert [int(x) for x in got["scores"]] == [w["score"] for w in wants]
    assert [(int(a), int(b)) for a, b in zip(got["spans"][1], got["spans"][3])] == [w["end"] for w in wants]


def check_score_only(got, wants):
    check_ends(got, wants)
    assert (got["spans"][0] == -1).all() and (got["spans"][2] == -1).all()


def check_walks(got, pairs, params, wants):
    """Every pair of a full-storage OVERLAP batch: score, smallest best end cell, and the walk -- complete, its span an
    admissible window that attains the score, its columns re-scored on the two windows give the score."""
    from bialign_amd.batch import encode_flat
    from bialign_amd.verify import rescore_trace
    model, fb = encode_flat(pairs, params)
    mols_a, mols_b = fb.molecules("a"), fb.molecules("b")
    check_ends(got, wants)
    for p, want in enumerate(wants):
        n, m = len(pairs[p][0]), len(pairs[p][1])
        assert bool(got["complete"][p]), p
        sa, ea, sb, eb = span = tuple(int(x[p]) for x in got["spans"])
        assert oe.window_score(want, n, m, span) == want["score"], (p, span)
        assert (sa, sb) in want["starts"], (p, span)
        total, idx, drift = rescore_trace(got["traces"][p], mols_a[p][0][sa:ea], mols_a[p][1][sa:ea], mols_b[p][0][sb:eb], mols_b[p][1][sb:eb],
                                          model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"], params["shift_cost"],
                                          got["affine"])
        assert total == want["score"] and idx == (ea - sa, eb - sb, ea - sa, eb - sb) and drift <= params["max_shift"], p


# ---- the inputs: every geometry occurs ----------------------------------------------------------------------------------

def test_inputs_have_every_geometry(ref):
    """A condition on the inputs, from the helper alone: for each recurrence every planted kind yields a pair whose expected
    spans have that kind's geometry, some pair's best end lies on column m before A's end, and some pair's on row n before
    B's end.  Otherwise the mode could not be told from FIT in either direction, or from global."""
    for cost in ("affine", "one-layer"):
        seen, col_m, row_n = set(), False, False
        for s in SHIFTS:
            for kind, n, m, planted in case_pairs(cost, s):
                want = ref[("main", cost, s, kind, n, m, planted)]
                assert want["score"] >= 0
                if planted and oe.geometry(planted, want, n, m):
                    seen.add(planted)
                col_m |= want["end"][1] == m and want["end"][0] < n
                row_n |= want["end"][0] == n and want["end"][1] < m
        assert seen == set(oe.KINDS) and col_m and row_n, (cost, seen, col_m, row_n)


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
        got = run_overlap(pairs, params)
        check_walks(got, pairs, params, wants)
        for p, (c, want) in enumerate(zip(todo, wants)):   # one pair per shape: the OVERLAP layers
            if want["layers"] is not None:
                oe.compare_layers(got["batch"].dump_layers(p).astype(np.int64), want["layers"], c[1], c[2], s)
        # a fill-only run leaves the scores and the ends, and no start
        got["batch"].run(fill_only=True)
        np.testing.assert_array_equal(got["batch"].scores(), got["scores"])
        start_a, end_a, start_b, end_b = got["batch"].overlap_spans()
        assert (start_a == -1).all() and (start_b == -1).all()
        np.testing.assert_array_equal(end_a, got["spans"][1])
        np.testing.assert_array_equal(end_b, got["spans"][3])
        got["batch"].close()


@pytest.mark.parametrize("cost,s", main_cases(), ids=lambda v: str(v))
def test_score_only_against_the_oracle(cost, s, ref):
    """The LEAN sweeps fold the end cells into the pair's key themselves; end_key_finish_kernel decodes it."""
    for kind in ("protein", "rna"):
        todo = [c for c in case_pairs(cost, s) if c[0] == kind]
        if not todo:
            continue
        got = run_overlap([pair_of(*c) for c in todo], params_of(kind, cost, s), score_only=True)
        got["batch"].close()
        check_score_only(got, [ref[("main", cost, s, *c)] for c in todo])


# ---- every kernel sees the mode -------------------------------------------------------------------------------------

@pytest.mark.parametrize("pack", ["1", "0"])
@pytest.mark.parametrize("team", ["1", "3", "x3"])
def test_kernels_see_overlap(team, pack, ref, monkeypatch):
    """max_shift 1, affine, under the forced team shapes, packed records on and forced off, full storage and score-only:
    the small shapes (whose short periods admit one wave per pair whatever is asked), and two pairs long enough for a team
    of three, where timing() says which sweep ran: the three-waves-per-SIMD kernel (teams of 3: packed or LEAN records),
    fill_affine_kernel with packed, full and LEAN records, one wave, two, and as a cross-CU team."""
    monkeypatch.setenv("BIALIGN_TEAM", team)
    monkeypatch.setenv("BIALIGN_PACK", pack)
    params = params_of("protein", "affine", 1)
    small = [c for c in case_pairs("affine", 1) if c[0] == "protein"]
    long_pairs = [pair_of("protein", *TEAM_SHAPE, planted) for planted in TEAM_KINDS]
    long_wants = [ref[("team", planted)] for planted in TEAM_KINDS]
    # packed records need a column long enough for an interior step (Pack<1>::LO = 44 <= m - 1) in every pair of the batch
    wide, narrow = [c for c in small if c[2] >= 45], [c for c in small if c[2] < 45]
    assert wide and narrow
    for score_only in (False, True):
        for pairs, wants, is_long, packs in (([pair_of(*c) for c in wide], [ref[("main", "affine", 1, *c)] for c in wide], False, True),
                                             ([pair_of(*c) for c in narrow], [ref[("main", "affine", 1, *c)] for c in narrow], False, False),
                                             (long_pairs, long_wants, True, True)):
            got = run_overlap(pairs, params, score_only=score_only)
            got["batch"].close()
            t = got["timing"]
            if is_long:
                slim = team == "3" and (score_only or pack == "1")
                assert t["waves_per_pair"] == (1 if team == "1" else (3 if slim or team == "x3" else 2)), t
                assert t["cross_cu"] == (team == "x3"), t
            assert t["packed_records"] == (packs and pack == "1" and not score_only), t
            if score_only:
                check_score_only(got, wants)
            else:
                check_walks(got, pairs, params, wants)


def test_one_layer_teams_see_overlap(ref, monkeypatch):
    """fill_linear_kernel alone and as a team (two waves, and a cross-CU team) on the long pairs' shape, score-only and
    full."""
    params = params_of("protein", "one-layer", 1)
    pairs = [pair_of("protein", *TEAM_SHAPE, planted) for planted in TEAM_KINDS]
    wants = [ref[("team-one-layer", planted)] for planted in TEAM_KINDS]
    for team in ("1", "2", "x3"):
        monkeypatch.setenv("BIALIGN_TEAM", team)
        for score_only in (False, True):
            got = run_overlap(pairs, params, score_only=score_only)
            got["batch"].close()
            assert got["timing"]["waves_per_pair"] == int(team.lstrip("x")) and got["timing"]["cross_cu"] == (team == "x3")
            if score_only:
                check_score_only(got, wants)
            else:
                check_walks(got, pairs, params, wants)


def test_long_pairs_end_on_either_line(ref):
    """The long pairs' expectations, from the helper alone: one ends on row n, one on column m, each after a free start."""
    ends = {ref[("team", planted)]["end"] for planted in TEAM_KINDS}
    n, m = TEAM_SHAPE
    assert any(i == n and j < m for i, j in ends) and any(j == m and i < n for i, j in ends), ends
    for planted in TEAM_KINDS:
        assert oe.geometry(planted, ref[("team", planted)], n, m)


# ---- the forms of mu1 and mu2 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["mu1", "mu2"])
def test_dense_forms(form, ref):
    _, _, d1, d2 = form_tables()
    want = ref[("form", form)]
    kw = dict(mu1_dense=[d1]) if form == "mu1" else dict(mu2_dense=[d2])
    for score_only in (False, True):
        got = run_overlap([FORM_PAIR], FORM_PARAMS, score_only=score_only, **kw)
        got["batch"].close()
        check_ends(got, [want])
        if not score_only:
            span = tuple(int(x[0]) for x in got["spans"])
            assert bool(got["complete"][0]) and oe.window_score(want, 22, 50, span) == want["score"]


def test_feature_form(ref):
    from bialign_amd.batch import make_feature_batch
    want = ref[("form", "feature")]
    for score_only in (False, True):
        b = make_feature_batch(feature_molecules(), [(0, 1)], dict(synth.RNA_PARAMS), overlap=True, score_only=score_only)
        b.run()
        spans = b.overlap_spans()
        assert int(b.scores()[0]) == want["score"] and (int(spans[1][0]), int(spans[3][0])) == want["end"]
        if not score_only:
            _, ok = b.traces()
            assert bool(ok[0]) and oe.window_score(want, 20, 47, tuple(int(x[0]) for x in spans)) == want["score"]
        b.close()


# ---- null batches ---------------------------------------------------------------------------------------------------

def test_null_batch_scores_the_shuffles_in_overlap_mode(ref):
    want = [[ref[("null", p, r)]["score"] for r in range(NULL_R)] for p in range(len(NULL_PAIRS))]
    observed = [ref[("null", p, None)]["score"] for p in range(len(NULL_PAIRS))]
    nb = sg.null_batch(NULL_PAIRS, FORM_PARAMS, NULL_R, seed=NULL_SEED, overlap=True)
    nb.run()
    got = nb.null_scores()
    nb.close()
    assert got.tolist() == want
    z = sg.zscores(NULL_PAIRS, FORM_PARAMS, replicas=NULL_R, seed=NULL_SEED, overlap=True)
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
    nb = sg.null_feature_batch(mols, [(0, 1)], dict(synth.RNA_PARAMS), 4, seed=NULL_SEED, overlap=True)
    nb.run()
    assert nb.null_scores()[0].tolist() == [ref[("null-feature", r)]["score"] for r in range(4)]
    nb.close()
    _, _, d1, d2 = form_tables()
    nb = sg.null_dense_batch([FORM_PAIR], FORM_PARAMS, 4, seed=NULL_SEED, mu1_dense=[d1], mu2_dense=[d2], overlap=True)
    nb.run()
    assert nb.null_scores()[0].tolist() == [ref[("null-dense", r)]["score"] for r in range(4)]
    nb.close()


# ---- the order of the modes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", ["affine", "one-layer"])
def test_order_of_the_modes(cost, ref):
    """On the same pairs: global <= fit (A in B) <= overlap <= local, and fit (B in A) <= overlap -- every mode's windows
    are among the next one's."""
    from bialign_amd.batch import make_batch
    params = params_of("protein", cost, 1)
    todo = [c for c in case_pairs(cost, 1) if c[0] == "protein"]
    pairs = [pair_of(*c) for c in todo]
    swapped = [(sb, sa, tb, ta) for sa, sb, ta, tb in pairs]

    def scores(pp, **kw):
        b = make_batch(pp, params, score_only=True, **kw)
        b.run()
        out = b.scores().copy()
        b.close()
        return out
    glob, fit_ab, fit_ba, ovl, loc = scores(pairs), scores(pairs, fit=True), scores(swapped, fit=True), scores(pairs, overlap=True), \
        scores(pairs, local=True)
    assert ovl.tolist() == [ref[("main", cost, 1, *c)]["score"] for c in todo]
    assert (glob <= fit_ab).all() and (fit_ab <= ovl).all() and (ovl <= loc).all() and (fit_ba <= ovl).all()
    assert (glob < ovl).any() and (fit_ab < ovl).any() and (fit_ba < ovl).any()   # (the planted pairs tell the modes apart)


# ---- without the flag; refusals ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", ["affine", "one-layer"])
def test_unchanged_without_the_flag(cost):
    """Scores, traces and dumped layers of a global batch are the oracle's, bit for bit."""
    from bialign_amd._lib import BialignError, E_INVALID
    from bialign_amd.batch import make_batch
    from bialign_amd.engine import trace_codes_to_columns
    from oracle import oracle
    params = params_of("protein", cost, 1)
    pairs = [pair_of("protein", n, m, planted) for (n, m), planted in SHAPES.items()]
    b = make_batch(pairs, params)
    b.run()
    traces, ok = b.traces()
    for p, pair in enumerate(pairs):
        want = oracle.solve(*pair, params)
        n, m = len(pair[0]), len(pair[1])
        assert int(b.scores()[p]) == want["score"] and bool(ok[p]) == want["complete"]
        assert trace_codes_to_columns(traces[p]) == oracle.trace_to_lists(want["trace"])
        oe.compare_layers(b.dump_layers(p).astype(np.int64), want["layers"].astype(np.int64), n, m, 1)
    with pytest.raises(BialignError) as err:
        b.overlap_spans()
    assert err.value.code == E_INVALID
    b.close()


def test_spans_of_other_batches_are_refused():
    from bialign_amd._lib import BialignError, E_INVALID
    from bialign_amd.batch import make_batch
    for kw in (dict(fit=True), dict(local=True)):   # a FIT or LOCAL batch: no overlap spans
        b = make_batch([FORM_PAIR], FORM_PARAMS, **kw)
        b.run()
        with pytest.raises(BialignError) as err:
            b.overlap_spans()
        assert err.value.code == E_INVALID
        b.close()
    b = make_batch([FORM_PAIR], FORM_PARAMS, overlap=True)   # an OVERLAP batch: no fit or local spans
    b.run()
    for other in (b.fit_spans, b.local_spans):
        with pytest.raises(BialignError) as err:
            other()
        assert err.value.code == E_INVALID
    b.close()
    nb = sg.null_batch(NULL_PAIRS, FORM_PARAMS, 2, seed=NULL_SEED, overlap=True)   # a null batch: no observed alignments
    nb.run()
    with pytest.raises(BialignError) as err:
        nb.overlap_spans()
    assert err.value.code == E_INVALID
    nb.close()


@pytest.mark.parametrize("kw,s,code", [(dict(fit=True), 1, "E_INVALID"), (dict(local=True), 1, "E_INVALID"),
                                       (dict(lean_trace=True), 1, "E_UNSUPPORTED"), (dict(level_trace=True), 1, "E_UNSUPPORTED"),
                                       (dict(), 6, "E_UNSUPPORTED"), (dict(hbm_budget_bytes=64 << 10), 1, "E_NOMEM")],
                         ids=["fit", "local", "lean_trace", "level_trace", "max_shift 6", "budget"])
def test_refusals(kw, s, code):
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch
    with pytest.raises(_lib.BialignError) as err:
        make_batch([FORM_PAIR], dict(FORM_PARAMS, max_shift=s), overlap=True, **kw)
    assert err.value.code == getattr(_lib, code) and "OVERLAP" in err.value.message, err.value.message


# ---- the command line ---------------------------------------------------------------------------------------------------

def test_batch_cli_overlap(tmp_path, capsys, ref):
    """``batch_cli --overlap`` on two pairs: the span lines, and the rest of the block is what the single-pair CLI prints for
    the two windows."""
    from bialign_amd import batch_cli, cli
    cases = [("protein", 22, 50, "a_in_b"), ("protein", 50, 97, "a_suffix_b_prefix")]
    rows = []
    for t, c in enumerate(cases):
        sa, sb, ta, tb = pair_of(*c)
        rows.append(("a%d" % t, sa, ta, "b%d" % t, sb, tb))
    f = tmp_path / "pairs.tsv"
    f.write_text("".join("\t".join(r) + "\n" for r in rows))
    opts = ["--type", "Protein", "--simmatrix", "BLOSUM62", "--gap_opening_cost", "-150", "--gap_cost", "-50",
            "--shift_cost", "-150", "--structure_weight", "800", "--max_shift", "1", "--outmode", "sorted"]
    assert params_of("protein", "affine", 1)["structure_weight"] == 800
    batch_cli.main([str(f)] + opts + ["--overlap"])
    blocks = capsys.readouterr().out.split(">pair ")[1:]
    assert len(blocks) == 2
    for t, (c, (na, sa, ta, nb, sb, tb)) in enumerate(zip(cases, rows)):
        want = ref[("main", "affine", 1, *c)]
        lines = blocks[t].rstrip("\n").split("\n")
        at = lines.index(f"SCORE: {want['score']}")
        a_span, b_span = (re_span(lines[at + 1], "A"), re_span(lines[at + 2], "B"))
        assert (a_span[1], b_span[1]) == want["end"] and (a_span[0], b_span[0]) in want["starts"]
        cli.main([sa[a_span[0]:a_span[1]], sb[b_span[0]:b_span[1]], "--strA", ta[a_span[0]:a_span[1]], "--strB", tb[b_span[0]:b_span[1]],
                  "--nameA", na, "--nameB", nb] + opts)
        single = capsys.readouterr().out.rstrip("\n").split("\n")
        assert lines[at] == single[single.index(lines[at])] and lines[at + 3:] == single[single.index(lines[at]) + 1:]
    batch_cli.main([str(f)] + opts + ["--overlap", "--score_only"])
    lines = capsys.readouterr().out.strip().split("\n")
    for t, c in enumerate(cases):
        want = ref[("main", "affine", 1, *c)]
        assert lines[t].split("\t") == [f"pair {t}", rows[t][0], rows[t][3], str(want["score"]), str(want["end"][0]), str(want["end"][1])]


def re_span(line, which):
    """``A span\\t 3..9`` -> (2, 9): the 0-based half-open window."""
    import re
    got = re.fullmatch(rf"{which} span\t (\d+)\.\.(\d+)", line)
    assert got, line
    return int(got.group(1)) - 1, int(got.group(2))
