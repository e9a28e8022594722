"""Every copy of the free-end modes' tie rule on the GPU against the oracle, on the inputs of tests/tied_ends.py (verified
from the oracle alone by test_tied_ends_host.py): pairs whose best end is tied in a row, a column, on both end lines, in
different strips, lanes, waves and step classes; exact tandem repeats for the hit search; a pair in which nothing aligns;
and scaled twins at the edge of the int32 safety window.  There is no tolerance anywhere: scores, ends, spans, logs and
statuses are integers compared for equality with the oracle's.

The copies: free_end_scan (full-storage FIT and OVERLAP), the LEAN branches of fill_affine_kernel, fill_affine_slim_kernel
and fill_linear_kernel, RowBest / end_key_of / end_key_finish_kernel (LOCAL), and the masked argmax of fit_hits_kernel.

The oracle runs of every case of this module are made once, in spawn pools (``ref``), and shared: about 240 core-seconds,
32 s of wall time in a pool of 16, most of it the three pairs of the team shape (tied_ends.BUDGET).
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hits_expected as he
import local_expected as le
import test_gpu_fit as tgf
import test_gpu_fit_hits as tgh
import test_gpu_local as tgl
import test_gpu_overlap as tgo
import tied_ends as te
from free_ends_expected import tables_of
from free_ends_gpu import params_of

pytestmark = pytest.mark.gpu

RUN = {"fit": tgf.run_fit, "overlap": tgo.run_overlap, "local": tgl.run_local}
FLAG = {"fit": dict(fit=True), "overlap": dict(overlap=True), "local": dict(local=True)}


@pytest.fixture(scope="module")
def ref():
    cases = te.main_case_table()
    cases.update(te.team_case_table())
    cases.update(te.twin_case_table(scales=("k",)))
    return te.expected(cases)


def run(mode, pairs, params, **kw):
    got = RUN[mode](pairs, params, **kw)
    got["batch"].close()
    return got


def ends_of(mode, got):
    if mode == "fit":
        return [int(x) for x in got["spans"][1]]
    return [(int(a), int(b)) for a, b in zip(got["spans"][1], got["spans"][3])]


def check_ends(mode, got, wants):
    """Score and end: the oracle's smallest best end."""
    assert [int(x) for x in got["scores"]] == [w["score"] for w in wants]
    assert ends_of(mode, got) == [te.end_of(mode, w) for w in wants]


def check_full(mode, got, pairs, params, wants):
    """A full-storage run: score and end; the walk is complete, its window attains the score -- so its start is one of the
    oracle's optimal starts -- and its trace re-scores to the score (the modes' own check_walks)."""
    check_ends(mode, got, wants)
    if mode == "fit":
        tgf.check_walks(got, pairs, params, wants)
    elif mode == "overlap":
        tgo.check_walks(got, pairs, params, wants)
    else:
        tgl.check_walks(got, pairs, params, wants, [(params, *tables_of(pair, params)) for pair in pairs])


def check_lean(mode, got, wants, full=None):
    """A score-only run: score and end as the oracle's; no starts; ``full``: and as the full-storage run's, byte for byte."""
    check_ends(mode, got, wants)
    starts = got["spans"][:1] if mode == "fit" else got["spans"][0::2]
    assert all((x == -1).all() for x in starts)
    if full is not None:
        assert got["scores"].tobytes() == full["scores"].tobytes()
        ends = (lambda g: g["spans"][1:2]) if mode == "fit" else (lambda g: g["spans"][1::2])
        assert [x.tobytes() for x in ends(got)] == [x.tobytes() for x in ends(full)]


def main_of(ref, mode, cost, s):
    inputs = te.inputs_of(mode, cost, s)
    return [i.pair for i in inputs], [ref[(mode, "main", i.name, cost, s)] for i in inputs]


def team_of(ref, mode, cost):
    inputs = [i for i in te.TEAM.values() if mode in i.modes]
    return [i.pair for i in inputs], [ref[(mode, "team", i.name, cost, 1)] for i in inputs]


# ---- the table's inputs and their tall variants, every band ------------------------------------------------------------------------

@pytest.mark.parametrize("mode,cost,s", te.main_cases(), ids=lambda v: str(v))
def test_full_storage(mode, cost, s, ref):
    """free_end_scan (FIT, OVERLAP) and the folded keys (LOCAL) behind a full-storage sweep, and the walk from the end."""
    pairs, wants = main_of(ref, mode, cost, s)
    params = params_of("protein", cost, s)
    check_full(mode, run(mode, pairs, params), pairs, params, wants)


@pytest.mark.parametrize("mode,cost,s", te.main_cases(), ids=lambda v: str(v))
def test_score_only(mode, cost, s, ref, monkeypatch):
    """The LEAN sweeps keep the best end themselves.  max_shift 1, affine, FIT and OVERLAP: the pairs of the team shape too,
    in teams of three and, with the slim sweep off (BIALIGN_SLIM=0, as tests/test_gpu_window_edge.py's test_score_only), in
    teams of two, so that both LEAN copies of the rule run."""
    pairs, wants = main_of(ref, mode, cost, s)
    params = params_of("protein", cost, s)
    check_lean(mode, run(mode, pairs, params, score_only=True), wants, full=run(mode, pairs, params))
    if (cost, s) == ("affine", 1) and mode != "local":
        pairs, wants = team_of(ref, mode, cost)
        for team, slim, waves in (("3", None, 3), ("2", "0", 2)):   # fill_affine_slim_kernel; fill_affine_kernel as a team of two
            monkeypatch.setenv("BIALIGN_TEAM", team)
            if slim is not None:
                monkeypatch.setenv("BIALIGN_SLIM", slim)
            got = run(mode, pairs, params, score_only=True)
            assert got["timing"]["waves_per_pair"] == waves and not got["timing"]["cross_cu"], got["timing"]
            check_lean(mode, got, wants)


# ---- (b) the team shape: every sweep and record form ---------------------------------------------------------------------------------

@pytest.mark.parametrize("pack", ["1", "0"])
@pytest.mark.parametrize("team", ["1", "3", "x3"])
def test_kernel_variants(team, pack, ref, monkeypatch):
    """max_shift 1, affine, 101 x 278: tied ends of row n in a boundary step ahead of the interior run, in an interior step
    and on column m; tied ends of column m in strips of three different waves.  The forced team shapes, packed records on
    and forced off, full storage and score-only; timing() says which sweep ran (tests/test_gpu_fit.py, test_kernels_see_fit).
    One set of results: the oracle's."""
    monkeypatch.setenv("BIALIGN_TEAM", team)
    monkeypatch.setenv("BIALIGN_PACK", pack)
    params = params_of("protein", "affine", 1)
    for mode in ("fit", "overlap"):
        pairs, wants = team_of(ref, mode, "affine")
        for score_only in (False, True):
            got = run(mode, pairs, params, score_only=score_only)
            t = got["timing"]
            slim = team == "3" and (score_only or pack == "1")
            assert t["waves_per_pair"] == (1 if team == "1" else (3 if slim or team == "x3" else 2)), t
            assert t["cross_cu"] == (team == "x3"), t
            assert t["packed_records"] == (pack == "1" and not score_only), t
            if score_only:
                check_lean(mode, got, wants)
            else:
                check_full(mode, got, pairs, params, wants)


def test_one_layer_teams(ref, monkeypatch):
    """fill_linear_kernel alone and as a team (two waves, and a cross-CU team) on the same pairs, score-only and full."""
    params = params_of("protein", "one-layer", 1)
    for team in ("1", "2", "x3"):
        monkeypatch.setenv("BIALIGN_TEAM", team)
        for mode in ("fit", "overlap"):
            pairs, wants = team_of(ref, mode, "one-layer")
            for score_only in (False, True):
                got = run(mode, pairs, params, score_only=score_only)
                assert got["timing"]["waves_per_pair"] == int(team.lstrip("x")) and got["timing"]["cross_cu"] == (team == "x3")
                if score_only:
                    check_lean(mode, got, wants)
                else:
                    check_full(mode, got, pairs, params, wants)


# ---- (c) LOCAL teams ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", ["affine", "one-layer"])
def test_local_teams(cost, monkeypatch):
    """101 x 278 at max_shift 2, one wave and a team of four: two tied columns in one row, and a tied row in the strip of
    another wave.  An exact expectation is out of reach at this shape (test_tied_ends_host.py holds the pair's parts and its
    cut-down twin against the oracle): the score is a unit's oracle score against itself, the end the smallest planted one,
    the walk's window scores that by one oracle run, and the teams agree."""
    params = params_of("protein", cost, te.LOCAL_TEAM_SHIFT)
    pair = te.LOCAL_TEAM.pair
    score = te.self_score(te.U, params)
    base = None
    for team in te.LOCAL_TEAM_SIZES:
        monkeypatch.setenv("BIALIGN_TEAM", str(team))
        full = run("local", [pair], params)
        lean = run("local", [pair], params, score_only=True)
        assert full["timing"]["waves_per_pair"] == team and lean["timing"]["waves_per_pair"] == team
        for got in (full, lean):
            assert [int(x) for x in got["scores"]] == [score] and ends_of("local", got) == [te.LOCAL_TEAM_ENDS[0]]
        assert (lean["spans"][0] == -1).all() and (lean["spans"][2] == -1).all() and bool(full["complete"][0])
        cur = (full["scores"].tobytes(), [x.tobytes() for x in full["spans"]], full["traces"][0].tobytes())
        if base is None:
            base = cur
            sa, ea, sb, eb = (int(x[0]) for x in full["spans"])
            assert le.window_global(params, *tables_of(pair, params), sa, ea, sb, eb) == score
        assert cur == base


# ---- the hit search on exact repeats: fit-far and (d) the mask input ------------------------------------------------------------------

@pytest.mark.parametrize("cost", ["affine", "one-layer"])
def test_hits_on_exact_repeats(cost, ref, monkeypatch):
    """min_score 1: nearly every end is a candidate, so a wrong mask bit or a tie broken towards the larger column changes
    the log.  As many hits as copies, in rising order of end; packed records on and forced off; a second run repeats."""
    from bialign_amd.batch import make_batch
    params = params_of("protein", cost, 1)
    for inp, key, spans in ((te.BASE["fit-far"], ("fit", "main", "fit-far", cost, 1), te.FAR_SPANS),
                            (te.MASK, ("fit", "mask", te.MASK.name, cost, 1), te.MASK_SPANS)):
        spec = te.hit_spec(inp)
        base = None
        for pack in ("1", "0"):
            monkeypatch.setenv("BIALIGN_PACK", pack)
            b = make_batch([inp.pair], params, fit=True, hits=(spec[0], spec[2], spec[1]))
            got = tgh.search(b)
            again = tgh.search(b)
            b.close()
            t = got["timing"]
            if pack == "0" or cost != "affine":
                assert not t["packed_records"], t
            tgh.check_against_oracle(got, spec, [ref[key]], [inp.pair], params, cost == "affine")
            assert [h[:2] for h in got["hits"][0]] == spans and got["status"] == ["exhausted"], (inp, got["hits"], got["status"])
            tgh.same_results(again, got)
            if base is None:
                base = got
            tgh.same_results(got, base)


# ---- nothing aligns ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", te.MODES)
def test_nothing_aligns(mode, ref):
    """The pair of spacers in one batch with an aligning pair on either side of it, so that a stale or shared key shows.
    LOCAL: 0 at the origin, every cell tied -- a zeroed key lies below the origin's.  OVERLAP: 0 at (0, m), tied with
    (n, 0).  FIT: a constant profile, all of A in gaps, and a search that finds nothing."""
    from bialign_amd.batch import make_batch
    nothing = te.BASE["nothing"]
    other = te.BASE["cross" if mode == "overlap" else "row"]
    inputs = [other, nothing, other]
    for cost in ("affine", "one-layer"):
        params = params_of("protein", cost, 1)
        pairs = [i.pair for i in inputs]
        wants = [ref[(mode, "main", i.name, cost, 1)] for i in inputs]
        full = run(mode, pairs, params)
        check_full(mode, full, pairs, params, wants)
        check_lean(mode, run(mode, pairs, params, score_only=True), wants, full=full)
        spans = [int(x[1]) for x in full["spans"]]
        if mode == "local":
            assert int(full["scores"][1]) == 0 and spans == [0, 0, 0, 0] and len(full["traces"][1]) == 0
        elif mode == "overlap":
            assert int(full["scores"][1]) == 0 and spans[1::2] == [0, nothing.m] and len(full["traces"][1]) == 0
            assert spans[0] == spans[1] and spans[2] == spans[3]
        else:
            assert int(full["scores"][1]) == (-1000 if cost == "affine" else -700) and spans == [0, 0]
            assert len(full["traces"][1]) == nothing.n
            spec = he.resolve((3, 1))
            b = make_batch(pairs, params, fit=True, hits=(3, 1))
            got = tgh.search(b)
            b.close()
            tgh.check_against_oracle(got, spec, wants, pairs, params, cost == "affine")
            assert got["hits"][1] == [] and got["walks"][1] == [] and got["status"][1] == "exhausted"
            assert got["profiles"][1].tolist() == [int(full["scores"][1])] * (nothing.m + 1)
            assert len(got["hits"][0]) == 3 and got["hits"][0][0][1] == wants[0]["end_b"]


# ---- (e) dense forms ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", te.MODES)
def test_dense_forms(mode, ref):
    """The pairs' own tables as dense mu1 and mu2: the D1 kernels, the same expectations."""
    for cost in ("affine", "one-layer"):
        params = params_of("protein", cost, 1)
        for inp in (i for i in te.DENSE if mode in i.modes):
            want = ref[(mode, "main", inp.name, cost, 1)]
            kw = te.dense_kw(inp, params)
            full = run(mode, [inp.pair], params, **kw)
            check_full(mode, full, [inp.pair], params, [want])
            check_lean(mode, run(mode, [inp.pair], params, score_only=True, **kw), [want], full=full)


# ---- (f) the window's edge ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", te.MODES)
def test_window_edge(mode, ref):
    """Every score times the largest k the safety window admits: the floors, LOCAL's clamp at 0 beside "-infinity" cells,
    the biased score of end_key_of and the walks' stop rule at 2^22 .. 2^24.  One step further the batch is refused."""
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch
    refused = 0
    for t in (t for t in te.TWINS.values() if mode in t.modes):
        params, want = t.at(t.k), ref[(mode, "twin", t.name, "k")]
        full = run(mode, [t.pair], params)
        check_full(mode, full, [t.pair], params, [want])
        check_lean(mode, run(mode, [t.pair], params, score_only=True), [want], full=full)
        if mode == "fit" and t.inp.name == "fit-far":
            spec = te.hit_spec(t)
            b = make_batch([t.pair], params, fit=True, hits=(spec[0], spec[2], spec[1]))
            got = tgh.search(b)
            b.close()
            tgh.check_against_oracle(got, spec, [want], [t.pair], params, t.costs == "affine")
            assert [h[:2] for h in got["hits"][0]] == te.FAR_SPANS and got["status"] == ["exhausted"]
        if not refused:
            with pytest.raises(_lib.BialignError) as err:
                make_batch([t.pair], t.at(t.k + 1), **FLAG[mode]).close()
            assert err.value.code == _lib.E_RANGE and "safety window" in err.value.message
            refused += 1
    assert refused
