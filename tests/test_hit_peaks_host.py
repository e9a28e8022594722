"""Peak candidates and per-pair thresholds of the hit search (include/bialign.h, "Hit search") without a GPU:
  * tests/hits_peaks_expected.py itself: ``peaks`` on hand-made profiles; ``replay`` accepts a consistent log and rejects
    a walk from a non-peak end, a walk below the pair's threshold and a wrong status;
  * the condition on the planted input (``hits_expected.PLANTED``), from the oracle alone: what the peak rule exists for;
  * the front ends refuse bad ``peaks``, ``min_permille`` and ``min_scores`` before any device call;
  * ``significance.hit_zscores`` against ``zscores_from_stats`` on hand-made stats."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_expected as fe
import hits_expected as he
import hits_peaks_expected as hp
from hits_expected import PLANTED, PLANTED_COSTS, planted_case
from test_fit_hits_host import HITS, LOG, OPTS, PAIR, SPEC, hand_glob

# ---- peaks on hand-made profiles --------------------------------------------------------------------------------------

@pytest.mark.parametrize("what,E,want", [
    ("a strict maximum", [1, 5, 2], [1]),
    ("a plateau: its left end, behind a strict rise", [0, 3, 3, 3, 1], [1]),
    ("a plateau that begins the profile", [3, 3, 1], [0]),
    ("j = 0", [4, 2, 3], [0, 2]),
    ("j = m", [1, 2, 3], [2]),
    ("j = m behind a plateau is no peak", [1, 3, 3], [1]),
    ("a constant profile", [7, 7, 7, 7], [0]),
    ("one end", [5], [0]),
    ("two maxima, a valley between", [1, 9, 4, 4, 9, 2], [1, 4]),
], ids=lambda v: v if isinstance(v, str) else "")
def test_peaks(what, E, want):
    assert np.flatnonzero(hp.peaks(E)).tolist() == want


def test_the_smallest_global_argmax_is_a_peak():
    rng = np.random.default_rng(5)
    for m in (0, 1, 2, 5, 40):
        for hi in (1, 2, 4):   # few values: plateaus and ties everywhere
            for _ in range(50):
                E = rng.integers(0, hi + 1, m + 1)
                assert hp.peaks(E)[int(np.argmax(E))], E
    assert hp.peaks(he.profile(hand_glob()))[3]


# ---- replay under the peak rule and a threshold -----------------------------------------------------------------------
# hand_glob's E = (-100, -100, -100, 50, 30, 40, 40): the peaks are the ends 0, 3 and 5.

PEAK_LOG = [LOG[0], LOG[1]]   # the ends 3 and 5; the ends 4 and 6 are no peaks


def test_replay_accepts_a_consistent_log():
    assert np.flatnonzero(hp.peaks(he.profile(hand_glob()))).tolist() == [0, 3, 5]
    hp.replay(hand_glob(), SPEC, LOG, HITS, "exhausted")   # the old rule, unchanged
    hp.replay(hand_glob(), SPEC, PEAK_LOG, HITS, "exhausted", peaks=True)
    hp.replay(hand_glob(), (2, 10, 25), PEAK_LOG, HITS, "max_hits", peaks=True)
    hp.replay(hand_glob(), (1, 10, 1), LOG[:1], HITS[:1], "max_hits", peaks=True, threshold=45)
    hp.replay(hand_glob(), SPEC, LOG[:1], HITS[:1], "exhausted", threshold=45)      # the threshold stands for min_score
    hp.replay(hand_glob(), SPEC, LOG[:3], HITS, "exhausted", threshold=40)
    hp.replay(hand_glob(), SPEC, [], [], "exhausted", peaks=True, threshold=51)
    for rule in (min, max):
        assert hp.greedy(hand_glob(), SPEC, rule) == he.greedy(hand_glob(), SPEC, rule) == (HITS, LOG, "exhausted")
        assert hp.greedy(hand_glob(), SPEC, rule, peaks=True) == (HITS, PEAK_LOG, "exhausted")
        assert hp.greedy(hand_glob(), SPEC, rule, threshold=45) == (HITS[:1], LOG[:1], "exhausted")
    assert hp.threshold([5, 2001, 7], 1, 500) == 1001 and hp.threshold([5, 2001, 7], 1500, 500) == 1500
    assert hp.threshold([-3, -1], 1, 1000) == 1 and hp.threshold([5, 2000], 1, 0) == 1


@pytest.mark.parametrize("what,log,hits,status,kw", [
    ("is no peak", LOG[:3], HITS, "exhausted", dict(peaks=True)),
    ("below the threshold", LOG, HITS, "exhausted", dict(threshold=35)),
    ("below the threshold", PEAK_LOG, HITS, "exhausted", dict(peaks=True, threshold=45)),
    ("wrong status", PEAK_LOG, HITS, "max_walks", dict(peaks=True)),
    ("wrong status", LOG[:1], HITS[:1], "max_hits", dict(threshold=45)),
    ("candidates left", LOG[:1], HITS[:1], "exhausted", dict(peaks=True)),
    ("wrong end", [LOG[1]], [HITS[1]], "exhausted", dict(peaks=True)),
], ids=lambda v: v if isinstance(v, str) and " " in v else "")
def test_replay_rejects(what, log, hits, status, kw):
    with pytest.raises(AssertionError, match=what):
        hp.replay(hand_glob(), SPEC, log, hits, status, **kw)


# ---- the planted input: the condition, from the oracle alone -----------------------------------------------------------

def test_planted_input_under_the_peak_rule():
    """A 22 against B 150 with three planted copies.  With today's defaults (max_hits 3, max_walks 12) the search without
    the flag spends its walks on the ends behind hit 0 and reports one copy; from the peaks it reports all three."""
    wants = fe.expected_many({cost: planted_case(cost)[3] for cost in PLANTED_COSTS})
    n = PLANTED["n"]
    for cost in PLANTED_COSTS:
        _, windows, _, _ = planted_case(cost)
        glob = wants[cost]["glob"]
        E = he.profile(glob)
        spec = he.resolve((3, int(min(glob[w, w + n] for w in windows))))
        assert spec[1] == 12
        for rule in (min, max):
            hits, walks, status = hp.greedy(glob, spec, rule)
            assert (len(hits), status) == (1, "max_walks") and len(walks) == 12, (cost, rule, hits, status)
            hits, walks, status = hp.greedy(glob, spec, rule, peaks=True)
            assert len(hits) == 3 and len(walks) <= 12, (cost, rule, hits, walks, status)
            for w in windows:   # one hit per planted window
                assert sum(he.meets((w, w + n), h[:2]) for h in hits) == 1, (cost, rule, w, hits)
            hp.replay(glob, spec, walks, hits, status, peaks=True)
            # min_score 1 and half the pair's fit score: three hits, exhausted; the picks are a prefix of the run at the
            # lower threshold spec[2] // 2 (T >= that, since Emax >= spec[2])
            T = hp.threshold(E, 1, 500)
            assert T >= spec[2] // 2
            wide = he.resolve((4, 1))
            hits, walks, status = hp.greedy(glob, wide, rule, peaks=True, threshold=T)
            assert (len(hits), status) == (3, "exhausted") and len(walks) <= 16, (cost, rule, hits, walks, status)
            hp.replay(glob, wide, walks, hits, status, peaks=True, threshold=T)
            low = hp.greedy(glob, wide, rule, peaks=True, threshold=spec[2] // 2)
            assert low[1][:len(walks)] == walks and low[0][:len(hits)] == hits, (cost, rule, walks, low)


# ---- the front ends refuse before any device call ---------------------------------------------------------------------

BAD_RULES = [
    (dict(peaks=1), "peaks must be a bool"),
    (dict(peaks="yes"), "peaks must be a bool"),
    (dict(peaks=None), "peaks must be a bool"),
    (dict(min_permille=-1), "min_permille"),
    (dict(min_permille=1001), "min_permille"),
    (dict(min_permille=0.5), "min_permille"),
    (dict(min_permille="500"), "min_permille"),
    (dict(min_permille=True), "min_permille"),
    (dict(min_permille=None), "min_permille"),
    (dict(min_scores=[0]), "min_scores"),
    (dict(min_scores=[-5]), "min_scores"),
    (dict(min_scores=[1, 2]), "min_scores"),
    (dict(min_scores=[]), "min_scores"),
    (dict(min_scores=[1.5]), "min_scores"),
    (dict(min_scores=["7"]), "min_scores"),
    (dict(min_scores=[2 ** 31]), "min_scores"),
    (dict(min_scores=7), "min_scores"),
    (dict(min_scores=[[1]]), "min_scores"),
    (dict(min_scores=[True]), "min_scores"),
]


@pytest.mark.parametrize("kw,match", BAD_RULES, ids=lambda v: "" if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_make_batch_refuses_bad_rules(kw, match, monkeypatch):
    from bialign_amd import batch, engine, synth
    called = []
    monkeypatch.setattr(engine, "default_engine", lambda device=0: called.append(device))
    with pytest.raises(ValueError, match=match):
        batch.make_batch([PAIR], dict(synth.PROTEIN_PARAMS), fit=True, hits=dict(max_hits=3, min_score=100, **kw))
    with pytest.raises(ValueError, match=match):
        batch.check_hit_rules(**kw, npairs=1)
    assert not called


@pytest.mark.parametrize("hits,match", [
    (dict(min_score=100), "max_hits, min_score"),
    (dict(max_hits=3), "max_hits, min_score"),
    (dict(max_hits=3, min_score=100, peak=True), "not peak"),
    (dict(max_hits=0, min_score=100, peaks=True), "max_hits must be"),
    (dict(max_hits=3, min_score=100, max_walks=2), "max_walks"),
], ids=lambda v: "" if isinstance(v, str) else "-".join(v))
def test_make_batch_refuses_bad_dicts(hits, match, monkeypatch):
    from bialign_amd import batch, engine, synth
    called = []
    monkeypatch.setattr(engine, "default_engine", lambda device=0: called.append(device))
    with pytest.raises(ValueError, match=match):
        batch.make_batch([PAIR], dict(synth.PROTEIN_PARAMS), fit=True, hits=hits)
    with pytest.raises(ValueError, match="fit=True"):
        batch.make_batch([PAIR], dict(synth.PROTEIN_PARAMS), hits=dict(max_hits=3, min_score=100, peaks=True))
    assert not called


def test_checked_arguments():
    from bialign_amd import batch
    assert batch.check_hit_rules() == (False, None, 0)
    peaks, scores, permille = batch.check_hit_rules(np.True_, (5, 2 ** 31 - 1), np.int64(1000), npairs=2)
    assert peaks is True and permille == 1000 and scores.dtype == np.int32 and scores.tolist() == [5, 2 ** 31 - 1]
    got = batch.check_hits_arg(dict(max_hits=3, min_score=100, peaks=True, min_scores=[7]), True, False, npairs=1)
    assert got["min_scores"].tolist() == [7] and got["min_scores"].dtype == np.int32
    assert {k: v for k, v in got.items() if k != "min_scores"} == dict(max_hits=3, min_score=100, max_walks=0, peaks=True,
                                                                      min_permille=0)
    assert batch.check_hits_arg((3, 100), True, False) == (3, 100, 0)   # today's tuple, as it was


@pytest.mark.parametrize("extra,match", [
    (["--fit", "--hit_peaks"], "--hit_peaks and --hit_min_permille need --hits"),
    (["--fit", "--hit_min_permille", "500"], "--hit_peaks and --hit_min_permille need --hits"),
    (["--fit", "--hit_min_permille", "0"], "--hit_peaks and --hit_min_permille need --hits"),
    (["--hit_peaks", "--hit_min_score", "100"], "--hit_peaks and --hit_min_permille need --hits"),
    (["--fit", "--hits", "3", "--hit_min_score", "100", "--hit_min_permille", "1001"], "min_permille must be an int in 0..1000"),
    (["--fit", "--hits", "3", "--hit_min_score", "100", "--hit_min_permille", "-1"], "min_permille must be an int in 0..1000"),
    (["--hits", "3", "--hit_min_score", "100", "--hit_peaks"], "--hits needs --fit"),
    (["--fit", "--hits", "3", "--hit_min_score", "100", "--hit_peaks", "--zscore", "8"], "excludes --score_only and --zscore"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else "")
def test_batch_cli_refuses(extra, match, tmp_path, capsys, monkeypatch):
    from bialign_amd import batch, batch_cli
    called = []
    monkeypatch.setattr(batch, "make_batch", lambda *a, **kw: called.append(kw))
    f = tmp_path / "pairs.tsv"
    f.write_text("\t".join(("a", PAIR[0], PAIR[2], "b", PAIR[1], PAIR[3])) + "\n")
    with pytest.raises(SystemExit) as err:
        batch_cli.main([str(f)] + OPTS + extra)
    assert err.value.code == 2 and match in capsys.readouterr().err and not called


def test_batch_cli_hit_options():
    from bialign_amd import batch_cli
    parse = lambda *extra: batch_cli.check_hit_options(
        batch_cli.build_parser(), batch_cli.build_parser().parse_args(["x.tsv", "--fit", "--hits", "4", "--hit_min_score", "900", *extra]))
    assert parse() == (4, 900, 0)
    assert parse("--hit_peaks") == dict(max_hits=4, min_score=900, max_walks=0, peaks=True, min_permille=0)
    assert parse("--hit_min_permille", "250") == dict(max_hits=4, min_score=900, max_walks=0, peaks=False, min_permille=250)
    assert parse("--hit_peaks", "--hit_min_permille", "1000")["min_permille"] == 1000


# ---- significance.hit_zscores -----------------------------------------------------------------------------------------

def test_hit_zscores_against_zscores_from_stats():
    from bialign_amd import significance as sg
    # pair 0: four replicas 10, 20, 30, 40; pair 1: std = 0; pair 2: R = 1; pair 3: no hits
    stats = dict(replicas=np.array([4, 3, 1, 4], dtype=np.int32), sum=np.array([100, 60, 20, 100], dtype=np.int64),
                 sumsq=np.array([3000, 1200, 400, 3000], dtype=np.int64), n_ge=np.zeros(4, dtype=np.int32))
    hits = [[(0, 5, 90, None), (7, 12, 60, None), (20, 25, 25, None)], [(0, 4, 50, None)], [(1, 3, 40, None), (5, 7, 30, None)], []]
    z = sg.hit_zscores(hits, stats)
    assert [len(x) for x in z] == [3, 1, 2, 0] and all(x.dtype == np.float64 for x in z)
    for rank in range(3):   # rank by rank, the scores of that rank as the observed scores
        observed = [h[rank][2] if rank < len(h) else 0 for h in hits]
        want = sg.zscores_from_stats(observed, stats)["z"]
        for p, h in enumerate(hits):
            if rank < len(h):
                assert z[p][rank] == want[p] or (np.isnan(z[p][rank]) and np.isnan(want[p])), (p, rank)
    assert z[0][0] == (90 - 25.0) / (500 / 3) ** 0.5   # sample sd of 10, 20, 30, 40
    assert np.isnan(z[1]).all() and np.isnan(z[2]).all()
    with pytest.raises(ValueError, match="one entry per pair"):
        sg.hit_zscores(hits[:3], stats)
    with pytest.raises(ValueError, match="inconsistent"):
        sg.hit_zscores([[(0, 1, 5, None)]], dict(replicas=[2], sum=[10], sumsq=[10], n_ge=[0]))
