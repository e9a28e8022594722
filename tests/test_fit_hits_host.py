"""The hit search of FIT batches (include/bialign.h, "Hit search") without a GPU:
  * tests/hits_expected.py itself: ``replay`` accepts a consistent log and rejects a wrong end, a wrong tie, a wrong
    acceptance and a wrong status;
  * the front ends refuse what the search does not take before any device call (``make_batch(hits=)``, ``batch_cli``);
  * the condition the inputs with several placements must meet, from the oracle alone (``hits_expected.PLANTED``, which
    tests/test_gpu_fit_hits.py runs on the GPU)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_expected as fe
import hits_expected as he
from hits_expected import PLANTED, PLANTED_COSTS, planted_case, planted_spec

# ---- replay on a hand-made table -----------------------------------------------------------------------------------

def hand_glob():
    """m = 6.  E = (-100, -100, -100, 50, 30, 40, 40): the best placement is [1, 3); [4, 5) and [4, 6) tie at 40; [2, 4)
    (30) runs into [1, 3)."""
    glob = np.full((7, 7), fe.NONE, dtype=np.int64)
    glob[np.triu_indices(7)] = -100
    glob[1, 3], glob[4, 5], glob[4, 6], glob[2, 4] = 50, 40, 40, 30
    return glob


LOG = [(3, 1, 50, True), (5, 4, 40, True), (6, 4, 40, False), (4, 2, 30, False)]
HITS = [(1, 3, 50), (4, 5, 40)]
SPEC = (5, 10, 25)


def test_replay_accepts_a_consistent_log():
    he.replay(hand_glob(), SPEC, LOG, HITS, "exhausted")
    he.replay(hand_glob(), (2, 10, 25), LOG[:2], HITS, "max_hits")
    he.replay(hand_glob(), (5, 3, 25), LOG[:3], HITS, "max_walks")
    he.replay(hand_glob(), (2, 2, 25), LOG[:2], HITS, "max_hits")   # both bounds met by one walk: MAX_HITS comes first
    he.replay(hand_glob(), (5, 10, 51), [], [], "exhausted")
    for rule in (min, max):
        assert he.greedy(hand_glob(), SPEC, rule) == (HITS, LOG, "exhausted")
    assert he.resolve((3, 7)) == (3, 12, 7) and he.resolve((3, 7, 5)) == (3, 5, 7)


@pytest.mark.parametrize("what,log,hits,status", [
    ("wrong end", [(5, 4, 40, True)] + LOG[1:], HITS, "exhausted"),
    ("wrong tie", [LOG[0], (6, 4, 40, True)], [HITS[0], (4, 6, 40)], "exhausted"),
    ("wrong acceptance", LOG[:2] + [(6, 4, 40, True)] + LOG[3:], HITS + [(4, 6, 40)], "exhausted"),
    ("wrong status", LOG, HITS, "max_walks"),
    ("no optimal start", [(3, 0, 50, True)], [(0, 3, 50)], "exhausted"),
    ("candidates left", LOG[:3], HITS, "exhausted"),
    ("after the search had to stop", LOG, HITS, "max_hits"),
], ids=lambda v: v if isinstance(v, str) and " " in v else "")
def test_replay_rejects(what, log, hits, status):
    spec = (2, 10, 25) if what == "after the search had to stop" else SPEC
    with pytest.raises(AssertionError, match=what):
        he.replay(hand_glob(), spec, log, hits, status)


# ---- the front ends refuse before any device call -------------------------------------------------------------------

PAIR = ("ACDEFGHIK", "AACDEFGHIKAACDEFGHIKAA", "HHHHEEEEC", "CCHHHHEEEECCHHHHEEEECC")


@pytest.mark.parametrize("kw,match", [
    (dict(hits=(3, 100)), "fit=True"),
    (dict(hits=(3, 100), fit=True, score_only=True), "score_only"),
    (dict(hits=(0, 100), fit=True), "max_hits"),
    (dict(hits=(257, 100), fit=True), "max_hits"),
    (dict(hits=(3, 0), fit=True), "min_score"),
    (dict(hits=(4, 100, 3), fit=True), "max_walks"),
    (dict(hits=(3,), fit=True), "hits must be"),
], ids=lambda v: "" if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_make_batch_refuses_hits(kw, match, monkeypatch):
    from bialign_amd import batch, engine, synth
    called = []
    monkeypatch.setattr(engine, "default_engine", lambda device=0: called.append(device))
    with pytest.raises(ValueError, match=match):
        batch.make_batch([PAIR], dict(synth.PROTEIN_PARAMS), **kw)
    assert not called


OPTS = ["--type", "Protein", "--simmatrix", "BLOSUM62", "--gap_opening_cost", "-150", "--gap_cost", "-50",
        "--shift_cost", "-150", "--structure_weight", "800", "--max_shift", "1", "--outmode", "sorted"]


@pytest.mark.parametrize("extra,match", [
    (["--hits", "3", "--hit_min_score", "100"], "--hits needs --fit"),
    (["--fit", "--hits", "3", "--hit_min_score", "100", "--score_only"], "excludes --score_only and --zscore"),
    (["--fit", "--hits", "3", "--hit_min_score", "100", "--zscore", "8"], "excludes --score_only and --zscore"),
    (["--fit", "--hits", "3"], "go together"),
    (["--fit", "--hit_min_score", "100"], "go together"),
    (["--fit", "--hits", "300", "--hit_min_score", "100"], "max_hits"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else "")
def test_batch_cli_refuses_hits(extra, match, tmp_path, capsys, monkeypatch):
    from bialign_amd import batch, batch_cli
    called = []
    monkeypatch.setattr(batch, "make_batch", lambda *a, **kw: called.append(kw))
    f = tmp_path / "pairs.tsv"
    f.write_text("\t".join(("a", PAIR[0], PAIR[2], "b", PAIR[1], PAIR[3])) + "\n")
    with pytest.raises(SystemExit) as err:
        batch_cli.main([str(f)] + OPTS + extra)
    assert err.value.code == 2 and match in capsys.readouterr().err and not called


def test_batch_cli_hit_lines():
    from bialign_amd import batch_cli
    args = batch_cli.build_parser().parse_args(["x.tsv", "--fit", "--hits", "4", "--hit_min_score", "900"])
    assert batch_cli.check_hit_options(batch_cli.build_parser(), args) == (4, 900, 0)
    assert batch_cli.check_hit_options(batch_cli.build_parser(), batch_cli.build_parser().parse_args(["x.tsv", "--fit"])) is None
    assert batch_cli.hit_line(1, 30, 52, 1234) == "hit 1\tB span\t 31..52\t1234"


# ---- inputs with several placements: the condition, from the oracle alone -------------------------------------------

def test_planted_inputs_hold_their_copies():
    wants = fe.expected_many({cost: planted_case(cost)[3] for cost in PLANTED_COSTS})
    n = PLANTED["n"]
    for cost in PLANTED_COSTS:
        _, windows, _, _ = planted_case(cost)
        glob = wants[cost]["glob"]
        spec = planted_spec(glob, windows)
        assert spec[2] >= 1
        for rule in (min, max):
            hits, walks, status = he.greedy(glob, spec, rule)
            assert status == "exhausted" and len(hits) == PLANTED["copies"], (cost, rule, hits, status)
            for w in windows:   # every planted window is met by a hit
                assert sum(he.meets((w, w + n), h[:2]) for h in hits) >= 1, (cost, rule, w, hits)
            he.replay(glob, spec, walks, hits, status)
