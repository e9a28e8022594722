"""The ghost feed's steady-block fast path (bialign_feed.hpp: a scalar base plus lane constants instead of 3 x 64 recomputed
source addresses; the unpack takes a steady block as packed without a per-lane test) computes what the general path
computes: full nine-layer dumps, scores and traces against the oracle on the smallest shapes each team size admits
(T * 72 + 64 <= P and two strips per wave) -- tests/test_feed_fastpath_host.py asserts that each of them has steady and
non-steady blocks beyond the first strips.  The fast path lives in fill_affine_slim_kernel (max_shift 1, teams of 2, 3,
6); fill_affine_kernel keeps the general path through the same factored source function, covered here with BIALIGN_SLIM=0
(its max_shift 2 and 3 forms have no fast path and get no case of their own: the existing packed-record tests run them)."""
import numpy as np
import pytest

from bialign_amd import synth

pytestmark = pytest.mark.gpu

PARAMS = dict(synth.PROTEIN_PARAMS)      # max_shift 1, affine


def solve_and_check(pair, params, team):
    from oracle import oracle
    from bialign_amd.batch import make_batch
    from bialign_amd.engine import trace_codes_to_columns
    n, m, s = len(pair[0]), len(pair[1]), params["max_shift"]
    ref = oracle.solve(*pair, params)
    b = make_batch([pair], params)
    b.run()
    t = b.timing()
    traces, ok = b.traces()
    layers = b.dump_layers(0)
    score = int(b.scores()[0])
    b.close()
    assert t["packed_records"] and t["recovered_runs"] == 0
    if team is not None:
        assert t["waves_per_pair"] == team
    assert score == ref["score"]
    assert trace_codes_to_columns(traces[0]) == oracle.trace_to_lists(ref["trace"])
    assert bool(ok[0]) == ref["complete"]
    for g, e in zip(oracle.band_values(layers, n, m, s), oracle.band_values(ref["layers"], n, m, s)):
        np.testing.assert_array_equal(g, e)


@pytest.mark.parametrize("team,n,m", [(2, 61, 256), (3, 110, 280), (6, 221, 500)])
def test_slim_sweep_forced_teams(team, n, m, monkeypatch):
    monkeypatch.setenv("BIALIGN_PACK", "1")
    monkeypatch.setenv("BIALIGN_TEAM", str(team))
    solve_and_check(synth.protein_pair(7100 + n, n, m), PARAMS, team)


@pytest.mark.parametrize("team,n,m", [(1, 61, 256), (2, 110, 280), (4, 221, 500)])
def test_two_wave_sweep_keeps_the_general_path(team, n, m, monkeypatch):
    monkeypatch.setenv("BIALIGN_PACK", "1")
    monkeypatch.setenv("BIALIGN_SLIM", "0")
    monkeypatch.setenv("BIALIGN_TEAM", str(team))
    solve_and_check(synth.protein_pair(7200 + n, n, m), PARAMS, team)


def test_last_strip_cut_short(monkeypatch):
    """n = 105 against 20 rows per strip: the sixth strip holds six rows, the sweep's last records end the pair's region."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    monkeypatch.setenv("BIALIGN_TEAM", "3")
    solve_and_check(synth.protein_pair(7305, 105, 280), PARAMS, 3)


def test_no_steady_block_at_all(monkeypatch):
    """m = 46: no phase of the period leaves room for a whole steady block (a period this short admits no team, so the
    pair runs on one wave of fill_affine_kernel)."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    solve_and_check(synth.protein_pair(7346, 61, 46), PARAMS, None)


def test_ragged_launch_of_six_pairs(monkeypatch):
    """Six pairs of different (n, m) in teams of three: a workgroup holds four pairs, steady() differs from wave to wave
    inside it.  Scores and traces of all six, every layer cell of three."""
    from oracle import oracle
    from bialign_amd.batch import make_batch
    from bialign_amd.engine import trace_codes_to_columns
    monkeypatch.setenv("BIALIGN_PACK", "1")
    monkeypatch.setenv("BIALIGN_TEAM", "3")
    shapes = [(110, 280), (127, 301), (141, 288), (118, 333), (163, 295), (150, 312)]
    pairs = [synth.protein_pair(7400 + t, n, m) for t, (n, m) in enumerate(shapes)]
    b = make_batch(pairs, PARAMS)
    b.run()
    t = b.timing()
    assert t["packed_records"] and t["recovered_runs"] == 0 and t["waves_per_pair"] == 3
    scores = b.scores()
    traces, ok = b.traces()
    refs = [oracle.solve(*pair, PARAMS) for pair in pairs]
    for k, ref in enumerate(refs):
        assert int(scores[k]) == ref["score"] and bool(ok[k]) == ref["complete"]
        assert trace_codes_to_columns(traces[k]) == oracle.trace_to_lists(ref["trace"])
    for k in (0, 3, 5):
        n, m = shapes[k]
        for g, e in zip(oracle.band_values(b.dump_layers(k), n, m, 1), oracle.band_values(refs[k]["layers"], n, m, 1)):
            np.testing.assert_array_equal(g, e)
    b.close()
