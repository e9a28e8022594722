"""The library reports the plan the host check computes: tests/plan_check.hip runs the planner's functions
(bialign_plan.hpp) on the CPU, the library runs them between its allocations, and for the same input -- every batch
with an explicit HBM budget far below the free memory, so that the budget alone decides -- chunks, storage mode,
layer bytes, cells, trace bytes, packed records and the forced team sizes are equal.  Every batch also runs once and
scores what the oracle scores."""
import numpy as np
import pytest

import plan_host as ph
import window_edge as we
from bialign_amd import synth

pytestmark = pytest.mark.gpu

SIX = [(41, 46), (64, 300), (40, 47), (66, 298), (43, 45), (62, 301)]     # P = 64 (no team fits) and P ~ 300 (teams of 2)
FEATURE_SHAPES = [(50, 61), (44, 58), (61, 50), (47, 66)]
SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE = 1, 2, 4
#: name -> (budget in bytes, expected chunks, expected storage mode)
TILED = {"one-chunk": (64 << 20, 1, 0), "three-chunks": (12 << 20, 3, 0), "lean": (3 << 20, 6, LEAN_TRACE)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ph.build(tmp_path_factory.mktemp("plan"))


@pytest.fixture(scope="module")
def six():
    from oracle import oracle
    pairs = [synth.protein_pair(7100 + t, n, m) for t, (n, m) in enumerate(SIX)]
    params = dict(synth.PROTEIN_PARAMS)
    return pairs, params, [oracle.solve(*p, dict(params), want_trace=False)["score"] for p in pairs]


def reported(b):
    """What the library tells of a batch's plan, after one run."""
    b.run()
    info, t = b.current_info(), b.timing()
    out = dict(nchunks=info["nchunks"], storage=info["storage"], hbm_layer_bytes=info["hbm_layer_bytes"], cells=info["cells"],
               trace_bytes=info["trace_bytes"], packed_records=int(t["packed_records"]), waves_per_pair=t["waves_per_pair"],
               scores=[int(v) for v in b.scores()], table_bytes=b.feature_info()["table_bytes"])
    b.close()
    return out


def planned(plan):
    last = plan.teams[-1] if plan.teams else None       # (the timing holds the last launch's team)
    return dict(nchunks=plan.nchunks, storage=plan.storage, hbm_layer_bytes=4 * plan.max_chunk_dwords, cells=plan.cells,
                trace_bytes=plan.trace_bytes, packed_records=plan.pack, waves_per_pair=last["tw"] * last["gw"] if last else None)


def agree(got, plan, waves=True):
    assert plan.rc == 0, plan.msg
    want = planned(plan)
    if not waves:
        want.pop("waves_per_pair")
    print({k: (got[k], v) for k, v in want.items()})
    assert {k: got[k] for k in want} == want


@pytest.mark.parametrize("team", ["1", "2", "3"])
@pytest.mark.parametrize("name", list(TILED))
def test_six_ragged_pairs_packed(exe, six, name, team, monkeypatch):
    from bialign_amd.batch import make_batch
    pairs, params, scores = six
    budget, nchunks, storage = TILED[name]
    env = {"BIALIGN_PACK": "1", "BIALIGN_TEAM": team}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan, = ph.plans(exe, [ph.request(pairs=SIX, budget=budget, **ph.scoring_words(params, pairs))], env)
    assert (plan.nchunks, plan.storage, plan.pack) == (nchunks, storage, int(storage == 0))
    assert storage == 0 or budget < 4 * max(z["full_dwords"] for z in plan.sizes)       # below one pair's full layers
    got = reported(make_batch(pairs, params, hbm_budget_bytes=budget))
    agree(got, plan)
    assert got["scores"] == scores


def test_wide_band_falls_back_to_level_trace(exe):
    from oracle import oracle
    from bialign_amd.batch import make_batch
    pair, params = synth.protein_pair(5023, 23, 31), dict(synth.PROTEIN_PARAMS, max_shift=6)
    words = ph.scoring_words(params, [pair])
    full, plan = ph.plans(exe, [ph.request(pairs=[(23, 31)], **words), ph.request(pairs=[(23, 31)], budget=6150000, **words)])
    assert full.storage == 0 and 4 * full.max_chunk_dwords > 6150000 and plan.storage == LEVEL_TRACE
    got = reported(make_batch([pair], params, hbm_budget_bytes=6150000))
    agree(got, plan, waves=False)        # (the wide path's parts are not team_shape's)
    assert got["scores"] == [oracle.solve(*pair, dict(params), want_trace=False)["score"]]


def test_feature_batch_with_table_scratch_in_two_chunks(exe):
    from oracle import oracle
    from bialign_amd.batch import make_feature_batch
    params = dict(synth.RNA_PARAMS, max_shift=2)
    draw = lambda seed, n: "".join(np.random.default_rng(seed).choice(list("ACGU"), size=n))  # noqa: E731
    mols, index = [], []
    for t, (n, m) in enumerate(FEATURE_SHAPES):
        mols += [(draw(7200 + t, n), we.fractional(7300 + t, n)), (draw(7250 + t, m), we.fractional(7350 + t, m))]
        index.append((2 * t, 2 * t + 1))
    got = reported(make_feature_batch(mols, index, params, hbm_budget_bytes=8 << 20))
    fmax = lambda side, f: repr(max(float(np.max(mols[2 * t + side][1][f])) for t in range(len(index))))  # noqa: E731
    s1 = ph.scoring_words(params, [(mols[a][0], mols[c][0], "." * len(mols[a][0]), "." * len(mols[c][0])) for a, c in index])
    plan, = ph.plans(exe, [ph.request(pairs=FEATURE_SHAPES, budget=8 << 20, form="feature", sw=params["structure_weight"],
                                      fa=",".join(fmax(0, f) for f in range(3)), fb=",".join(fmax(1, f) for f in range(3)), **s1)])
    agree(got, plan)
    assert plan.nchunks == 2 and plan.max_chunk_tab_dwords > 0 and got["table_bytes"] == 4 * plan.max_chunk_tab_dwords
    for p, (a, c) in enumerate(index):
        n, m = FEATURE_SHAPES[p]
        mu1, _ = oracle.mu_tables(mols[a][0], mols[c][0], "." * n, "." * m, params)
        mu2 = np.zeros((n + 1, m + 1), dtype=np.int32)
        mu2[1:, 1:] = we.host_table(mols[a][1], mols[c][1], params["structure_weight"])
        assert got["scores"][p] == oracle.solve_tables(n, m, params, mu1, mu2, want_trace=False)["score"]


def test_wide_score_only_rings_in_chunks(exe):
    """A wide-band SCORE_ONLY batch under a budget of its largest ring and 1 MiB: the library cuts it where the planner
    does, by the rings, and still reports layers only."""
    from oracle import oracle
    from bialign_amd.batch import make_batch
    shapes = [(30, 55), (41, 46), (52, 37), (63, 28), (3, 40)]
    pairs = [synth.protein_pair(7400 + t, n, m) for t, (n, m) in enumerate(shapes)]
    params = dict(synth.PROTEIN_PARAMS, max_shift=8)
    budget = 4 * ph.ring_dwords(63, 8) + (1 << 20)
    plan, = ph.plans(exe, [ph.request(pairs=shapes, budget=budget, flags=SCORE_ONLY, **ph.scoring_words(params, pairs))])
    assert plan.rc == 0 and plan.storage == SCORE_ONLY and plan.nchunks > 1 and plan.max_chunk_dwords <= 16 * len(shapes)
    assert plan.max_chunk_ring_dwords >= ph.ring_dwords(63, 8) and 4 * (plan.max_chunk_dwords + plan.max_chunk_ring_dwords) <= budget
    got = reported(make_batch(pairs, params, score_only=True, hbm_budget_bytes=budget))
    agree(got, plan, waves=False)        # (the wide path's parts are not team_shape's)
    assert got["scores"] == [oracle.solve(*p, dict(params), want_trace=False)["score"] for p in pairs]


def test_wide_full_storage_in_chunks_and_a_one_pair_launch(exe):
    """Full storage at max_shift 7, cut into chunks by layers and rings together.  dump_layers re-fills one pair in a launch
    of its own: a pair that is neither the first of its chunk nor in the first chunk finds its ring at its own offset of
    the ring area.  A second run reuses the buffer, rings included."""
    from oracle import oracle
    from bialign_amd.batch import make_batch
    from bialign_amd.engine import trace_codes_to_columns
    shapes = [(30, 28), (5, 41), (41, 5), (1, 1), (17, 18), (36, 36), (2, 30), (24, 9)]
    pairs = [synth.protein_pair(7500 + t, n, m) for t, (n, m) in enumerate(shapes)]
    params = dict(synth.PROTEIN_PARAMS, max_shift=7)
    budget = 18 << 20   # (the largest pair: 14.8 MB of layers and 2.4 MB of ring)
    plan, = ph.plans(exe, [ph.request(pairs=shapes, budget=budget, **ph.scoring_words(params, pairs))])
    assert plan.rc == 0 and plan.storage == 0 and plan.nchunks >= 3
    # the last pair (by offset) of a chunk behind the first that holds several pairs
    inner = [b - 1 for a, b in zip(plan.chunks[1:], plan.chunks[2:]) if b - a >= 2]
    assert inner and all(plan.rings[p]["ring_off"] > 0 and plan.pairs[p]["layer_off"] > 0 for p in inner)
    pick = inner[0]
    b = make_batch(pairs, params, hbm_budget_bytes=budget)
    b.run()
    info = b.current_info()
    assert (info["nchunks"], info["storage"], info["hbm_layer_bytes"]) == (plan.nchunks, 0, 4 * plan.max_chunk_dwords)
    scores, (traces, ok) = b.scores().copy(), b.traces()
    traces = [t.copy() for t in traces]
    refs = [oracle.solve(*p, params) for p in pairs]
    assert [int(v) for v in scores] == [r["score"] for r in refs]
    n, m = shapes[pick]
    assert trace_codes_to_columns(traces[pick]) == oracle.trace_to_lists(refs[pick]["trace"])
    layers = b.dump_layers(pick)
    for g, e in zip(oracle.band_values(layers, n, m, 7), oracle.band_values(refs[pick]["layers"], n, m, 7)):
        np.testing.assert_array_equal(g, e)
    b.run()
    np.testing.assert_array_equal(b.scores(), scores)
    again, ok2 = b.traces()
    assert all(np.array_equal(x, y) for x, y in zip(again, traces)) and np.array_equal(ok, ok2)
    b.close()
