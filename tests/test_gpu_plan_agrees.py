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
LEAN_TRACE, LEVEL_TRACE = 2, 4
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
