"""A run is a list of stages per chunk -- tables, fill, traceback, hits -- and every stage's time and launch count is
that of the last run, whatever the number of chunks."""
import pytest

from bialign_amd import synth

pytestmark = pytest.mark.gpu


def results(b):
    traces, complete = b.traces()
    hits, status = b.fit_hits()
    return dict(scores=b.scores().tolist(), traces=[t.tolist() for t in traces], complete=complete.tolist(),
                spans=[x.tolist() for x in b.fit_spans()], status=status,
                hits=[[(s, e, score, t.tolist()) for s, e, score, t in per_pair] for per_pair in hits])


def test_every_stage_of_a_chunked_feature_fit_batch_with_hits():
    """FEATURE form (tables are built per chunk), fit alignments with a hit search, and a budget of half the layers:
    all four stages run in each of at least two chunks, are counted and timed per run, and give what one chunk gives."""
    from bialign_amd.batch import make_feature_batch
    from bialign_amd.scoring import rna_features
    params = dict(synth.RNA_PARAMS, max_shift=1)
    mols, index = [], []
    for t in range(6):
        seq_a, seq_b, str_a, str_b = synth.rna_pair(7300 + t, 12 + (5 * t) % 9, 40 + (8 * t) % 21)
        mols += [(seq_a, rna_features(seq_a, structure=str_a)), (seq_b, rna_features(seq_b, structure=str_b))]
        index.append((2 * t, 2 * t + 1))

    one = make_feature_batch(mols, index, params, fit=True)
    one.set_hits(4, 1)
    one.run()
    assert one.info["nchunks"] == 1
    want = results(one)
    budget = one.info["hbm_layer_bytes"] // 2
    one.close()

    b = make_feature_batch(mols, index, params, fit=True, hbm_budget_bytes=budget)
    b.set_hits(4, 1)
    nchunks = b.info["nchunks"]
    assert nchunks >= 2
    b.run()
    timing, finfo = b.timing(), b.feature_info()
    assert timing["fill_launches"] == nchunks and finfo["build_launches"] == nchunks
    assert timing["fill_ms"] > 0 and timing["traceback_ms"] > 0 and finfo["build_ms"] > 0
    assert b.hit_info()["search_ms"] > 0
    assert results(b) == want
    b.run()
    assert b.feature_info()["build_launches"] == nchunks  # per run, not cumulative
    b.run(fill_only=True)
    assert b.timing()["traceback_ms"] >= 0 and b.scores().tolist() == want["scores"]
    b.close()
