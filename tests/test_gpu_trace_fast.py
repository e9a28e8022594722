"""The affine traceback's short-chain kernel (traceback_affine_fast_kernel, bialign_trace_fast.hpp) against its test
partner, the generic kernel (BIALIGN_TRACE_FAST=0), and the CPU oracle: scores, traces, lengths and completeness, at the
smallest shapes that exercise each mechanism -- the table of candidates, the carried row across strip changes, the side
path through full records, the LDS trace buffer and its flushes, the clip at trace_cap.  Records are packed by
BIALIGN_PACK=1 wherever the layout allows; where it does not (no interior phase at all) the batch walks on the generic
kernel in both runs and only the oracle comparison bites."""
import numpy as np
import pytest

from bialign_amd import synth

pytestmark = pytest.mark.gpu


def run(pairs, params, monkeypatch, fast, **kw):
    from bialign_amd.batch import make_batch
    monkeypatch.setenv("BIALIGN_TRACE_FAST", "1" if fast else "0")
    b = make_batch(pairs, params, **kw)
    b.run()
    traces, ok = b.traces()
    out = dict(scores=np.array(b.scores()), traces=[np.array(t) for t in traces], ok=np.array(ok), packed=b.timing()["packed_records"])
    b.close()
    return out


def both(pairs, params, monkeypatch, **kw):
    """Both kernels on the same batch: identical in everything they write."""
    fast, generic = run(pairs, params, monkeypatch, True, **kw), run(pairs, params, monkeypatch, False, **kw)
    assert fast["packed"] == generic["packed"]
    np.testing.assert_array_equal(fast["scores"], generic["scores"])
    np.testing.assert_array_equal(fast["ok"], generic["ok"])
    assert [len(t) for t in fast["traces"]] == [len(t) for t in generic["traces"]]
    for x, y in zip(fast["traces"], generic["traces"]):
        np.testing.assert_array_equal(x, y)
    return fast


def against_oracle(got, pairs, params, which=None):
    from oracle import oracle
    from bialign_amd.engine import trace_codes_to_columns
    for t in (range(len(pairs)) if which is None else which):
        ref = oracle.solve(*pairs[t], params)
        assert int(got["scores"][t]) == ref["score"]
        assert trace_codes_to_columns(got["traces"][t]) == oracle.trace_to_lists(ref["trace"])
        assert bool(got["ok"][t]) == ref["complete"]


# the three extra shapes per max_shift are the smallest with all-interior columns in several strips (tests/trace_fast_check.hip)
@pytest.mark.parametrize("n,m,s,packed", [(45, 45, 1, True), (47, 61, 1, True), (130, 97, 1, True), (97, 230, 1, True),
                                           (25, 30, 2, False), (60, 41, 2, True), (41, 120, 2, True),
                                           (20, 26, 3, False), (50, 37, 3, True), (37, 90, 3, True)])
def test_shapes(n, m, s, packed, monkeypatch):
    """Three or more strips (RR = 20, 11, 8), ragged, walks that cross strip changes."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs, params = [synth.protein_pair(6100 + n + s, n, m)], dict(synth.PROTEIN_PARAMS, max_shift=s)
    got = both(pairs, params, monkeypatch)
    assert got["packed"] == packed
    against_oracle(got, pairs, params)


def test_one_strip_nothing_interior(monkeypatch):
    """n < RR: every column takes the side path."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs, params = [synth.protein_pair(6200, 12, 60)], dict(synth.PROTEIN_PARAMS)
    got = both(pairs, params, monkeypatch)
    assert got["packed"]
    against_oracle(got, pairs, params)


@pytest.mark.parametrize("s,beta", [(1, 0), (2, 0), (1, -1), (2, -1), (3, -1)])
def test_ties_decided_by_the_look_ahead(s, beta, monkeypatch):
    """shift_cost = 0 and gap_opening_cost = 0: many candidates reproduce a cell.  (gap_opening_cost = 0 selects the
    one-layer recurrence, whose kernels are not touched: that case only shows the switch leaves it alone.  With
    gap_opening_cost = -1 the recurrence is the affine one, packed, and the key of pyx:554-565 picks among the ties.)"""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    params = dict(synth.PROTEIN_PARAMS, max_shift=s, shift_cost=0, gap_opening_cost=beta)
    pairs = [synth.protein_pair(6300 + s, 90, 140)]
    got = both(pairs, params, monkeypatch)
    assert got["packed"] == (beta != 0)
    against_oracle(got, pairs, params)


def test_rna_toy(monkeypatch):
    """The README's RNA toy (score 6800) and a longer RNA pair."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    toy = ("GCGGGGGAUAUCCCCAUCG", "GGGGAUAUCCCCAUCG", "...(((.....))).....", ".(((.....)))....")
    params = dict(synth.RNA_PARAMS)
    got = both([toy], params, monkeypatch)   # too short for a packed record: the generic kernel, whatever the switch
    assert int(got["scores"][0]) == 6800 and not got["packed"]
    against_oracle(got, [toy], params)
    pairs = [synth.rna_pair(6400, 80, 130)]
    got = both(pairs, params, monkeypatch)
    assert got["packed"]
    against_oracle(got, pairs, params)


def test_ragged_batch_of_70(monkeypatch):
    """order[] and the per-pair offsets: 70 pairs of different lengths, every one against the generic kernel, six against
    the oracle."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs = [synth.protein_pair(6500 + t, 30 + (37 * t) % 120, 50 + (53 * t) % 110) for t in range(70)]
    params = dict(synth.PROTEIN_PARAMS)
    got = both(pairs, params, monkeypatch)
    assert got["packed"]
    against_oracle(got, pairs, params, which=(0, 13, 29, 44, 58, 69))


def test_trace_cap_clips(monkeypatch):
    """A trace_cap below the trace's length: the first trace_cap columns of the walk, i.e. the trace's tail -- with the
    whole clipped trace in LDS, and flushed in pieces."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs, params = [synth.protein_pair(6600, 130, 140)], dict(synth.PROTEIN_PARAMS)
    full = run(pairs, params, monkeypatch, True)
    against_oracle(full, pairs, params)
    assert len(full["traces"][0]) > 150
    for lds in (None, "64"):
        if lds:
            monkeypatch.setenv("BIALIGN_TRACE_LDS", lds)
        monkeypatch.setenv("BIALIGN_TRACE_CAP", "150")
        got = both(pairs, params, monkeypatch)
        monkeypatch.delenv("BIALIGN_TRACE_CAP")
        assert len(got["traces"][0]) == 150 and int(got["scores"][0]) == int(full["scores"][0])
        np.testing.assert_array_equal(got["traces"][0], full["traces"][0][-150:])


@pytest.mark.parametrize("lds", ["256", "64"])
def test_trace_buffer_flushes(lds, monkeypatch):
    """(700, 650) with a trace buffer of 256 bytes (and of 64): the trace leaves LDS in three and more pieces, laid from
    the end of the pair's trace bytes and moved to the front."""
    monkeypatch.setenv("BIALIGN_TRACE_LDS", lds)
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs, params = [synth.protein_pair(6700, 700, 650), synth.protein_pair(6701, 90, 300)], dict(synth.PROTEIN_PARAMS)
    got = both(pairs, params, monkeypatch)
    assert got["packed"] and len(got["traces"][0]) > 3 * int(lds)
    against_oracle(got, pairs, params)


def test_dense_mu2_packed_still_runs(monkeypatch):
    """A dense-mu2 packed batch takes the generic kernel whatever the switch says, and matches the oracle."""
    from oracle import oracle
    from bialign_amd.engine import trace_codes_to_columns
    rng = np.random.default_rng(67)
    shapes = [(150, 170), (90, 220)]
    pairs = [synth.rna_pair(6800 + t, n, m) for t, (n, m) in enumerate(shapes)]
    tabs = [rng.integers(0, 1200, size=(n, m)).astype(np.int32) for n, m in shapes]
    params = dict(synth.RNA_PARAMS, max_shift=1)
    got = both(pairs, params, monkeypatch, mu2_dense=tabs)
    assert got["packed"]
    for t, (pair, (n, m)) in enumerate(zip(pairs, shapes)):
        mu1, _ = oracle.mu_tables(*pair, params)
        mu2 = np.zeros((n + 1, m + 1), dtype=np.int32)
        mu2[1:, 1:] = tabs[t]
        ref = oracle.solve_tables(n, m, params, mu1, mu2)
        assert int(got["scores"][t]) == ref["score"]
        assert trace_codes_to_columns(got["traces"][t]) == oracle.trace_to_lists(ref["trace"])
