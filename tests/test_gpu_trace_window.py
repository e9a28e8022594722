"""The LDS window of the affine traceback's short-chain kernel (TraceWindow, bialign_trace_fast.hpp): the walk with the
window against the same kernel without it (BIALIGN_TRACE_WINDOW=0), against the generic kernel (BIALIGN_TRACE_FAST=0) and,
for a sample, against the CPU oracle -- scores, traces, lengths and completeness, bit for bit.  The window only changes
where a value is read from, so nothing may differ.  Shapes: three strips and more with columns beyond LO + 3, long
one-sided gap runs (the slot drift's extremes), max_shift 2 (a window of three DMA instructions per record) and 3 (no
window: the switch must leave that walk alone).  Every case also runs with the shortest ring (BIALIGN_TRACE_WINDOW_K=4:
no lead, every record waited for at once), where refills and wraps come every column."""
import numpy as np
import pytest

from bialign_amd import synth

pytestmark = pytest.mark.gpu

MODES = {"window": {}, "window_k4": {"BIALIGN_TRACE_WINDOW_K": "4"}, "no_window": {"BIALIGN_TRACE_WINDOW": "0"},
         "generic": {"BIALIGN_TRACE_FAST": "0"}}


def run(pairs, params, monkeypatch, mode, **kw):
    from bialign_amd.batch import make_batch
    for name in ("BIALIGN_TRACE_WINDOW_K", "BIALIGN_TRACE_WINDOW", "BIALIGN_TRACE_FAST"):
        monkeypatch.delenv(name, raising=False)
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    b = make_batch(pairs, params, **kw)
    b.run()
    traces, ok = b.traces()
    out = dict(scores=np.array(b.scores()), traces=[np.array(t) for t in traces], ok=np.array(ok), packed=b.timing()["packed_records"])
    b.close()
    return out


def all_modes(pairs, params, monkeypatch, **kw):
    """Every mode on the same batch: identical in everything they write."""
    ref = run(pairs, params, monkeypatch, "generic", **kw)
    for mode in ("window", "window_k4", "no_window"):
        got = run(pairs, params, monkeypatch, mode, **kw)
        assert got["packed"] == ref["packed"], mode
        np.testing.assert_array_equal(got["scores"], ref["scores"], err_msg=mode)
        np.testing.assert_array_equal(got["ok"], ref["ok"], err_msg=mode)
        assert [len(t) for t in got["traces"]] == [len(t) for t in ref["traces"]], mode
        for x, y in zip(got["traces"], ref["traces"]):
            np.testing.assert_array_equal(x, y, err_msg=mode)
    return ref


def against_oracle(got, pairs, params, which=None):
    from oracle import oracle
    from bialign_amd.engine import trace_codes_to_columns
    for t in (range(len(pairs)) if which is None else which):
        ref = oracle.solve(*pairs[t], params)
        assert int(got["scores"][t]) == ref["score"]
        assert trace_codes_to_columns(got["traces"][t]) == oracle.trace_to_lists(ref["trace"])
        assert bool(got["ok"][t]) == ref["complete"]


# (130, 41) at max_shift 1: m < LO + 3, no interior phase and no packed record -- the batch walks on the generic kernel in
# every mode and only the oracle comparison bites
SHAPES = [(45, 70, 1), (64, 64, 1), (41, 130, 1), (130, 41, 1), (100, 100, 2), (100, 100, 3)]


@pytest.mark.parametrize("n,m,s", SHAPES)
def test_protein_shapes(n, m, s, monkeypatch):
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs, params = [synth.protein_pair(9100 + n + s, n, m)], dict(synth.PROTEIN_PARAMS, max_shift=s)
    got = all_modes(pairs, params, monkeypatch)
    assert got["packed"] == ((n, m) != (130, 41))
    against_oracle(got, pairs, params)


@pytest.mark.parametrize("n,m,s", SHAPES)
def test_rna_shapes(n, m, s, monkeypatch):
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs, params = [synth.rna_pair(9200 + n + s, n, m)], dict(synth.RNA_PARAMS, max_shift=s)
    got = all_modes(pairs, params, monkeypatch)
    assert got["packed"] == ((n, m) != (130, 41))
    if s < 3:
        against_oracle(got, pairs, params)


@pytest.mark.parametrize("s", [1, 2])
def test_mixed_shapes_in_one_launch(s, monkeypatch):
    """order[] and the per-pair strips: each workgroup keeps a window of its own pair."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    shapes = [(45, 70), (64, 64), (41, 130), (130, 60), (100, 100), (150, 90), (33, 200), (97, 230)]
    pairs = [synth.protein_pair(9300 + t, n, m) for t, (n, m) in enumerate(shapes)]
    params = dict(synth.PROTEIN_PARAMS, max_shift=s)
    got = all_modes(pairs, params, monkeypatch)
    assert got["packed"]
    against_oracle(got, pairs, params, which=(2, 5, 7))


def test_trace_buffer_flushes_while_the_window_is_live(monkeypatch):
    """A 64-byte trace buffer: the flushes' stores (two and more per trace) run between the window's DMAs and their counted
    waits."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    monkeypatch.setenv("BIALIGN_TRACE_LDS", "64")
    pairs, params = [synth.protein_pair(9400, 130, 160), synth.protein_pair(9401, 41, 130)], dict(synth.PROTEIN_PARAMS)
    got = all_modes(pairs, params, monkeypatch)
    assert got["packed"] and len(got["traces"][0]) > 2 * 64
    against_oracle(got, pairs, params)


def test_trace_cap_below_the_longest_trace(monkeypatch):
    """trace_cap = 150 < 2 (n + m) + 2: the walk goes on past the cap, window and all, and keeps the trace's tail."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    pairs, params = [synth.protein_pair(9500, 130, 140)], dict(synth.PROTEIN_PARAMS)
    full = run(pairs, params, monkeypatch, "window")
    against_oracle(full, pairs, params)
    assert len(full["traces"][0]) > 150
    monkeypatch.setenv("BIALIGN_TRACE_CAP", "150")
    got = all_modes(pairs, params, monkeypatch)
    assert len(got["traces"][0]) == 150 and int(got["scores"][0]) == int(full["scores"][0])
    np.testing.assert_array_equal(got["traces"][0], full["traces"][0][-150:])
