"""The scalar addressing of fill_affine_slim_kernel's interior steps (a scalar record base plus lane
constants for the stores, a one-instruction ghost source, unclamped code fetches, scalar mirrors of lane 0's column and
strip) computes what the per-lane form computed: score, trace, completeness flag and every dumped layer cell against the
oracle, and the same against the two-wave kernel (BIALIGN_SLIM=0), which keeps the per-lane form.
tests/test_step_addr_host.py proves the addresses themselves on the CPU.

Two of the shapes admit no slim team (team_shape(): T * 72 + 64 <= P, P >= 256 and two strips per wave): m = 46 has P = 64,
and n = 45 has three strips.  They run on whatever kernel the host picks -- what they pin is the layout around the first
interior run and around strips that end mid-block, which both kernels share."""
import numpy as np
import pytest

from bialign_amd import synth

pytestmark = pytest.mark.gpu

PARAMS = dict(synth.PROTEIN_PARAMS)      # max_shift 1, affine


def run_batch(pairs, params, dump=(), **kw):
    from bialign_amd.batch import make_batch
    b = make_batch(pairs, params, **kw)
    b.run()
    out = dict(timing=b.timing(), info=dict(b.info), scores=[int(x) for x in b.scores()], traces=None, ok=None)
    if not kw.get("score_only"):
        traces, ok = b.traces()
        out["traces"], out["ok"] = [np.array(t) for t in traces], [bool(x) for x in ok]
    out["layers"] = {k: b.dump_layers(k) for k in dump}
    b.close()
    return out


def check(pairs, params, monkeypatch, team=None, dump=(), slim_team=None, **kw):
    """Oracle parity of the batch, then the same batch on the two-wave kernel: everything equal."""
    from oracle import oracle
    from bialign_amd.engine import trace_codes_to_columns
    s = params["max_shift"]
    monkeypatch.setenv("BIALIGN_PACK", "1")
    if team is not None:
        monkeypatch.setenv("BIALIGN_TEAM", str(team))
    got = run_batch(pairs, params, dump=dump, **kw)
    t = got["timing"]
    print(dict(waves=t["waves_per_pair"], packed=t["packed_records"], recovered=t["recovered_runs"], nchunks=got["info"].get("nchunks")))
    assert t["recovered_runs"] == 0
    if slim_team is not None:
        assert t["waves_per_pair"] == slim_team
    refs = [oracle.solve(*pair, params) for pair in pairs]
    for k, ref in enumerate(refs):
        assert got["scores"][k] == ref["score"], k
        if got["traces"] is not None:
            assert trace_codes_to_columns(got["traces"][k]) == oracle.trace_to_lists(ref["trace"]), k
            assert got["ok"][k] == ref["complete"], k
    for k in dump:
        n, m = len(pairs[k][0]), len(pairs[k][1])
        for g, e in zip(oracle.band_values(got["layers"][k], n, m, s), oracle.band_values(refs[k]["layers"], n, m, s)):
            np.testing.assert_array_equal(g, e)
    monkeypatch.setenv("BIALIGN_SLIM", "0")
    monkeypatch.delenv("BIALIGN_TEAM", raising=False)
    old = run_batch(pairs, params, dump=dump, **kw)
    assert old["timing"]["recovered_runs"] == 0
    assert old["scores"] == got["scores"] and old["ok"] == got["ok"]
    if got["traces"] is not None:
        for a, b in zip(old["traces"], got["traces"]):
            np.testing.assert_array_equal(a, b)
    for k in dump:
        n, m = len(pairs[k][0]), len(pairs[k][1])
        for g, e in zip(oracle.band_values(got["layers"][k], n, m, s), oracle.band_values(old["layers"][k], n, m, s)):
            np.testing.assert_array_equal(g, e)
    return got


def test_first_interior_run(monkeypatch):
    """m = 46 is the first m with an interior step (LO = 44 <= m - 1): one run of two steps per strip; n = 41 is the first
    length with three strips, so with strips beyond Q0."""
    check([synth.protein_pair(8146, 41, 46)], PARAMS, monkeypatch, dump=(0,))


def test_teams_of_three_strips_end_mid_block(monkeypatch):
    """n = 45, m = 300: P = 302 is no multiple of the ghost block, so a strip ends mid-block and partners start their
    interior runs at different steps of a block.  (Three strips admit no team: see the module's docstring.)"""
    check([synth.protein_pair(8245, 45, 300)], PARAMS, monkeypatch, team=3, dump=(0,))


def test_teams_of_three_strips_end_mid_block_on_the_slim_kernel(monkeypatch):
    """... and the same period with six strips, which the three-wave kernel takes in teams of three."""
    check([synth.protein_pair(8210, 110, 300)], PARAMS, monkeypatch, team=3, dump=(0,), slim_team=3)


def test_teams_of_three_part_filled_last_strip(monkeypatch):
    """n = 130, m = 278: P = 280 is the shortest period that admits teams of three; the seventh strip holds eleven rows,
    so storing lanes of rows beyond n write their slots of the last records."""
    check([synth.protein_pair(8330, 130, 278)], PARAMS, monkeypatch, team=3, dump=(0,), slim_team=3)


def test_ragged_batch_one_base_per_wave(monkeypatch):
    """Five pairs of different (n, m, P) in teams of three: a workgroup holds four pairs, each wave its own scalar base."""
    shapes = [(110, 280), (127, 301), (141, 288), (118, 333), (163, 295)]
    pairs = [synth.protein_pair(8400 + t, n, m) for t, (n, m) in enumerate(shapes)]
    check(pairs, PARAMS, monkeypatch, team=3, dump=(1, 4), slim_team=3)


def test_chunked_batch_layer_offsets_differ(monkeypatch):
    """A small HBM budget cuts three pairs into chunks: the pairs' storage starts at different offsets of the buffer."""
    from bialign_amd.batch import make_batch
    pairs = [synth.protein_pair(8500 + t, 110 + 7 * t, 280 + 5 * t) for t in range(3)]
    monkeypatch.setenv("BIALIGN_PACK", "1")
    probe = make_batch(pairs, PARAMS)
    one_chunk = probe.info["hbm_layer_bytes"]
    assert probe.info["nchunks"] == 1
    probe.close()
    got = check(pairs, PARAMS, monkeypatch, team=3, dump=(0, 2), slim_team=3, hbm_budget_bytes=int(one_chunk * 0.75))
    assert got["info"]["nchunks"] > 1


@pytest.mark.parametrize("mode", ["score_only", "lean_trace"])
def test_reduced_storage_lean_stores(mode, monkeypatch):
    """Score-only batches and the lean traceback's sweep take the LEAN form: the bottom row's plain records."""
    pairs = [synth.protein_pair(8600 + t, n, m) for t, (n, m) in enumerate([(130, 278), (110, 300)])]
    check(pairs, PARAMS, monkeypatch, team=3, slim_team=3, **{mode: True})
