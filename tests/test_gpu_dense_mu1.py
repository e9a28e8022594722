"""GPU parity of the DENSE-mu1 form of the C ABI (bialign_pairs.mu1_dense, ABI 10): per-pair tables of
position-specific sequence scores.  Against golden vectors of the compiled reference, against the LOOKUP form
on the same scores, and against the oracle on random tables in every storage mode, team shape and band width."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from bialign_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("dense_mu1.json")
LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)


def run(pairs, params, mu1=None, mu2=None, layers=False, budget=0, score_only=False, lean_trace=False):
    from bialign_amd.batch import make_batch
    from bialign_amd.engine import trace_codes_to_columns
    b = make_batch(pairs, params, mu1_dense=mu1, mu2_dense=mu2, hbm_budget_bytes=budget,
                   score_only=score_only, lean_trace=lean_trace)
    b.run()
    out = dict(scores=[int(v) for v in b.scores()], timing=b.timing(), info=dict(b.info))
    if not score_only:
        traces, ok = b.traces()
        out["traces"], out["complete"] = [trace_codes_to_columns(t) for t in traces], [bool(v) for v in ok]
    if layers:
        out["layers"] = b.dump_layers(0)
    b.close()
    return out


def table(rng, n, m, lo=-300, hi=900):
    return rng.integers(lo, hi + 1, size=(n, m)).astype(np.int32)


def check(got, pair, params, t1, t2=None, p=0):
    """got (pair p) against the oracle on the same tables: score, trace, completeness, layers if dumped."""
    from oracle import oracle
    (sa, sb, ta, tb), s = pair, params["max_shift"]
    n, m = len(sa), len(sb)
    _, mu2 = oracle.mu_tables(sa, sb, ta, tb, params)
    mu1 = np.zeros((n + 1, m + 1), dtype=np.int64)
    mu1[1:, 1:] = t1
    if t2 is not None:
        mu2 = np.zeros((n + 1, m + 1), dtype=np.int64)
        mu2[1:, 1:] = t2
    ref = oracle.solve_tables(n, m, params, mu1, mu2)
    assert got["scores"][p] == ref["score"]
    if "traces" in got:
        assert got["traces"][p] == oracle.trace_to_lists(ref["trace"])
        assert got["complete"][p] == ref["complete"]
    if "layers" in got:
        for g, e in zip(oracle.band_values(got["layers"], n, m, s), oracle.band_values(ref["layers"], n, m, s)):
            np.testing.assert_array_equal(g, e)


@pytest.mark.parametrize("rec", GOLDEN, ids=[r["name"] for r in GOLDEN])
def test_golden_through_the_c_abi_and_bialigner(rec):
    import contextlib
    import io
    from oracle import oracle
    from bialign_amd import bialignment as ba
    pair, tab = (rec["seqA"], rec["seqB"], rec["strA"], rec["strB"]), np.asarray(rec["mu1"])
    got = run([pair], rec["params"], mu1=[tab], layers="layers" in rec)
    assert (got["scores"][0], got["traces"][0], got["complete"][0]) == (rec["score"], rec["trace"], rec["complete"])
    if "layers" in rec:
        n, m, s = len(rec["seqA"]), len(rec["seqB"]), rec["params"]["max_shift"]
        for g, e in zip(oracle.band_values(got["layers"], n, m, s), rec["layers"]):
            np.testing.assert_array_equal(np.ravel(g), np.ravel(e))
    b = ba.BiAligner(*pair, seq_similarity=tab, **rec["params"])
    assert int(b.optimize()) == rec["score"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        trace = b.traceback()
    assert [[int(v) for v in col] for col in trace] == rec["trace"]
    assert ("WARNING" not in buf.getvalue()) == rec["complete"]
    assert all(isinstance(x, str) for x in b.decode_trace(trace))


@pytest.mark.parametrize("s", range(6))
@pytest.mark.parametrize("ov", [{}, LIN], ids=["affine", "linear"])
def test_table_of_the_lookup_scores_equals_the_lookup_form(s, ov):
    from bialign_amd.batch import encode_flat
    pair = synth.protein_pair(400 + s, 90, 83)
    params = dict(synth.PROTEIN_PARAMS, max_shift=s, **ov)
    model, fb = encode_flat([pair], params)
    want = run([pair], params, layers=True)
    got = run([pair], params, mu1=[model.s1[np.ix_(fb.seq_a, fb.seq_b)]], layers=True)
    assert (got["scores"], got["traces"], got["complete"]) == (want["scores"], want["traces"], want["complete"])
    np.testing.assert_array_equal(got["layers"], want["layers"])


@pytest.mark.parametrize("n,m,s,seed,ov,team,both", [
    (130, 75, 1, 11, {}, None, False), (75, 130, 2, 12, {}, None, False), (200, 190, 0, 13, {}, None, False),
    (61, 64, 3, 14, {}, None, False), (40, 50, 4, 15, {}, None, False), (33, 45, 5, 16, {}, None, False),
    (257, 129, 1, 17, dict(gap_opening_cost=100), None, False), (60, 70, 3, 18, dict(gap_opening_cost=50), None, True),
    (130, 75, 1, 19, LIN, None, False), (75, 130, 2, 20, LIN, None, False), (50, 60, 3, 21, LIN, None, False),
    (33, 45, 5, 22, LIN, None, True),
    (300, 310, 1, 23, {}, "2", False), (170, 400, 1, 24, {}, "4", True), (100, 300, 2, 25, {}, "4", False),
    (330, 650, 1, 26, {}, "x4", False), (200, 400, 2, 27, {}, "x5", True), (420, 400, 0, 28, {}, "2", True),
    (300, 320, 1, 29, LIN, "2", False), (330, 650, 1, 30, LIN, "x4", True)])
def test_random_tables_vs_oracle(n, m, s, seed, ov, team, both, monkeypatch):
    """Every layer cell, score and trace; teams in a workgroup and across CUs; dense mu1 alone and with dense mu2."""
    if team:
        monkeypatch.setenv("BIALIGN_TEAM", team)
    rng = np.random.default_rng(seed)
    pair = synth.protein_pair(seed, n, m)
    params = dict(synth.PROTEIN_PARAMS, max_shift=s, **ov)
    t1, t2 = table(rng, n, m), (table(rng, n, m, -100, 400) if both else None)
    got = run([pair], params, mu1=[t1], mu2=None if t2 is None else [t2], layers=True)
    if team:
        assert got["timing"]["waves_per_pair"] == int(team.lstrip("x"))
        assert got["timing"]["cross_cu"] == team.startswith("x")
    check(got, pair, params, t1, t2)


@pytest.mark.parametrize("s", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("ov", [{}, LIN], ids=["affine", "linear"])
def test_reduced_storage_vs_oracle(s, ov):
    t1 = table(np.random.default_rng(40 + s), 300, 140)
    pair = synth.protein_pair(40 + s, 300, 140)
    params = dict(synth.PROTEIN_PARAMS, max_shift=s, **ov)
    check(run([pair], params, mu1=[t1], score_only=True), pair, params, t1)
    check(run([pair], params, mu1=[t1], lean_trace=True), pair, params, t1)
    full = run([pair], params, mu1=[t1])["info"]["hbm_layer_bytes"]
    got = run([pair], params, mu1=[t1], budget=full * 3 // 4)  # full layers do not fit: the engine picks the lean traceback
    assert got["info"]["storage"] == 2
    check(got, pair, params, t1)


@pytest.mark.parametrize("s", [6, 8])
@pytest.mark.parametrize("parts", [None, "1"])
def test_wide_band_vs_oracle(s, parts, monkeypatch):
    if parts:
        monkeypatch.setenv("BIALIGN_WIDE_PARTS", parts)
    rng = np.random.default_rng(60 + s)
    pair = synth.protein_pair(60 + s, 40, 36)
    for ov, both in (({}, False), (LIN, False), ({}, True)):
        params = dict(synth.PROTEIN_PARAMS, max_shift=s, **ov)
        t1, t2 = table(rng, 40, 36), (table(rng, 40, 36, -100, 400) if both else None)
        mu2 = None if t2 is None else [t2]
        check(run([pair], params, mu1=[t1], mu2=mu2, layers=True), pair, params, t1, t2)
        if params["gap_opening_cost"]:
            check(run([pair], params, mu1=[t1], mu2=mu2, score_only=True), pair, params, t1, t2)


def test_ragged_batch_chunked():
    rng = np.random.default_rng(70)
    shapes = [(40, 33), (5, 90), (90, 5), (64, 64), (1, 1), (17, 18), (100, 100), (2, 50), (1, 70), (70, 1)]
    pairs = [synth.protein_pair(500 + t, n, m) for t, (n, m) in enumerate(shapes)]
    tabs = [table(rng, n, m) for n, m in shapes]
    for params in (dict(synth.PROTEIN_PARAMS), dict(synth.PROTEIN_PARAMS, max_shift=2, **LIN)):
        got = run(pairs, params, mu1=tabs, budget=5 << 20)
        assert got["info"]["nchunks"] > 1 or not params["gap_opening_cost"]
        for t, pair in enumerate(pairs):
            check(got, pair, params, tabs[t], p=t)


def test_raw_abi_null_codes_and_errors():
    """Through raw ctypes: NULL sequence codes with a one-entry s1 work; no mu1_off is E_INVALID; |mu1| near 2^28
    is E_RANGE.  A table of the wrong shape is a ValueError in Python."""
    from bialign_amd import _lib
    from bialign_amd.batch import encode_flat, make_batch
    from bialign_amd.engine import default_engine
    pair, params = synth.protein_pair(80, 60, 50), dict(synth.PROTEIN_PARAMS)
    model, fb = encode_flat([pair], params)
    s1, s2, off = np.zeros((1, 1), np.int32), np.ascontiguousarray(model.s2, np.int32), np.zeros(1, np.int64)
    p = lambda a, t: a.ctypes.data_as(t)

    def create(tab, with_off=True):
        prm = _lib.Params(params["gap_opening_cost"], params["gap_cost"], params["shift_cost"], 1, 0, 0)
        sc = _lib.Scoring(1, p(s1, _lib.c_i32p), s2.shape[0], p(s2, _lib.c_i32p))
        pr = _lib.Pairs(1, p(fb.len_a, _lib.c_i32p), p(fb.len_b, _lib.c_i32p), p(fb.off_a, _lib.c_i64p),
                        p(fb.off_b, _lib.c_i64p), None, p(fb.cls_a, _lib.c_u8p), None, p(fb.cls_b, _lib.c_u8p),
                        None, None, p(tab, _lib.c_i32p), p(off, _lib.c_i64p) if with_off else None)
        h = ctypes.c_void_p()
        return _lib.lib.bialign_batch_create(default_engine()._h, ctypes.byref(prm), ctypes.byref(sc),
                                             ctypes.byref(pr), 0, ctypes.byref(h)), h

    tab = table(np.random.default_rng(80), 60, 50)
    rc, h = create(tab)
    assert rc == 0, _lib.lib.bialign_last_error()
    try:
        assert _lib.lib.bialign_batch_run(h, _lib.RUN_FILL_ONLY) == 0
        out = np.zeros(1, dtype=np.int32)
        assert _lib.lib.bialign_batch_get_scores(h, p(out, _lib.c_i32p)) == 0
    finally:
        _lib.lib.bialign_batch_destroy(h)
    check(dict(scores=[int(out[0])]), pair, params, tab)
    assert create(tab, with_off=False)[0] == _lib.E_INVALID
    assert create(np.full((60, 50), (1 << 28) - 5, dtype=np.int32))[0] == _lib.E_RANGE
    for bad in ([np.zeros((60, 49), dtype=np.int32)], []):
        with pytest.raises(ValueError):
            make_batch([pair], params, mu1_dense=bad)


def test_fuzz_against_oracle():
    import time
    rng = np.random.default_rng(82)
    t0, it = time.time(), 0
    while time.time() - t0 < 30 and it < 400:
        s, n, m = int(rng.integers(0, 8)), int(rng.integers(1, 60)), int(rng.integers(1, 60))
        affine = bool(rng.integers(0, 2))
        params = dict(synth.PROTEIN_PARAMS, max_shift=s, gap_opening_cost=int(rng.integers(-300, 60)) or -1 if affine else 0,
                      gap_cost=int(rng.integers(-300, 1)), shift_cost=int(rng.integers(-400, 1)))
        pair = synth.protein_pair(600 + it, n, m)
        t1 = table(rng, n, m, lo=int(rng.integers(-2000, 1)), hi=int(rng.integers(0, 3000)))
        t2 = table(rng, n, m) if rng.integers(0, 3) == 0 else None
        lean = s <= 5 and rng.integers(0, 3) == 0
        got = run([pair], params, mu1=[t1], mu2=None if t2 is None else [t2], lean_trace=lean)
        check(got, pair, params, t1, t2)
        it += 1
    assert it >= 20
