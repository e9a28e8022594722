"""DENSE-form null batches (bialign_batch_create_null_dense): pairs scored through dense mu1 and / or mu2 tables against
shuffles of B made on the GPU -- every replica's tables are the real pair's with their columns permuted, chunk by chunk,
from the one uploaded copy.  The replicas' tables and codes against the Python mirror bit for bit, the scores against the
CPU oracle on the real tables with permuted B columns and against a host-expanded DENSE batch, the reduction against
numpy; all comparisons exact."""
import ctypes
import functools

import numpy as np
import pytest

from bialign_amd import significance as sg
from bialign_amd import synth

pytestmark = pytest.mark.gpu

LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
FORMS = ("mu1", "mu2", "both")
SHAPES = [(20, 37), (33, 21), (40, 28), (26, 26)]   # the scored pairs: 20..40 residues


def marked_tables(pairs):
    """Distinct values, i * 1000 + j for mu1 and its negative for mu2: a wrong row or column shows."""
    mu1 = [np.arange(len(a), dtype=np.int32)[:, None] * 1000 + np.arange(len(b), dtype=np.int32)[None, :] for a, b, _, _ in pairs]
    return mu1, [-t for t in mu1]


def random_tables(pairs, seed):
    """mu1 like a PSSM in the x100 scale of the score tables, mu2 like structure scores: random integers."""
    rng = np.random.default_rng(seed)
    mu1 = [rng.integers(-400, 1100, size=(len(a), len(b)), dtype=np.int32) for a, b, _, _ in pairs]
    mu2 = [rng.integers(0, 800, size=(len(a), len(b)), dtype=np.int32) for a, b, _, _ in pairs]
    return mu1, mu2


def form_kw(form, mu1, mu2):
    return dict(mu1_dense=mu1 if form in ("mu1", "both") else None, mu2_dense=mu2 if form in ("mu2", "both") else None)


def run_null(pairs, params, R, seed=0, **kw):
    b = sg.null_dense_batch(pairs, params, R, seed=seed, **kw)
    b.run()
    out = b.null_scores().copy(), dict(b.current_info()), b.timing(), b.feature_info()
    b.close()
    return out


def check_replica(b, p, r, seed, form, mu1, mu2, mols_b, msg):
    """Tables and codes of replica r of pair p as the batch holds them, against the mirror."""
    got1, got2 = b.null_tables(p, r)
    seq, cls = b.dump_null_codes(p, r)
    perm = sg.permutation(seed, p, r, mu1[p].shape[1])
    if form in ("mu1", "both"):
        assert got1.dtype == np.int32
        np.testing.assert_array_equal(got1, sg.shuffle_tables(mu1[p], seed, p, r), err_msg=msg)
        assert not seq.any()                                                  # the codes a dense form replaces: zeros
    else:
        assert got1 is None
        np.testing.assert_array_equal(seq, mols_b[p][0][perm], err_msg=msg)   # the LOOKUP side moves with the same perm
    if form in ("mu2", "both"):
        np.testing.assert_array_equal(got2, sg.shuffle_tables(mu2[p], seed, p, r), err_msg=msg)
        assert not cls.any()
    else:
        assert got2 is None
        np.testing.assert_array_equal(cls, mols_b[p][1][perm], err_msg=msg)


# ---- 1. the replicas' tables and codes against the mirror

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("R", [1, 7])
def test_tables_and_codes_equal_mirror(R, form):
    from bialign_amd.batch import encode_flat
    # len B: less than a wave, one wave less one, exactly one, one more, two and a bit; len A: one row, exactly a tile of
    # rows, one more, two tiles and a row
    shapes = [(n, m) for m in (1, 2, 63, 64, 65, 130) for n in (1, 16, 17, 33)]
    pairs = [synth.protein_pair(8500 + t, n, m) for t, (n, m) in enumerate(shapes)]
    params = dict(synth.PROTEIN_PARAMS)
    mu1, mu2 = marked_tables(pairs)
    kw = form_kw(form, mu1, mu2)
    mols_b = encode_flat(pairs, params)[1].molecules("b")
    seed, nforms = 77, 2 if form == "both" else 1
    whole = sg.null_dense_batch(pairs, params, R, seed=seed, **kw)
    info, finfo = whole.info, whole.feature_info()
    whole.close()
    assert info["nchunks"] == 1 and finfo["table_bytes"] == 4 * nforms * R * sum(n * m for n, m in shapes)
    # a third of what one chunk took: cut into several chunks, so that the scratch holds other chunks' tables in between
    b = sg.null_dense_batch(pairs, params, R, seed=seed, hbm_budget_bytes=(info["hbm_layer_bytes"] + finfo["table_bytes"]) // 3, **kw)
    assert b.info["npairs"] == len(pairs) and b.info["nchunks"] > 1
    assert b.null_info()["replica_bytes"] == (2 + 2) * R * sum(m for _, m in shapes)   # codes of both kinds, 16-bit permutations
    assert b.feature_info()["form"] == ("lookup" if form == "mu1" else "dense")
    for when in ("before run", "after run"):
        for p in range(len(pairs)):
            for r in sorted({0, R - 1}):
                check_replica(b, p, r, seed, form, mu1, mu2, mols_b, f"{when} p={p} r={r}")
        b.run()
    assert b.feature_info()["build_launches"] == b.info["nchunks"]
    b.close()


def test_row_beyond_the_lds_tile_is_gathered_from_global_memory():
    """len B = 16385: one row of a table exceeds the 64 KiB tile.  Values repeat (the int32 safety window leaves no room
    for 16385 distinct ones at this length) but no two neighbouring columns agree."""
    from bialign_amd.batch import make_batch
    n, m, R, seed = 2, 16385, 2, 3
    pairs = [synth.protein_pair(8590, n, m)]
    params = dict(synth.PROTEIN_PARAMS)
    tab = ((np.arange(m, dtype=np.int64)[None, :] * 31 + np.arange(n, dtype=np.int64)[:, None] * 1009) % 3001).astype(np.int32)
    mu1, mu2 = [tab], [-tab]
    b = sg.null_dense_batch(pairs, params, R, seed=seed, mu1_dense=mu1, mu2_dense=mu2)
    for r in range(R):
        check_replica(b, 0, r, seed, "both", mu1, mu2, None, f"r={r}")
    b.run()
    scores = b.null_scores().copy()
    check_replica(b, 0, R - 1, seed, "both", mu1, mu2, None, "after run")
    b.close()
    hb = make_batch([sg.shuffle_b(pairs[0], seed, 0, r) for r in range(R)], params, score_only=True,
                    mu1_dense=[sg.shuffle_tables(tab, seed, 0, r) for r in range(R)],
                    mu2_dense=[sg.shuffle_tables(-tab, seed, 0, r) for r in range(R)])
    hb.run()
    np.testing.assert_array_equal(hb.scores().reshape(1, R), scores)
    hb.close()


# ---- 2. pairs that share one B through off_b

@pytest.mark.parametrize("form", ["mu1", "mu2"])
def test_pairs_sharing_one_b_get_different_shuffles(form):
    from bialign_amd.batch import encode_flat
    from bialign_amd.engine import Batch, default_engine
    pair = synth.protein_pair(8600, 20, 40)
    params = dict(synth.PROTEIN_PARAMS)
    model, fb = encode_flat([pair] * 3, params)
    fb.off_b = np.zeros(3, dtype=np.int64)                      # all three pairs point at the first copy of B
    fb.seq_b, fb.cls_b = fb.seq_b[:40].copy(), fb.cls_b[:40].copy()
    mu1, mu2 = marked_tables([pair] * 3)
    mu1 = [t + 100 * p for p, t in enumerate(mu1)]              # (the pairs' tables differ; B is the same)
    mu2 = [t - 100 * p for p, t in enumerate(mu2)]
    b = Batch(default_engine(), fb, None, model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"],
              params["shift_cost"], params["max_shift"], null_dense=(2, 5), **form_kw(form, mu1, mu2))
    assert b.null_info()["replica_bytes"] == 4 * 2 * 3 * 40     # replicas are per pair, whoever owns the molecule
    mols_b = [(fb.seq_b, fb.cls_b)] * 3
    codes = set()
    for p in range(3):
        for r in range(2):
            check_replica(b, p, r, 5, form, mu1, mu2, mols_b, f"p={p} r={r}")
            codes.add(b.dump_null_codes(p, r)[0 if form == "mu2" else 1].tobytes())
    b.close()
    assert len(codes) == 6


# ---- 3. scores against the oracle: the real pair's tables with their B columns permuted

@functools.lru_cache(maxsize=None)
def scored_pairs():
    pairs = tuple(synth.protein_pair(8700 + t, n, m) for t, (n, m) in enumerate(SHAPES))
    mu1, mu2 = random_tables(pairs, 8700)
    return pairs, mu1, mu2


def check_scores_vs_oracle(params, form, R, seed):
    from oracle import oracle
    pairs, mu1, mu2 = scored_pairs()
    pairs = list(pairs)
    scores, info, _, finfo = run_null(pairs, params, R, seed=seed, **form_kw(form, mu1, mu2))
    assert scores.shape == (len(pairs), R) and info["npairs"] == len(pairs)
    assert info["cells"] == R * sum(synth.cells_per_pair(n, m, params["max_shift"]) for n, m in SHAPES)
    assert finfo["build_launches"] == info["nchunks"]
    for p, pair in enumerate(pairs):
        n, m = SHAPES[p]
        o1, o2 = (np.array(t) for t in oracle.mu_tables(*pair, params))   # the LOOKUP side: the oracle's own tables
        if form in ("mu1", "both"):
            o1[1:, 1:] = mu1[p]
        if form in ("mu2", "both"):
            o2[1:, 1:] = mu2[p]
        for r in range(R):
            cols = np.concatenate([[0], 1 + sg.permutation(seed, p, r, m)])
            want = oracle.solve_tables(n, m, params, o1[:, cols], o2[:, cols], want_trace=False)["score"]
            assert int(scores[p, r]) == want, (p, r)


@pytest.mark.parametrize("s", [0, 1, 2, 5])
@pytest.mark.parametrize("ov", [{}, LIN], ids=["affine", "linear"])
def test_scores_equal_oracle(s, ov):
    form = FORMS[(s + (1 if ov else 0)) % 3]   # every form meets both recurrences
    check_scores_vs_oracle(dict(synth.PROTEIN_PARAMS, max_shift=s, **ov), form, 3, 11 + s)


def test_scores_equal_oracle_wide_band():
    check_scores_vs_oracle(dict(synth.PROTEIN_PARAMS, max_shift=7), "both", 3, 9)


def test_wide_band_rings_are_cut_into_chunks():
    """The batch of test_scores_equal_oracle_wide_band (both tables dense) under a budget of two rings (and 1 MiB: a replica's
    permuted tables are a few KB): several chunks; the same null scores, reductions and z-scores."""
    from oracle import oracle
    from wide_ring import check_chunked_null
    pairs, mu1, mu2 = scored_pairs()
    pairs = list(pairs)
    params, R, seed = dict(synth.PROTEIN_PARAMS, max_shift=7), 3, 9
    want = []
    for p, (n, m) in enumerate(SHAPES):
        o1, o2 = (np.array(t) for t in oracle.mu_tables(*pairs[p], params))
        o1[1:, 1:], o2[1:, 1:] = mu1[p], mu2[p]
        cols = [np.concatenate([[0], 1 + sg.permutation(seed, p, r, m)]) for r in range(R)]
        want.append([oracle.solve_tables(n, m, params, o1[:, c], o2[:, c], want_trace=False)["score"] for c in cols])
    observed = np.array([sorted(row)[R // 2] for row in want], dtype=np.int32)
    kw = form_kw("both", mu1, mu2)
    check_chunked_null(lambda bud: sg.null_dense_batch(pairs, params, R, seed=seed, hbm_budget_bytes=bud, **kw),
                       lambda bud: sg.zscores_dense(pairs, params, replicas=R, seed=seed, hbm_budget_bytes=bud, **kw),
                       [n for n, _ in SHAPES], 7, want, observed)


def test_scores_equal_oracle_general_beta():
    check_scores_vs_oracle(dict(synth.PROTEIN_PARAMS, gap_opening_cost=100), "mu1", 3, 3)


# ---- 4. equals the host-expanded batch, element for element

@pytest.mark.parametrize("form,ov", [("mu1", {}), ("mu2", dict(max_shift=2, **LIN)), ("both", dict(max_shift=2))],
                         ids=["mu1_affine_s1", "mu2_linear_s2", "both_affine_s2"])
def test_equals_host_expanded_dense_batch(form, ov):
    from bialign_amd.batch import make_batch
    pairs, mu1, mu2 = scored_pairs()
    pairs = list(pairs)
    params = dict(synth.PROTEIN_PARAMS, **ov)
    R, seed = 3, 31
    scores, _, _, _ = run_null(pairs, params, R, seed=seed, **form_kw(form, mu1, mu2))
    virt = [(p, r) for p in range(len(pairs)) for r in range(R)]
    ext = [sg.shuffle_b(pairs[p], seed, p, r) for p, r in virt]
    kw = form_kw(form, [sg.shuffle_tables(mu1[p], seed, p, r) for p, r in virt], [sg.shuffle_tables(mu2[p], seed, p, r) for p, r in virt])
    b = make_batch(ext, params, score_only=True, **kw)
    b.run()
    np.testing.assert_array_equal(b.scores().reshape(len(pairs), R), scores)
    b.close()


# ---- 5. the result does not depend on the plan, and does depend on the seed

def test_independent_of_chunks_and_team(monkeypatch):
    pairs = [synth.protein_pair(8800 + t, 300 - 7 * t, 310 + 5 * t) for t in range(3)]
    params = dict(synth.PROTEIN_PARAMS)
    mu1, _ = random_tables(pairs, 8800)
    R, seed = 3, 8
    base, info, _, finfo = run_null(pairs, params, R, seed=seed, mu1_dense=mu1)
    assert info["nchunks"] == 1 and finfo["build_launches"] == 1
    # One chunk holds all nine virtual pairs: hbm_layer_bytes is the sum of their SCORE_ONLY layers, table_bytes the sum
    # of their permuted tables (4 * n * m each).  A budget of all the layers plus half the tables holds the layers alone
    # but not layers and tables: the tables force the cut.
    layers, tables = info["hbm_layer_bytes"], finfo["table_bytes"]
    assert tables == R * sum(4 * len(a) * len(b) for a, b, _, _ in pairs)
    budget = layers + tables // 2
    assert layers <= budget < layers + tables
    chunked, info_c, _, finfo_c = run_null(pairs, params, R, seed=seed, mu1_dense=mu1, hbm_budget_bytes=budget)
    assert info_c["nchunks"] > 1 and finfo_c["build_launches"] == info_c["nchunks"]
    assert finfo_c["table_bytes"] + info_c["hbm_layer_bytes"] <= budget
    np.testing.assert_array_equal(chunked, base)
    monkeypatch.setenv("BIALIGN_TEAM", "1")
    solo, _, timing_1, _ = run_null(pairs, params, R, seed=seed, mu1_dense=mu1)
    monkeypatch.setenv("BIALIGN_TEAM", "2")
    duo, _, timing_2, _ = run_null(pairs, params, R, seed=seed, mu1_dense=mu1)
    monkeypatch.delenv("BIALIGN_TEAM")
    assert timing_1["waves_per_pair"] == 1 and timing_2["waves_per_pair"] in (1, 2)   # (2 where the pairs' period admits it)
    np.testing.assert_array_equal(solo, base)
    np.testing.assert_array_equal(duo, base)
    other, _, _, _ = run_null(pairs, params, R, seed=seed + 1, mu1_dense=mu1)
    assert not np.array_equal(other, base)


# ---- 6. the reduction, and z-scores end to end

@pytest.mark.parametrize("R", [1, 65])
def test_stats_and_zscores(R):
    from bialign_amd.batch import make_batch
    pairs = [synth.protein_pair(8900, 38, 45)]
    params = dict(synth.PROTEIN_PARAMS)
    pssm = [np.random.default_rng(8900).integers(-400, 1100, size=(38, 45))]   # (int64: the range check passes it on)
    ob = make_batch(pairs, params, score_only=True, mu1_dense=pssm)
    ob.run()
    observed = ob.scores().copy()
    ob.close()
    b = sg.null_dense_batch(pairs, params, R, seed=R, mu1_dense=pssm)
    b.run()
    sc = b.null_scores().astype(np.int64)
    for obs in (observed, None):
        st = b.null_stats(obs)
        np.testing.assert_array_equal(st["sum"], sc.sum(axis=1))
        np.testing.assert_array_equal(st["sumsq"], (sc * sc).sum(axis=1))
        np.testing.assert_array_equal(st["min"], sc.min(axis=1))
        np.testing.assert_array_equal(st["max"], sc.max(axis=1))
        np.testing.assert_array_equal(st["replicas"], [R])
        want = (sc >= observed[:, None].astype(np.int64)).sum(axis=1) if obs is not None else [0]
        np.testing.assert_array_equal(st["n_ge"], want)
    ni = b.null_info()
    assert ni["shuffle_ms"] > 0 and ni["stats_ms"] > 0 and b.feature_info()["build_ms"] > 0
    want_z = sg.zscores_from_stats(observed, b.null_stats(observed))
    b.close()
    for given in (None, observed):
        z = sg.zscores_dense(pairs, params, replicas=R, seed=R, mu1_dense=pssm, observed=given)
        assert sorted(z) == sorted(want_z)
        for k in want_z:
            np.testing.assert_array_equal(z[k], want_z[k])   # (nan == nan here: R = 1 has no deviation)


# ---- 7. refusals through the C ABI; the engine goes on working

def raw_create(pair, params, flags=0, replicas=3, mu1=True, mu2=False, mu1_off=True, fill=7, budget=0, keep_open=False):
    """bialign_batch_create_null_dense through ctypes alone, on one pair."""
    from bialign_amd import _lib
    from bialign_amd.batch import encode_flat
    from bialign_amd.engine import default_engine, _ptr
    model, fb = encode_flat([pair], params)
    n, m = len(pair[0]), len(pair[1])
    keep = dict(fb=fb, s1=np.ascontiguousarray(model.s1, np.int32), s2=np.ascontiguousarray(model.s2, np.int32),
                tab=np.full(n * m, fill, np.int32), off=np.zeros(1, np.int64))
    prm = _lib.Params(params["gap_opening_cost"], params["gap_cost"], params["shift_cost"], params["max_shift"], 0, flags)
    sc = _lib.Scoring(keep["s1"].shape[0], _ptr(keep["s1"], ctypes.c_int32), keep["s2"].shape[0], _ptr(keep["s2"], ctypes.c_int32))
    tab, off = _ptr(keep["tab"], ctypes.c_int32), _ptr(keep["off"], ctypes.c_int64)
    pr = _lib.Pairs(1, _ptr(fb.len_a, ctypes.c_int32), _ptr(fb.len_b, ctypes.c_int32), _ptr(fb.off_a, ctypes.c_int64),
                    _ptr(fb.off_b, ctypes.c_int64), _ptr(fb.seq_a, ctypes.c_uint8), _ptr(fb.cls_a, ctypes.c_uint8),
                    _ptr(fb.seq_b, ctypes.c_uint8), _ptr(fb.cls_b, ctypes.c_uint8), tab if mu2 else None, off if mu2 else None,
                    tab if mu1 else None, off if (mu1 and mu1_off) else None)
    h = ctypes.c_void_p()
    rc = _lib.lib.bialign_batch_create_null_dense(default_engine()._h, ctypes.byref(prm), ctypes.byref(sc), ctypes.byref(pr),
                                                  ctypes.byref(_lib.NullSpec(replicas, 0)), int(budget), ctypes.byref(h))
    msg = _lib.lib.bialign_last_error().decode()
    if h:
        _lib.lib.bialign_batch_destroy(h)
    return rc, msg


def test_refusals():
    from bialign_amd import _lib
    from bialign_amd._lib import BialignError
    pair = synth.protein_pair(8950, 12, 10)
    params = dict(synth.PROTEIN_PARAMS)
    tab = [np.full((12, 10), 7, np.int32)]
    good, _, _, _ = run_null([pair], params, 3, mu1_dense=tab)

    def still_works():
        again, _, _, _ = run_null([pair], params, 3, mu1_dense=tab)
        np.testing.assert_array_equal(again, good)

    assert raw_create(pair, params)[0] == 0
    assert raw_create(pair, params, flags=_lib.BATCH_SCORE_ONLY, mu2=True)[0] == 0
    rc, msg = raw_create(pair, params, mu1=False, mu2=False)                  # neither table: the LOOKUP entry point's batch
    assert rc == _lib.E_INVALID and "bialign_batch_create_null" in msg, msg
    still_works()
    for flag in (_lib.BATCH_LEAN_TRACE, _lib.BATCH_LEVEL_TRACE):
        rc, msg = raw_create(pair, params, flags=flag)
        assert rc == _lib.E_INVALID and "SCORE_ONLY" in msg, msg
        still_works()
    for bad in (0, 65536):
        rc, msg = raw_create(pair, params, replicas=bad)
        assert rc == _lib.E_INVALID and "replicas" in msg, msg
    rc, msg = raw_create(pair, dict(params, max_shift=7, **LIN))              # the one-layer recurrence beyond the tiled band
    assert rc == _lib.E_UNSUPPORTED, msg
    still_works()
    rc, msg = raw_create(pair, params, fill=-(1 << 27))                       # a table magnitude outside the window
    assert rc == _lib.E_RANGE and "safety window" in msg, msg
    still_works()
    rc, msg = raw_create(pair, params, mu1_off=False)
    assert rc == _lib.E_INVALID and "mu1_off" in msg, msg
    big = synth.protein_pair(8951, 600, 600)                                  # one replica's table alone is 1.44 MB
    rc, msg = raw_create(big, dict(params, **LIN), budget=1 << 20)
    assert rc == _lib.E_NOMEM and "pair 0" in msg and "one replica" in msg, msg
    still_works()
    b = sg.null_dense_batch([pair], params, 3, mu1_dense=tab)
    b.run()
    for call in (b.scores, b.traces, lambda: b.dump_layers(0), lambda: b.dump_mu2(0)):
        with pytest.raises(BialignError) as e:
            call()
        assert e.value.code == _lib.E_INVALID
    out = np.zeros(120, np.int32)
    i32p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert _lib.lib.bialign_batch_dump_null_tables(b._h, 0, 0, i32p, i32p) == _lib.E_INVALID   # mu2 is in LOOKUP form
    assert _lib.lib.bialign_batch_dump_null_tables(b._h, 0, 3, i32p, None) == _lib.E_INVALID   # replica out of range
    assert _lib.lib.bialign_batch_dump_null_tables(b._h, 0, 2, i32p, None) == 0
    np.testing.assert_array_equal(out, 7)
    np.testing.assert_array_equal(b.null_scores(), good)
    b.close()
    lookup = sg.null_batch([pair], params, 3)                                 # a LOOKUP null batch has no tables
    rc = _lib.lib.bialign_batch_dump_null_tables(lookup._h, 0, 0, i32p, None)
    assert rc == _lib.E_INVALID and "DENSE-form null batch" in _lib.lib.bialign_last_error().decode()
    with pytest.raises(ValueError):
        lookup.null_tables(0, 0)
    lookup.close()
    still_works()
