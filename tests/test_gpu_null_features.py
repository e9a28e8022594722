"""FEATURE-form null batches (bialign_batch_create_null_features): RNA molecules with real-valued structure features
against shuffles of B made on the GPU -- sequence codes and three planes of doubles, a residue's numbers moving with
its letter -- whose mu2 tables the GPU builds per chunk.  The shuffles against the Python mirror bit for bit, the scores
against the CPU oracle on the unshuffled tables with permuted B columns and against a host-expanded FEATURE batch, the
reduction against numpy; all comparisons exact."""
import ctypes
import functools

import numpy as np
import pytest

from bialign_amd import significance as sg
from bialign_amd import synth

pytestmark = pytest.mark.gpu

LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
SHAPES = [(3, 55), (55, 3), (17, 31), (40, 22), (28, 28)]   # 5 ragged pairs, lengths 3..55
KEYS = ("up", "down", "unp")
SW = synth.RNA_PARAMS["structure_weight"]


def molecule(seed, n, grid=False):
    """(sequence, (up, down, unp)): random ACGU, non-negative random numbers.  grid: every number is q / sw for an
    integer q, so that sw * sqrt(p * p') sits on an integer wherever two such numbers meet themselves."""
    rng = np.random.default_rng(seed)
    seq = "".join(rng.choice(list("ACGU"), size=n))
    if grid:
        return seq, tuple(rng.integers(0, SW + 1, size=n).astype(np.float64) / SW for _ in range(3))
    feats = [rng.random(n) for _ in range(3)]
    feats[0][rng.integers(0, 4, size=n) == 0] = 0.0   # some exact zeros
    return seq, tuple(feats)


@functools.lru_cache(maxsize=None)
def shape_molecules(seed):
    """The five pairs of SHAPES as molecules 2t, 2t + 1.  The last pair (28 x 28) sits on the integer grid, and its B
    carries A's numbers (rolled by five residues): every row of its table meets its own q in some column, where
    sw * sqrt(q / sw * q / sw) is the integer q or a hair beside it -- a rounding slip would change the entry."""
    mols = []
    for t, (n, m) in enumerate(SHAPES):
        grid = t == len(SHAPES) - 1
        mols += [molecule(seed + 2 * t, n, grid), molecule(seed + 2 * t + 1, m, grid)]
    seq_b, _ = mols[-1]
    mols[-1] = (seq_b, tuple(np.roll(f, 5) for f in mols[-2][1]))
    return tuple(mols), tuple((2 * t, 2 * t + 1) for t in range(len(SHAPES)))


def model_and_codes(mols, params):
    from bialign_amd.scoring import ScoreModel
    model = ScoreModel(params, sequences=[s for s, _ in mols], structures=["."])
    return model, [model.encode_sequence(s) for s, _ in mols]


def codes_of(mols, params):
    return model_and_codes(mols, params)[1]


def run_null(mols, index, params, R, seed=0, **kw):
    b = sg.null_feature_batch(list(mols), list(index), params, R, seed=seed, **kw)
    b.run()
    out = b.null_scores().copy(), dict(b.current_info()), b.timing(), b.feature_info()
    b.close()
    return out


def host_expanded(mols, index, params, R, seed):
    """The same virtual pairs as an ordinary FEATURE batch over molecules extended by the mirror's shuffles."""
    ext, idx = list(mols), []
    for p, (ia, ib) in enumerate(index):
        for r in range(R):
            ext.append(sg.shuffle_features(mols[ib][0], mols[ib][1], seed, p, r))
            idx.append((ia, len(ext) - 1))
    return ext, idx


# ---- 1. the shuffle against the mirror

@pytest.mark.parametrize("R", [1, 7])
def test_shuffle_equals_mirror(R):
    lens_b = [1, 2, 3, 17, 64, 65, 130]   # less than a wave, exactly one, one more, two and a bit
    mols = []
    for t, m in enumerate(lens_b):
        mols += [molecule(8000 + 2 * t, 9 + t), molecule(8001 + 2 * t, m, grid=(t == 3))]
    index = [(2 * t, 2 * t + 1) for t in range(len(lens_b))]
    params = dict(synth.RNA_PARAMS)
    codes = codes_of(mols, params)
    seed = 77
    b = sg.null_feature_batch(mols, index, params, R, seed=seed)
    assert b.info["npairs"] == len(index)
    # codes of both kinds (1 byte each) and three planes of doubles per replica residue
    assert b.null_info()["replica_bytes"] == (2 + 24) * R * sum(lens_b)
    assert b.feature_info()["form"] == "feature"
    for when in ("before run", "after run"):
        for p, (_, ib) in enumerate(index):
            for r in sorted({0, R - 1}):
                perm = sg.permutation(seed, p, r, lens_b[p])
                seq, cls = b.dump_null_codes(p, r)
                np.testing.assert_array_equal(seq, codes[ib][perm], err_msg=f"{when} p={p} r={r}")
                assert not cls.any()
                want_seq, want = sg.shuffle_features(mols[ib][0], mols[ib][1], seed, p, r)
                assert want_seq == "".join(mols[ib][0][x] for x in perm)
                for g, w in zip(b.dump_null_features(p, r), want):
                    assert g.dtype == np.float64
                    np.testing.assert_array_equal(g.view(np.uint64), w.view(np.uint64), err_msg=f"{when} p={p} r={r}")
        b.run()
    b.close()


# ---- 2. pairs that share one B

def test_pairs_sharing_one_b_get_different_shuffles():
    mols = [molecule(8100 + t, 20 + t) for t in range(3)] + [molecule(8103, 40)]
    index = [(0, 3), (1, 3), (2, 3)]
    params = dict(synth.RNA_PARAMS)
    codes = codes_of(mols, params)[3]
    b = sg.null_feature_batch(mols, index, params, 2, seed=5)
    assert b.null_info()["replica_bytes"] == 26 * 2 * 3 * 40   # replicas are per pair, whoever owns the molecule
    got = [[(b.dump_null_codes(p, r)[0], b.dump_null_features(p, r)) for r in range(2)] for p in range(3)]
    b.close()
    for p in range(3):
        for r in range(2):
            perm = sg.permutation(5, p, r, 40)
            np.testing.assert_array_equal(got[p][r][0], codes[perm])
            for g, f in zip(got[p][r][1], mols[3][1]):
                np.testing.assert_array_equal(g.view(np.uint64), f[perm].view(np.uint64))
    assert len({got[p][r][0].tobytes() for p in range(3) for r in range(2)}) == 6
    assert len({got[p][r][1][0].tobytes() for p in range(3) for r in range(2)}) == 6


# ---- 3. scores against the oracle: the real pair's tables with their B columns permuted

@functools.lru_cache(maxsize=None)
def oracle_tables(seed, sw):
    """Per pair of shape_molecules(seed): (n, m, mu2 padded with row and column 0) -- mu2 does not depend on the gap
    parameters, so every case of the same molecules shares it."""
    from bialign_amd.scoring import dense_mu2_from_features
    mols, index = shape_molecules(seed)
    one_based = lambda f: {k: np.concatenate([[0.0], v]) for k, v in zip(KEYS, f)}  # noqa: E731
    out = []
    for ia, ib in index:
        n, m = len(mols[ia][0]), len(mols[ib][0])
        mu2 = np.zeros((n + 1, m + 1), dtype=np.int32)
        mu2[1:, 1:] = dense_mu2_from_features(one_based(mols[ia][1]), one_based(mols[ib][1]), sw)
        out.append((n, m, mu2))
    return out


def check_scores_vs_oracle(mol_seed, params, R, seed):
    from oracle import oracle
    mols, index = shape_molecules(mol_seed)
    scores, info, _, finfo = run_null(mols, index, params, R, seed=seed)
    assert scores.shape == (len(index), R) and info["npairs"] == len(index)
    assert info["cells"] == R * sum(synth.cells_per_pair(n, m, params["max_shift"]) for n, m in SHAPES)
    assert finfo["form"] == "feature" and finfo["build_launches"] == info["nchunks"]
    for p, ((ia, ib), (n, m, mu2)) in enumerate(zip(index, oracle_tables(mol_seed, params["structure_weight"]))):
        mu1, _ = oracle.mu_tables(mols[ia][0], mols[ib][0], "." * n, "." * m, params)
        for r in range(R):
            cols = np.concatenate([[0], 1 + sg.permutation(seed, p, r, m)])
            want = oracle.solve_tables(n, m, params, mu1[:, cols], mu2[:, cols], want_trace=False)["score"]
            assert int(scores[p, r]) == want, (p, r)


@pytest.mark.parametrize("s", [0, 1, 2, 5])
@pytest.mark.parametrize("ov", [{}, LIN], ids=["affine", "linear"])
def test_scores_equal_oracle(s, ov):
    check_scores_vs_oracle(8200, dict(synth.RNA_PARAMS, max_shift=s, **ov), 4, 11 + s)


def test_scores_equal_oracle_wide_band():
    check_scores_vs_oracle(8200, dict(synth.RNA_PARAMS, max_shift=7), 4, 9)


def test_wide_band_rings_are_cut_into_chunks():
    """The batch of test_scores_equal_oracle_wide_band under a budget of two rings (and 1 MiB: the per-chunk mu2 tables are a
    few KB): several chunks, each with a builder launch of its own; the same null scores, reductions and z-scores."""
    from oracle import oracle
    from wide_ring import check_chunked_null
    mols, index = shape_molecules(8200)
    params, R, seed = dict(synth.RNA_PARAMS, max_shift=7), 4, 9
    want = []
    for p, ((ia, ib), (n, m, mu2)) in enumerate(zip(index, oracle_tables(8200, params["structure_weight"]))):
        mu1, _ = oracle.mu_tables(mols[ia][0], mols[ib][0], "." * n, "." * m, params)
        cols = [np.concatenate([[0], 1 + sg.permutation(seed, p, r, m)]) for r in range(R)]
        want.append([oracle.solve_tables(n, m, params, mu1[:, c], mu2[:, c], want_trace=False)["score"] for c in cols])
    observed = np.array([sorted(row)[R // 2] for row in want], dtype=np.int32)
    check_chunked_null(lambda bud: sg.null_feature_batch(list(mols), list(index), params, R, seed=seed, hbm_budget_bytes=bud),
                       lambda bud: sg.zscores_features(list(mols), list(index), params, replicas=R, seed=seed, hbm_budget_bytes=bud),
                       [n for n, _ in SHAPES], 7, want, observed)


def test_scores_equal_oracle_general_beta():
    check_scores_vs_oracle(8200, dict(synth.RNA_PARAMS, gap_opening_cost=100), 4, 3)


# ---- 4. equals the host-expanded batch

@pytest.mark.parametrize("ov", [{}, dict(max_shift=2, **LIN)], ids=["affine_s1", "linear_s2"])
def test_equals_host_expanded_feature_batch(ov):
    from bialign_amd.batch import make_feature_batch
    mols, index = shape_molecules(8200)
    params = dict(synth.RNA_PARAMS, **ov)
    R, seed = 4, 31
    scores, _, _, _ = run_null(mols, index, params, R, seed=seed)
    ext, idx = host_expanded(mols, index, params, R, seed)
    b = make_feature_batch(ext, idx, params, score_only=True)
    b.run()
    np.testing.assert_array_equal(b.scores().reshape(len(index), R), scores)
    b.close()


# ---- 5. the result does not depend on the plan

def test_independent_of_chunks_and_team(monkeypatch):
    mols, index = [], []
    for t in range(3):
        mols += [molecule(8300 + 2 * t, 300 - 7 * t), molecule(8301 + 2 * t, 310 + 5 * t)]
        index.append((2 * t, 2 * t + 1))
    params = dict(synth.RNA_PARAMS)
    R, seed = 3, 8
    base, info, _, finfo = run_null(mols, index, params, R, seed=seed)
    assert info["nchunks"] == 1 and finfo["build_launches"] == 1
    # One chunk holds all nine virtual pairs: hbm_layer_bytes is the sum of their SCORE_ONLY layers (about 1.6 MB each:
    # 84 dwords per sweep step of the affine s=1 kernel, some 4 900 steps), table_bytes the sum of their tables
    # (4 * n * m, about 0.37 MB each).  A budget of all the layers plus half the tables holds the layers alone but not
    # layers and tables: the tables force the cut.
    layers, tables = info["hbm_layer_bytes"], finfo["table_bytes"]
    assert tables == R * sum(4 * len(mols[a][0]) * len(mols[b][0]) for a, b in index)
    budget = layers + tables // 2
    assert layers <= budget < layers + tables
    chunked, info_c, _, finfo_c = run_null(mols, index, params, R, seed=seed, hbm_budget_bytes=budget)
    assert info_c["nchunks"] > 1 and finfo_c["build_launches"] == info_c["nchunks"]
    assert finfo_c["table_bytes"] + info_c["hbm_layer_bytes"] <= budget
    np.testing.assert_array_equal(chunked, base)
    monkeypatch.setenv("BIALIGN_TEAM", "1")
    solo, _, timing_1, _ = run_null(mols, index, params, R, seed=seed)
    monkeypatch.delenv("BIALIGN_TEAM")
    assert timing_1["waves_per_pair"] == 1
    np.testing.assert_array_equal(solo, base)
    other, _, _, _ = run_null(mols, index, params, R, seed=seed + 1)
    assert not np.array_equal(other, base)


# ---- 6. the reduction, and z-scores end to end

@pytest.mark.parametrize("R", [1, 65])
def test_stats_and_zscores(R):
    from bialign_amd.batch import make_feature_batch
    mols, index = shape_molecules(8200)
    params = dict(synth.RNA_PARAMS)
    ob = make_feature_batch(list(mols), list(index), params, score_only=True)
    ob.run()
    observed = ob.scores().copy()
    ob.close()
    b = sg.null_feature_batch(list(mols), list(index), params, R, seed=R)
    b.run()
    sc = b.null_scores().astype(np.int64)
    for obs in (observed, None):
        st = b.null_stats(obs)
        np.testing.assert_array_equal(st["sum"], sc.sum(axis=1))
        np.testing.assert_array_equal(st["sumsq"], (sc * sc).sum(axis=1))
        np.testing.assert_array_equal(st["min"], sc.min(axis=1))
        np.testing.assert_array_equal(st["max"], sc.max(axis=1))
        np.testing.assert_array_equal(st["replicas"], [R] * len(index))
        want = (sc >= observed[:, None].astype(np.int64)).sum(axis=1) if obs is not None else [0] * len(index)
        np.testing.assert_array_equal(st["n_ge"], want)
    ni = b.null_info()
    assert ni["shuffle_ms"] > 0 and ni["stats_ms"] > 0 and b.feature_info()["build_ms"] > 0
    want_z = sg.zscores_from_stats(observed, b.null_stats(observed))
    b.close()
    for given in (None, observed):
        z = sg.zscores_features(list(mols), list(index), params, replicas=R, seed=R, observed=given)
        assert sorted(z) == sorted(want_z)
        for k in want_z:
            np.testing.assert_array_equal(z[k], want_z[k])   # (nan == nan here: R = 1 has no deviation)


# ---- 7. refusals through the C ABI; the engine goes on working

def raw_create(mols, flags=0, replicas=3, dense1=False, feat_edit=None, params=None, budget=0, sw=SW):
    """bialign_batch_create_null_features through ctypes alone, on one pair (molecule 0 against molecule 1)."""
    from bialign_amd import _lib
    from bialign_amd.engine import default_engine, _ptr
    params = params or dict(synth.RNA_PARAMS)
    n, m = len(mols[0][0]), len(mols[1][0])
    model, codes = model_and_codes(mols, params)
    keep = dict(len_a=np.array([n], np.int32), len_b=np.array([m], np.int32), off=np.zeros(1, np.int64),
                seq_a=np.ascontiguousarray(codes[0], np.uint8), seq_b=np.ascontiguousarray(codes[1], np.uint8),
                s1=np.ascontiguousarray(model.s1, np.int32), s2=np.ascontiguousarray(model.s2, np.int32),
                tab=np.zeros(n * m, np.int32))
    assert max(keep["seq_a"].max(), keep["seq_b"].max()) < keep["s1"].shape[0]
    fa = [np.ascontiguousarray(f, np.float64).copy() for f in mols[0][1]]
    fb = [np.ascontiguousarray(f, np.float64).copy() for f in mols[1][1]]
    if feat_edit:
        feat_edit(fa, fb)
    prm = _lib.Params(params["gap_opening_cost"], params["gap_cost"], params["shift_cost"], params["max_shift"], 0, flags)
    sc = _lib.Scoring(keep["s1"].shape[0], _ptr(keep["s1"], ctypes.c_int32), keep["s2"].shape[0], _ptr(keep["s2"], ctypes.c_int32))
    pr = _lib.Pairs(1, _ptr(keep["len_a"], ctypes.c_int32), _ptr(keep["len_b"], ctypes.c_int32),
                    _ptr(keep["off"], ctypes.c_int64), _ptr(keep["off"], ctypes.c_int64),
                    _ptr(keep["seq_a"], ctypes.c_uint8), None, _ptr(keep["seq_b"], ctypes.c_uint8), None, None, None,
                    _ptr(keep["tab"], ctypes.c_int32) if dense1 else None, _ptr(keep["off"], ctypes.c_int64) if dense1 else None)
    ft = _lib.Features(sw, *(_ptr(x, ctypes.c_double) for x in fa + fb))
    h = ctypes.c_void_p()
    rc = _lib.lib.bialign_batch_create_null_features(default_engine()._h, ctypes.byref(prm), ctypes.byref(sc), ctypes.byref(pr),
                                                     ctypes.byref(ft), ctypes.byref(_lib.NullSpec(replicas, 0)), int(budget),
                                                     ctypes.byref(h))
    msg = _lib.lib.bialign_last_error().decode()
    if h:
        _lib.lib.bialign_batch_destroy(h)
    return rc, msg


def test_refusals():
    from bialign_amd import _lib
    from bialign_amd._lib import BialignError
    mols = [molecule(8400, 12), molecule(8401, 10)]
    params = dict(synth.RNA_PARAMS)
    good, _, _, _ = run_null(mols, [(0, 1)], params, 3)

    def still_works():
        again, _, _, _ = run_null(mols, [(0, 1)], params, 3)
        np.testing.assert_array_equal(again, good)

    assert raw_create(mols)[0] == 0                                   # cls_a / cls_b / mu2_dense NULL: fine
    assert raw_create(mols, flags=_lib.BATCH_SCORE_ONLY)[0] == 0
    rc, msg = raw_create(mols, dense1=True)
    assert rc == _lib.E_UNSUPPORTED and "LOOKUP" in msg, msg
    still_works()
    for bad in (-0.125, float("nan")):
        def edit(fa, fb, bad=bad):
            fb[1][4] = bad
        rc, msg = raw_create(mols, feat_edit=edit)
        assert rc == _lib.E_INVALID and "pair 0" in msg and "position 5" in msg and "down_b" in msg, msg
        still_works()
    for flag in (_lib.BATCH_LEAN_TRACE, _lib.BATCH_LEVEL_TRACE):
        rc, msg = raw_create(mols, flags=flag)
        assert rc == _lib.E_INVALID and "SCORE_ONLY" in msg, msg
        still_works()
    for bad in (0, 65536):
        rc, msg = raw_create(mols, replicas=bad)
        assert rc == _lib.E_INVALID and "replicas" in msg, msg
    rc, msg = raw_create(mols, params=dict(params, max_shift=6, **LIN))   # the one-layer recurrence beyond the tiled band
    assert rc == _lib.E_UNSUPPORTED, msg
    still_works()
    rc, msg = raw_create(mols, sw=1 << 27)
    assert rc == _lib.E_RANGE and "safety window" in msg, msg
    big = [molecule(8402, 600), molecule(8403, 600)]                      # one replica's table alone is 1.44 MB
    rc, msg = raw_create(big, params=dict(params, **LIN), budget=1 << 20)
    assert rc == _lib.E_NOMEM and "pair 0" in msg and "one replica" in msg, msg
    still_works()
    b = sg.null_feature_batch(mols, [(0, 1)], params, 3)
    b.run()
    for call in (b.scores, b.traces, lambda: b.dump_layers(0), lambda: b.dump_mu2(0)):
        with pytest.raises(BialignError) as e:
            call()
        assert e.value.code == _lib.E_INVALID
    np.testing.assert_array_equal(b.null_scores(), good)
    b.close()
    from bialign_amd.batch import make_batch
    lookup = sg.null_batch([synth.rna_pair(7, 12, 10)], params, 3)        # a LOOKUP null batch has no feature planes
    with pytest.raises(BialignError) as e:
        lookup.dump_null_features(0, 0)
    assert e.value.code == _lib.E_INVALID
    lookup.close()
    plain = make_batch([synth.rna_pair(7, 12, 10)], params)
    out = np.zeros(10)
    rc = _lib.lib.bialign_batch_dump_null_features(plain._h, 0, 0, *(out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),) * 3)
    assert rc == _lib.E_INVALID
    plain.close()
    still_works()
