"""FEATURE-form null batches, host side (no GPU): the Python mirror of what a replica of B holds (letters and three
numbers per residue gathered through the header's permutation), the added C-ABI symbols, and argument errors raised
before the library is called."""
import os
import re
import types

import numpy as np
import pytest

from bialign_amd import significance as sg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bialign.h")
PARAMS = dict(type="RNA", simmatrix=None, structure_weight=400, gap_opening_cost=-200, gap_cost=-50, shift_cost=-150,
              max_shift=1, sequence_match_similarity=100, sequence_mismatch_similarity=0)


def molecule(seed, n):
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list("ACGU"), size=n)), tuple(rng.random(n) for _ in range(3))


# ---- the mirror

@pytest.mark.parametrize("m", [1, 2, 3, 17, 64, 65, 130])
def test_shuffle_features_is_indexing_by_the_permutation(m):
    seq, feats = molecule(100 + m, m)
    for seed, p, r in [(0, 0, 0), (77, 3, 6), (0xFFFFFFFF, 2 ** 31 - 2, 65534)]:
        perm = sg.permutation(seed, p, r, m)
        got_seq, got = sg.shuffle_features(seq, feats, seed, p, r)
        assert got_seq == "".join(seq[x] for x in perm)
        for f, g in zip(feats, got):
            assert g.dtype == np.float64
            np.testing.assert_array_equal(g.view(np.uint64), f[perm].view(np.uint64))   # moved, not recomputed
    if m == 1:
        assert sg.shuffle_features(seq, feats, 5, 6, 7)[0] == seq
        for f, g in zip(feats, sg.shuffle_features(seq, feats, 5, 6, 7)[1]):
            np.testing.assert_array_equal(g, f)


def test_letter_and_its_three_numbers_land_at_the_same_index():
    """Every residue is made recognisable: letter x of an alphabet of 40, and the numbers x, x + 0.25, x + 0.5."""
    m = 40
    seq = "".join(chr(ord("0") + x) for x in range(m))
    base = np.arange(m, dtype=np.float64)
    got_seq, (up, down, unp) = sg.shuffle_features(seq, (base, base + 0.25, base + 0.5), 9, 4, 2)
    where = np.array([ord(c) - ord("0") for c in got_seq], dtype=np.float64)
    assert sorted(where.tolist()) == base.tolist() and where.tolist() != base.tolist()
    np.testing.assert_array_equal(up, where)
    np.testing.assert_array_equal(down, where + 0.25)
    np.testing.assert_array_equal(unp, where + 0.5)
    # ... and it is the null model of the LOOKUP RNA null: the same positions move as in shuffle_b
    _, sb, _, _ = sg.shuffle_b(("A", seq, ".", "." * m), 9, 4, 2)
    assert sb == got_seq
    with pytest.raises(ValueError):
        sg.shuffle_features("ACG", (base, base, base), 0, 0, 0)
    with pytest.raises(ValueError):
        sg.shuffle_features("ACG", (base[:3], base[:3]), 0, 0, 0)


# ---- the C ABI: added symbols, ABI still 10

def test_header_and_binding_declare_the_new_symbols():
    from bialign_amd import _lib
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(bialign_[a-z_]+)\s*\(", text))
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("bialign_batch_create_null_features", "bialign_batch_dump_null_features"):
        assert name in declared and name in bound
        assert hasattr(_lib.lib, name)
    assert "#define BIALIGN_ABI_VERSION 10" in text and _lib.ABI_VERSION == 10
    assert _lib.lib.bialign_abi_version() == 10


# ---- engine.Batch: what it refuses itself, before the library

def test_batch_refuses_dense_tables_and_trace_modes_before_the_library(monkeypatch):
    from bialign_amd import _lib, engine

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib.lib, "bialign_batch_create_null", boom, raising=False)
    monkeypatch.setattr(_lib.lib, "bialign_batch_create_null_features", boom, raising=False)
    mol = [(np.zeros(3, np.uint8), np.zeros(3, np.uint8))]
    s = np.zeros((1, 1), np.int32)
    f = [tuple(np.full(3, 0.25) for _ in range(3))]
    feats = (400, f, f)
    for kw in (dict(mu2_dense=[np.zeros((3, 3), np.int32)]), dict(mu1_dense=[np.zeros((3, 3), np.int32)]),
               dict(lean_trace=True), dict(level_trace=True)):
        with pytest.raises(ValueError):
            engine.Batch(None, mol, mol, s, s, -1, -1, -1, 1, null=(3, 0), mu2_features=feats, **kw)
    for bad in ((0, 0), (65536, 0), (3, -1), (3, 2 ** 32), (2.5, 0), 7):
        with pytest.raises((ValueError, TypeError)):
            engine.Batch(None, mol, mol, s, s, -1, -1, -1, 1, null=bad, mu2_features=feats)
    # the combination itself is valid now: it gets as far as the (patched) entry point -- the FEATURE one
    eng = types.SimpleNamespace(_h=None, _batches=set())
    with pytest.raises(AssertionError, match="the library was reached"):
        engine.Batch(eng, mol, mol, s, s, -1, -1, -1, 1, null=(3, 0), mu2_features=feats)
    monkeypatch.setattr(_lib.lib, "bialign_batch_create_null_features", lambda *a, **k: _lib.E_INVALID, raising=False)
    with pytest.raises(_lib.BialignError):   # (the LOOKUP entry point, still patched to fail on call, is not the one taken)
        engine.Batch(eng, mol, mol, s, s, -1, -1, -1, 1, null=(3, 0), mu2_features=feats)


# ---- null_feature_batch / zscores_features: argument errors before the library is loaded or called

MOLS = [molecule(1, 5), molecule(2, 4), molecule(3, 6)]
INDEX = [(0, 1), (2, 1)]


@pytest.mark.parametrize("fn", [sg.null_feature_batch, sg.zscores_features])
def test_argument_errors_before_any_library_call(fn, monkeypatch):
    import bialign_amd.batch as batch
    import bialign_amd.engine as engine

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(engine, "Batch", boom)
    monkeypatch.setattr(engine, "default_engine", boom)
    monkeypatch.setattr(batch, "make_feature_batch", boom)
    for bad in (0, -1, 65536, 2.5, "7"):
        with pytest.raises((ValueError, TypeError)):
            fn(MOLS, INDEX, PARAMS, replicas=bad)
    for bad_seed in (-1, 2 ** 32, 0.5):
        with pytest.raises(ValueError):
            fn(MOLS, INDEX, PARAMS, replicas=3, seed=bad_seed)
    for bad_index in ([], [(0, 3)], [(-1, 0)], [(0, 1), (3, 3)]):
        with pytest.raises(ValueError):
            fn(MOLS, bad_index, PARAMS, replicas=3)
    with pytest.raises(ValueError):
        fn([], INDEX, PARAMS, replicas=3)
    with pytest.raises(ValueError):
        fn(MOLS, [(0, 1)] * 40000, PARAMS, replicas=65535)   # npairs * replicas above INT32_MAX
    seq, (up, down, unp) = MOLS[0]
    ragged = (seq, (up, down[:-1], unp))
    short = (seq, (up[:-1], down[:-1], unp[:-1]))
    two = (seq, (up, down))
    nan, inf, neg = up.copy(), up.copy(), up.copy()
    nan[2], inf[0], neg[4] = float("nan"), float("inf"), -0.125
    for bad_mol in (ragged, short, two, (seq, (nan, down, unp)), (seq, (up, inf, unp)), (seq, (up, down, neg))):
        with pytest.raises(ValueError):
            fn([bad_mol] + MOLS[1:], INDEX, PARAMS, replicas=3)
    with pytest.raises(ValueError, match="math domain error"):
        fn([(seq, (up, down, neg))] + MOLS[1:], INDEX, PARAMS, replicas=3)
    for bad_obs in ([1], [1, 2, 3], [[1, 2]]):
        with pytest.raises(ValueError):
            sg.zscores_features(MOLS, INDEX, PARAMS, replicas=3, observed=bad_obs)
    # good arguments get through to the batch maker
    with pytest.raises(AssertionError, match="the library was reached"):
        fn(MOLS, INDEX, PARAMS, replicas=3, **({"observed": [1, 2]} if fn is sg.zscores_features else {}))


def test_make_feature_batch_checks_null_before_the_library(monkeypatch):
    import bialign_amd.batch as batch
    import bialign_amd.engine as engine

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(engine, "Batch", boom)
    monkeypatch.setattr(engine, "default_engine", boom)
    for kw in (dict(null=(0, 0)), dict(null=(3, -1)), dict(null=(3, 0), lean_trace=True), dict(null=(3, 0), level_trace=True),
               dict(null=(3, 0), mu1_dense=[np.zeros((5, 4), np.int32)] * 2)):
        with pytest.raises(ValueError):
            batch.make_feature_batch(MOLS, INDEX, PARAMS, **kw)
    with pytest.raises(AssertionError, match="the library was reached"):   # the default (null=None) is unchanged
        batch.make_feature_batch(MOLS, INDEX, PARAMS)
