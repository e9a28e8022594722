"""DENSE-form null batches, host side (no GPU): the Python mirror of a replica's tables (columns gathered through the
header's permutation), the added C-ABI symbols and their signatures as a C compiler reads the header, and argument errors
raised before the library is called."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from bialign_amd import significance as sg
from bialign_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bialign.h")
PARAMS = dict(synth.PROTEIN_PARAMS)
PAIRS = [("ACDEF", "ACDE", "HHHCC", "HHCC"), ("ACD", "ACDEFG", "HCC", "HHHCCE")]   # (5, 4) and (3, 6)


def table(n, m, sign=1):
    """Distinct values: a wrong row or column shows."""
    return sign * (np.arange(n, dtype=np.int32)[:, None] * 1000 + np.arange(m, dtype=np.int32)[None, :])


def tables(sign=1):
    return [table(len(a), len(b), sign) for a, b, _, _ in PAIRS]


# ---- the mirror

@pytest.mark.parametrize("m", [1, 2, 3, 17, 64, 65, 130])
def test_shuffle_tables_is_indexing_columns_by_the_permutation(m):
    tab = table(7, m)
    for seed, p, r in [(0, 0, 0), (77, 3, 6), (0xFFFFFFFF, 2 ** 31 - 2, 65534)]:
        perm = sg.permutation(seed, p, r, m)
        got = sg.shuffle_tables(tab, seed, p, r)
        assert got.dtype == tab.dtype and got.shape == tab.shape and got.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(got, tab[:, perm])
        np.testing.assert_array_equal(got // 1000, tab // 1000)          # rows stay
        np.testing.assert_array_equal(got[0] % 1000, perm)               # columns move as perm says
    if m == 1:
        np.testing.assert_array_equal(sg.shuffle_tables(tab, 5, 6, 7), tab)
    with pytest.raises(ValueError):
        sg.shuffle_tables(np.arange(m), 0, 0, 0)


def test_same_permutation_as_the_lookup_and_feature_nulls():
    """Equal (seed, pair, replica, m): column x of the replica's table is the column of the residue that shuffle_b and
    shuffle_features put at x."""
    m = 40
    letters = "".join(chr(ord("0") + x) for x in range(m))
    base = np.arange(m, dtype=np.float64)
    for seed, p, r in [(9, 4, 2), (0, 0, 0), (123456, 77, 19)]:
        got = sg.shuffle_tables(table(3, m), seed, p, r)
        _, sb, _, tb = sg.shuffle_b(("A", letters, ".", letters), seed, p, r)
        where = [ord(c) - ord("0") for c in sb]
        assert sb == tb and sorted(where) == list(range(m))
        np.testing.assert_array_equal(got[0], where)
        fs, (up, _, _) = sg.shuffle_features(letters, (base, base, base), seed, p, r)
        assert fs == sb
        np.testing.assert_array_equal(got[2] - 2000, up)


# ---- the C ABI: added symbols, ABI still 10, signatures as a C compiler reads the header

def test_header_and_binding_declare_the_new_symbols():
    from bialign_amd import _lib
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(bialign_[a-z_]+)\s*\(", text))
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("bialign_batch_create_null_dense", "bialign_batch_dump_null_tables"):
        assert name in declared and name in bound
        assert hasattr(_lib.lib, name)
    assert "#define BIALIGN_ABI_VERSION 10" in text and _lib.ABI_VERSION == 10
    assert _lib.lib.bialign_abi_version() == 10


def test_signatures_equal_the_headers(tmp_path):
    """The header's declarations must be assignable to function pointers of the types the binding assumes."""
    src = tmp_path / "sig.c"
    src.write_text(f'''#include "{HEADER}"
int (*create_null_dense)(bialign_engine*, const bialign_params*, const bialign_scoring*, const bialign_pairs*,
                         const bialign_null_spec*, int64_t, bialign_batch**) = bialign_batch_create_null_dense;
int (*dump_null_tables)(bialign_batch*, int32_t, int32_t, int32_t*, int32_t*) = bialign_batch_dump_null_tables;
int (*create_null)(bialign_engine*, const bialign_params*, const bialign_scoring*, const bialign_pairs*,
                   const bialign_null_spec*, int64_t, bialign_batch**) = bialign_batch_create_null;
''')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic-errors", "-c", "-o", str(tmp_path / "sig.o"), str(src)],
                   check=True)
    from bialign_amd import _lib
    by_name = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    # the binding: the same argument list as the LOOKUP entry point; the hook takes two int32 out pointers
    assert by_name["bialign_batch_create_null_dense"] == by_name["bialign_batch_create_null"]
    res, args = by_name["bialign_batch_dump_null_tables"]
    assert res is _lib.ctypes.c_int
    assert args == [_lib.ctypes.c_void_p, _lib.ctypes.c_int32, _lib.ctypes.c_int32, _lib.c_i32p, _lib.c_i32p]


# ---- engine.Batch: what it refuses itself, before the library

def boom(*a, **k):
    raise AssertionError("the library was reached")


def patch_creates(monkeypatch):
    from bialign_amd import _lib
    for name in ("bialign_batch_create", "bialign_batch_create_null", "bialign_batch_create_null_features",
                 "bialign_batch_create_features", "bialign_batch_create_null_dense"):
        monkeypatch.setattr(_lib.lib, name, boom, raising=False)


def test_batch_refuses_bad_arguments_before_the_library(monkeypatch):
    from bialign_amd import _lib, engine
    patch_creates(monkeypatch)
    mol = [(np.zeros(3, np.uint8), np.zeros(3, np.uint8))]
    s = np.zeros((1, 1), np.int32)
    good = [np.zeros((3, 3), np.int32)]
    f = [tuple(np.full(3, 0.25) for _ in range(3))]

    def make(eng=None, **kw):
        return engine.Batch(eng, mol, mol, s, s, -1, -1, -1, 1, **kw)
    with pytest.raises(ValueError, match="mu1_dense and / or mu2_dense"):
        make(null_dense=(3, 0))                                              # no dense table
    for kw in (dict(null=(3, 0)), dict(mu2_features=(400, f, f)), dict(lean_trace=True), dict(level_trace=True)):
        with pytest.raises(ValueError):
            make(null_dense=(3, 0), mu1_dense=good, **kw)
    for bad in ((0, 0), (65536, 0), (3, -1), (3, 2 ** 32), (2.5, 0), 7):
        with pytest.raises((ValueError, TypeError)):
            make(null_dense=bad, mu1_dense=good)
    for name in ("mu1_dense", "mu2_dense"):
        for bad_tab in ([np.zeros((3, 4), np.int32)], [np.zeros((3, 3), np.float64)], [[[1, 2, 3], [1, 2], [1, 2, 3]]],
                        good * 2, [np.full((3, 3), 2 ** 31, np.int64)]):
            with pytest.raises(ValueError):
                make(null_dense=(3, 0), **{name: bad_tab})
    # null= together with dense tables keeps raising
    with pytest.raises(ValueError):
        make(null=(3, 0), mu1_dense=good)
    # good arguments reach the new entry point, and not the LOOKUP one
    eng = types.SimpleNamespace(_h=None, _batches=set())
    for kw in (dict(mu1_dense=good), dict(mu2_dense=good), dict(mu1_dense=good, mu2_dense=good)):
        with pytest.raises(AssertionError, match="the library was reached"):
            make(eng, null_dense=(3, 0), **kw)
    monkeypatch.setattr(_lib.lib, "bialign_batch_create_null_dense", lambda *a, **k: _lib.E_INVALID, raising=False)
    with pytest.raises(_lib.BialignError):   # (bialign_batch_create_null, still patched to fail on call, is not the one taken)
        make(eng, null_dense=(3, 0), mu1_dense=good)


# ---- make_batch / null_dense_batch / zscores_dense: argument errors before the library is loaded or called

def callers():
    from bialign_amd import batch

    def via_make_batch(pairs, params, replicas=3, seed=0, **kw):
        return batch.make_batch(pairs, params, score_only=True, null_dense=(replicas, seed), **kw)
    return [via_make_batch, sg.null_dense_batch, sg.zscores_dense]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["make_batch", "null_dense_batch", "zscores_dense"])
def test_argument_errors_before_any_library_call(which, monkeypatch):
    import bialign_amd.engine as engine
    fn = callers()[which]
    monkeypatch.setattr(engine, "Batch", boom)
    monkeypatch.setattr(engine, "default_engine", boom)
    with pytest.raises(ValueError, match="mu1_dense and / or mu2_dense"):
        fn(PAIRS, PARAMS, replicas=3)                                        # no dense table
    for bad in (0, -1, 65536, 2.5, "7"):
        with pytest.raises((ValueError, TypeError)):
            fn(PAIRS, PARAMS, replicas=bad, mu1_dense=tables())
    for bad_seed in (-1, 2 ** 32, 0.5):
        with pytest.raises(ValueError):
            fn(PAIRS, PARAMS, replicas=3, seed=bad_seed, mu1_dense=tables())
    with pytest.raises(ValueError):
        fn([], PARAMS, replicas=3, mu1_dense=[])
    with pytest.raises(ValueError):
        fn(PAIRS[:1] * 40000, PARAMS, replicas=65535, mu1_dense=tables()[:1] * 40000)   # npairs * replicas above INT32_MAX
    t = tables()
    wrong_shape = [t[0], t[1].T]
    floats = [t[0], t[1].astype(np.float64)]
    ragged = [t[0], [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6]]]
    beyond = [t[0], t[1].astype(np.int64) + 2 ** 31]
    for name in ("mu1_dense", "mu2_dense"):
        for bad_tabs in (wrong_shape, floats, ragged, beyond, t[:1], t + t[:1]):
            with pytest.raises(ValueError):
                fn(PAIRS, PARAMS, replicas=3, **{name: bad_tabs})
        with pytest.raises(ValueError):                                      # one good form does not excuse the other
            fn(PAIRS, PARAMS, replicas=3, **{name: t, ("mu2_dense" if name == "mu1_dense" else "mu1_dense"): floats})
    if which == 0:
        from bialign_amd import batch
        for kw in (dict(lean_trace=True), dict(level_trace=True)):
            with pytest.raises(ValueError):
                batch.make_batch(PAIRS, PARAMS, null_dense=(3, 0), mu1_dense=t, **kw)
    if which == 2:
        for bad_obs in ([1], [1, 2, 3], [[1, 2]]):
            with pytest.raises(ValueError):
                sg.zscores_dense(PAIRS, PARAMS, replicas=3, mu1_dense=t, observed=bad_obs)
    # good arguments get through to the batch maker
    for kw in (dict(mu1_dense=t), dict(mu2_dense=tables(-1)), dict(mu1_dense=t, mu2_dense=tables(-1))):
        with pytest.raises(AssertionError, match="the library was reached"):
            fn(PAIRS, PARAMS, replicas=3, **kw, **({"observed": [1, 2]} if which == 2 else {}))


def test_good_arguments_reach_the_dense_entry_point_and_no_other(monkeypatch):
    """Through make_batch and the real engine.Batch: bialign_batch_create_null_dense is what is called."""
    import bialign_amd.engine as engine
    from bialign_amd import _lib
    patch_creates(monkeypatch)
    reached = []
    monkeypatch.setattr(_lib.lib, "bialign_batch_create_null_dense", lambda *a, **k: reached.append(len(a)) or _lib.E_INVALID,
                        raising=False)
    monkeypatch.setattr(engine, "default_engine", lambda *a, **k: types.SimpleNamespace(_h=None, _batches=set()))
    with pytest.raises(_lib.BialignError):
        sg.null_dense_batch(PAIRS, PARAMS, 3, seed=5, mu1_dense=tables())
    assert reached == [7]
