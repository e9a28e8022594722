"""FEATURE form of mu2 (include/bialign.h, bialign_features): the host side -- ABI layout, the factored-out feature
code, the host table the GPU builder is held to, and argument validation.  No GPU involved."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from bialign_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = load_golden("fractional_features.json")
NEW_FUNCTIONS = ["bialign_batch_create_features", "bialign_batch_get_feature_info", "bialign_batch_dump_mu2"]


def header():
    with open(os.path.join(REPO, "include", "bialign.h")) as fh:
        return fh.read()


def test_abi_gains_symbols_only():
    """ABI 10 stays: three new functions and one new input struct, nothing existing changes.

    ``bialign_batch_dump_mu2`` is bound through ``_lib.DIGIT_SYMBOLS`` rather than ``_lib.SYMBOLS``:
    tests/test_capi_symbols.py collects header names with a letters-and-underscores pattern, does not see a name
    with a digit, and requires ``SYMBOLS`` to equal what it collects."""
    from bialign_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"typedef\s+struct\s+bialign_features\s*\{", text)
    bound = [n for n, _, _ in _lib.SYMBOLS] + [n for n, _, _ in _lib.DIGIT_SYMBOLS]
    for name in NEW_FUNCTIONS:
        assert name in bound and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.ABI_VERSION == 10 and "#define BIALIGN_ABI_VERSION 10" in header()
    assert [f for f, _ in _lib.Pairs._fields_] == [
        "npairs", "len_a", "len_b", "off_a", "off_b", "seq_a", "cls_a", "seq_b", "cls_b", "mu2_dense", "mu2_off",
        "mu1_dense", "mu1_off"]
    assert ctypes.sizeof(_lib.Features) == 8 + 6 * ctypes.sizeof(ctypes.c_void_p)
    assert [f for f, _ in _lib.Features._fields_] == ["structure_weight", "up_a", "down_a", "unp_a", "up_b", "down_b", "unp_b"]
    assert ctypes.sizeof(_lib.BatchInfo) == 56 and ctypes.sizeof(_lib.Timing) == 40  # untouched


def test_library_exports_the_new_functions():
    from bialign_amd import build
    lib = ctypes.CDLL(build.build())
    for name in NEW_FUNCTIONS:
        assert hasattr(lib, name), name


def random_bpp(seed, n):
    """Upper-triangular base-pair probabilities, (n+1) x (n+1), 1-based, rows summing to at most 1."""
    rng = np.random.default_rng(seed)
    bpp = np.zeros((n + 1, n + 1))
    for i in range(1, n + 1):
        for j in range(i + 4, n + 1):
            if rng.random() < 0.2:
                bpp[i, j] = rng.random() * 0.3
    sym = bpp + bpp.T
    scale = max(1.0, float(sym.sum(axis=1).max()) * 1.05)
    return bpp / scale


def test_rna_features_are_bialigners_numbers_fixed_structure():
    from bialign_amd import bialignment as ba
    from bialign_amd.scoring import rna_features
    sa, sb, ta, tb = synth.rna_pair(5, 37, 41)
    b = ba.BiAligner(sa, sb, ta, tb, **dict(synth.RNA_PARAMS))
    for mol, seq, st in ((b.molA, sa, ta), (b.molB, sb, tb)):
        got = rna_features(seq, structure=st)
        assert len(got) == 3
        for arr, key in zip(got, ("up", "down", "unp")):
            assert arr.dtype == np.float64 and arr.shape == (len(seq),)
            assert arr.tobytes() == np.array(mol[key][1:], dtype=np.float64).tobytes(), key


def test_rna_features_are_bialigners_numbers_seeded_bpp():
    from bialign_amd import bialignment as ba
    from bialign_amd.scoring import rna_features
    sa, sb, _, _ = synth.rna_pair(6, 33, 29)
    bpa, bpb = random_bpp(21, len(sa)), random_bpp(22, len(sb))
    b = ba.BiAligner(sa, sb, None, None, bppA=bpa, bppB=bpb, **dict(synth.RNA_PARAMS))
    fractional = 0
    for mol, seq, bpp in ((b.molA, sa, bpa), (b.molB, sb, bpb)):
        got = rna_features(seq, bpp=bpp)
        for arr, key in zip(got, ("up", "down", "unp")):
            want = np.array(mol[key][1:], dtype=np.float64)
            assert arr.tobytes() == want.tobytes(), key
            fractional += int(((want != 0.0) & (want != 1.0)).sum())
    assert fractional > 20  # the case is about real numbers
    with pytest.raises(ValueError):
        rna_features(sa, bpp=bpa[:-1, :-1])
    with pytest.raises(ValueError):
        rna_features(sa, structure="." * (len(sa) + 1))


@pytest.mark.parametrize("rec", FEATURES, ids=[r["name"] for r in FEATURES])
def test_host_table_equals_the_references(rec):
    """The comparison side of the GPU tests is pinned to the compiled reference's own mu2 values."""
    from bialign_amd.scoring import dense_mu2_from_features
    assert len(rec["featuresA"]["up"]) == len(rec["seqA"]) + 1  # 1-based lists, entry 0 ignored
    tab = dense_mu2_from_features(rec["featuresA"], rec["featuresB"], rec["params"]["structure_weight"])
    assert tab.dtype == np.int32
    assert tab.tolist() == rec["mu2"]


def molecules(seed, lens):
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        raw = rng.dirichlet([0.6, 0.6, 0.9], size=n)
        seq = "".join(rng.choice(list("ACGU"), size=n))
        out.append((seq, (raw[:, 0].copy(), raw[:, 1].copy(), raw[:, 2].copy())))
    return out


def refuse_library(monkeypatch):
    """Any attempt to create a batch in the library fails the test: validation has to come first."""
    from bialign_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib.lib, "bialign_batch_create_features", boom)
    monkeypatch.setattr(_lib.lib, "bialign_batch_create", boom)
    monkeypatch.setattr(_lib.lib, "bialign_engine_create", boom)


def test_make_feature_batch_argument_errors(monkeypatch):
    from bialign_amd.batch import make_feature_batch
    refuse_library(monkeypatch)
    params = dict(synth.RNA_PARAMS)
    mols = molecules(1, [12, 9, 15])
    for bad_index in ([(0, 3)], [(-1, 0)], [(0, 1), (5, 1)]):
        with pytest.raises(ValueError, match="out of range"):
            make_feature_batch(mols, bad_index, params)
    with pytest.raises(ValueError):
        make_feature_batch(mols, [], params)

    def with_feature(t, which, fn):
        out = [(s, tuple(np.array(x) for x in f)) for s, f in mols]
        fn(out[t][1][which])
        return out

    def set_at(pos, val):
        def fn(arr):
            arr[pos] = val
        return fn
    with pytest.raises(ValueError, match="math domain error"):
        make_feature_batch(with_feature(1, 0, set_at(4, -1e-9)), [(0, 1)], params)
    for val in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="NaN or infinite"):
            make_feature_batch(with_feature(2, 2, set_at(0, val)), [(0, 2)], params)
    ragged = [(s, f) for s, f in mols]
    ragged[0] = (mols[0][0], (mols[0][1][0], mols[0][1][1][:-1], mols[0][1][2]))
    with pytest.raises(ValueError, match="one number per residue"):
        make_feature_batch(ragged, [(0, 1)], params)
    short = [(s, f) for s, f in mols]
    short[1] = (mols[1][0] + "A", mols[1][1])  # sequence longer than its features
    with pytest.raises(ValueError, match="one number per residue"):
        make_feature_batch(short, [(0, 1)], params)
    with pytest.raises(ValueError):
        make_feature_batch([(mols[0][0], mols[0][1][:2])], [(0, 0)], params)  # two arrays instead of three


def test_engine_batch_feature_argument_errors(monkeypatch):
    from bialign_amd.engine import Batch
    refuse_library(monkeypatch)
    (sa, fa), (sb, fb) = molecules(2, [10, 11])
    code = lambda s: (np.zeros(len(s), dtype=np.uint8), np.zeros(len(s), dtype=np.uint8))  # noqa: E731
    s1 = np.zeros((1, 1), dtype=np.int32)
    mk = lambda feat, **kw: Batch(None, [code(sa)], [code(sb)], s1, s1, -150, -50, -200, 1, mu2_features=feat, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="exclude"):
        mk((400, [fa], [fb]), mu2_dense=[np.zeros((10, 11), dtype=np.int32)])
    with pytest.raises(ValueError, match="one .* per pair"):
        mk((400, [fa, fa], [fb]))
    with pytest.raises(ValueError, match="one number per residue"):
        mk((400, [fb], [fb]))
    with pytest.raises(ValueError, match="math domain error"):
        mk((400, [fa], [tuple(-x for x in fb)]))
    with pytest.raises(ValueError, match="integer"):
        mk((400.5, [fa], [fb]))
    with pytest.raises(ValueError):
        mk((400, [fa]))
