"""Dense mu1 (position-specific sequence scores, include/bialign.h ABI 10): the host side -- ABI layout,
BiAligner(seq_similarity=), scoring.dense_mu1_from_pssm -- and the golden vectors against the CPU oracle."""
import os

import numpy as np
import pytest

from conftest import load_golden
from bialign_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = load_golden("dense_mu1.json")


def test_abi_10_pairs_end_with_the_dense_mu1_fields():
    from bialign_amd import _lib
    assert _lib.ABI_VERSION == 10
    assert [f for f, _ in _lib.Pairs._fields_][-2:] == ["mu1_dense", "mu1_off"]
    with open(os.path.join(REPO, "include", "bialign.h")) as fh:
        h = fh.read()
    assert "#define BIALIGN_ABI_VERSION 10" in h
    assert "const int32_t* mu1_dense;" in h and "const int64_t* mu1_off;" in h


def _aligner(n=7, m=6, seed=3, table=None, **ov):
    from bialign_amd import bialignment as ba
    sa, sb, ta, tb = synth.protein_pair(seed, n, m)
    params = dict(synth.PROTEIN_PARAMS, nameA="A", nameB="B", **ov)
    return ba.BiAligner(sa, sb, ta, tb, seq_similarity=table, **params)


def test_bialigner_seq_similarity_is_mu1():
    t = np.arange(42, dtype=np.int64).reshape(7, 6) * 13 - 200
    b = _aligner(table=t)
    for i in range(1, 8):
        for j in range(1, 7):
            assert b.mu1(i, j) == t[i - 1, j - 1]
    idx = (3, 4, 2, 5)
    scores = [sc for _, sc in b.recursion_cases(idx)]
    m1, m2 = int(t[2, 3]), b.mu2(2, 5)
    assert scores[0] == m1 + m2 and m1 + b._params["shift_cost"] in scores
    aff = list(b.affine_recursion_cases([1, 1, 1, 1], idx))
    plain = _aligner()
    aff_plain = list(plain.affine_recursion_cases([1, 1, 1, 1], idx))
    # same cases, scores shifted by the change of mu1 where the column matches in A
    d = m1 - plain.mu1(3, 4)
    assert [(s, o) for s, o, _ in aff] == [(s, o) for s, o, _ in aff_plain]
    assert aff[0][2] == aff_plain[0][2] + d


@pytest.mark.parametrize("shape", [(6, 7), (7,), (7, 6, 1)])
def test_bialigner_seq_similarity_shape_is_checked(shape):
    with pytest.raises(ValueError):
        _aligner(table=np.zeros(shape, dtype=np.int32))


def test_bialigner_seq_similarity_must_be_integer():
    with pytest.raises(ValueError):
        _aligner(table=np.zeros((7, 6), dtype=np.float64))


def test_dense_mu1_from_pssm_matches_a_loop():
    from bialign_amd.scoring import dense_mu1_from_pssm
    rng = np.random.default_rng(5)
    alphabet = "ACDEFGHIKLMNPQRSTVWY"
    pssm = rng.integers(-400, 900, size=(13, len(alphabet)))
    seq_b = "".join(rng.choice(list(alphabet), size=11))
    got = dense_mu1_from_pssm(pssm, alphabet, seq_b)
    want = np.array([[pssm[i, alphabet.index(c)] for c in seq_b] for i in range(13)])
    assert got.dtype == np.int32 and got.shape == (13, 11)
    np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError):
        dense_mu1_from_pssm(pssm, alphabet, "ACDXA")
    with pytest.raises(ValueError):
        dense_mu1_from_pssm(pssm[:, :5], alphabet, "ACD")


def _tables(rec):
    from oracle import oracle
    n, m = len(rec["seqA"]), len(rec["seqB"])
    _, mu2 = oracle.mu_tables(rec["seqA"], rec["seqB"], rec["strA"], rec["strB"], rec["params"])
    mu1 = np.zeros((n + 1, m + 1), dtype=np.int64)
    mu1[1:, 1:] = np.asarray(rec["mu1"])
    return n, m, mu1, mu2


def test_golden_file_covers_the_modes():
    names = [r["name"] for r in GOLDEN]
    assert any(n.startswith("rna") for n in names) and any(n.startswith("protein") for n in names)
    shifts = {r["params"]["max_shift"] for r in GOLDEN}
    assert {0, 1, 2, 3}.issubset(shifts) and max(shifts) > 5
    assert {r["params"]["gap_opening_cost"] != 0 for r in GOLDEN} == {True, False}
    assert any("layers" in r for r in GOLDEN)


@pytest.mark.parametrize("rec", GOLDEN, ids=[r["name"] for r in GOLDEN])
def test_golden_dense_mu1_against_the_oracle(rec):
    """The recorded reference runs with an overridden _sequence_similarity equal the oracle on the same tables."""
    from oracle import oracle
    n, m, mu1, mu2 = _tables(rec)
    ref = oracle.solve_tables(n, m, rec["params"], mu1, mu2)
    assert ref["score"] == rec["score"]
    assert oracle.trace_to_lists(ref["trace"]) == rec["trace"]
    assert ref["complete"] == rec["complete"]
