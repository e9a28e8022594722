"""The dinucleotide null model, host side (no GPU): the Python mirror of the header's DINUCLEOTIDE PERMUTATION -- known
answers, the properties it guarantees, coverage of every sequence it may produce, the capped fallback --, the added
C-ABI symbols, and the argument errors of ``shuffle=`` raised before the library is called."""
import collections
import os
import random
import re

import numpy as np
import pytest

from bialign_amd import significance as sg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bialign.h")
ALPHABETS = ["A", "AC", "ACGU", "ACDEFGHIKLMNPQRSTVWY"]
LENGTHS = list(range(1, 81)) + [200, 1000]


def molecules(m):
    """One random molecule of length m per alphabet, and a skewed one: all A but a single C in the middle."""
    rng = random.Random(1000 + m)
    mols = ["".join(rng.choice(alpha) for _ in range(m)) for alpha in ALPHABETS]
    mols.append("A" * (m // 2) + "C" + "A" * (m - m // 2 - 1))
    return mols


def pair_counts(s):
    return collections.Counter(zip(s, s[1:]))


def check_properties(letters, perm):
    m = len(letters)
    assert sorted(perm) == list(range(m)) and perm[0] == 0
    replica = [letters[x] for x in perm]
    assert pair_counts(replica) == pair_counts(letters)
    assert replica[0] == letters[0] and replica[-1] == letters[-1]
    if m <= 2:
        assert perm == list(range(m))


def test_known_answers():
    s = "GGGGAUAUCCCCAUCG"
    perm = sg.dinucleotide_permutation(0, 0, 0, s).tolist()
    assert perm == [0, 4, 5, 14, 10, 9, 11, 12, 13, 6, 7, 8, 15, 1, 3, 2]
    assert "".join(s[x] for x in perm) == "GAUCCCCAUAUCGGGG"
    assert sg.dinucleotide_permutation(12345, 3, 7, "GCGGGGGAUAUCCCCAUCG").tolist() == \
        [0, 1, 13, 12, 14, 18, 7, 10, 9, 8, 17, 15, 16, 11, 2, 4, 6, 5, 3]


@pytest.mark.parametrize("m", LENGTHS)
def test_properties(m):
    key = (7 * m, m % 5, m % 11)
    for letters in molecules(m):
        perm, draws, gave_up = sg._dinucleotide(*key, letters)
        check_properties(letters, perm.tolist())
        assert not gave_up and draws < sg.TREE_CAP          # the default cap never takes the fallback here
        # renaming the letters changes nothing: any sequence of hashable items with the same pattern
        renamed = [("x", -ord(c)) for c in letters]
        assert len(set(renamed)) == len(set(letters))
        assert sg.dinucleotide_permutation(*key, renamed).tolist() == perm.tolist()
        # CAP = 0: the fallback (unless the last letter is the only one that needs a tree), valid all the same
        perm0, draws0, gave_up0 = sg._dinucleotide(*key, letters, tree_cap=0)
        check_properties(letters, perm0.tolist())
        assert draws0 == 0 and gave_up0 == (m > 2 and len(set(letters[:-1]) - {letters[-1]}) > 0)


def test_replicas_pairs_and_seeds_differ():
    s = "".join(random.Random(5).choice("ACGU") for _ in range(64))
    base = sg.dinucleotide_permutation(9, 4, 2, s).tolist()
    assert sg.dinucleotide_permutation(9, 4, 3, s).tolist() != base
    assert sg.dinucleotide_permutation(9, 5, 2, s).tolist() != base
    assert sg.dinucleotide_permutation(10, 4, 2, s).tolist() != base


def sequences_with_the_same_pairs(s):
    """Brute force: every sequence with s's first letter and s's count of every ordered pair of neighbours."""
    out = []

    def extend(prefix, left):
        if len(prefix) == len(s):
            out.append(prefix)
            return
        for (a, b), k in sorted(left.items()):
            if a == prefix[-1] and k > 0:
                left[(a, b)] -= 1
                extend(prefix + b, left)
                left[(a, b)] += 1
    extend(s[0], dict(pair_counts(s)))
    return out


def test_coverage_is_complete_and_even():
    """40 000 replicas of ACAGCAACGAC: each of the 84 sequences with its pair counts and first letter appears, nothing
    else does, and every count lies within 5 sigma of the binomial (40000 / 84 = 476, sigma = 21.7).  Deterministic."""
    s = "ACAGCAACGAC"
    want = sequences_with_the_same_pairs(s)
    assert len(want) == 84 == len(set(want))
    counts = collections.Counter("".join(s[x] for x in sg.dinucleotide_permutation(3, 0, r, s).tolist()) for r in range(40000))
    assert set(counts) == set(want)
    assert 476 - 109 <= min(counts.values()) and max(counts.values()) <= 476 + 109


def test_shuffle_helpers_take_the_model():
    pair = ("ACGU", "GGGAAACCCUGAGA", "....", "(((...))).....")
    perm = sg.dinucleotide_permutation(7, 2, 5, pair[1]).tolist()
    sa, sb, ta, tb = sg.shuffle_b(pair, 7, 2, 5, rna=True, shuffle="dinucleotide")
    assert (sa, ta) == (pair[0], pair[2])
    assert sb == "".join(pair[1][x] for x in perm) and tb == "".join(pair[3][x] for x in perm)
    assert pair_counts(sb) == pair_counts(pair[1])
    assert sg.shuffle_b(pair, 7, 2, 5, rna=True, shuffle="mono") == sg.shuffle_b(pair, 7, 2, 5, rna=True)
    feats = tuple(np.arange(14, dtype=np.float64) + k for k in (0.25, 100.5, 1000.125))
    seq, planes = sg.shuffle_features(pair[1], feats, 7, 2, 5, shuffle="dinucleotide")
    assert seq == sb and all(np.array_equal(pl, f[perm]) for pl, f in zip(planes, feats))
    table = np.arange(3 * 14).reshape(3, 14)
    np.testing.assert_array_equal(sg.shuffle_tables(table, 7, 2, 5, shuffle="dinucleotide", letters=pair[1]), table[:, perm])
    np.testing.assert_array_equal(sg.shuffle_tables(table, 7, 2, 5), table[:, sg.permutation(7, 2, 5, 14)])
    for bad in (dict(), dict(letters="ACG")):   # a table has no letters of its own
        with pytest.raises(ValueError):
            sg.shuffle_tables(table, 7, 2, 5, shuffle="dinucleotide", **bad)


# ---- the C ABI: two added symbols, the constants, ABI still 10

def test_header_and_binding_declare_the_new_symbols():
    from bialign_amd import _lib
    with open(HEADER) as fh:
        raw = fh.read()
    declared = set(re.findall(r"\b(bialign_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", raw, flags=re.S)))
    for name in ("bialign_batch_set_null_model", "bialign_batch_get_null_model"):
        assert name in declared and name in {n for n, _, _ in _lib.SYMBOLS} and hasattr(_lib.lib, name)
    assert "#define BIALIGN_NULL_MONO 0" in raw and "#define BIALIGN_NULL_DINUCLEOTIDE 1" in raw
    assert (_lib.NULL_MONO, _lib.NULL_DINUCLEOTIDE) == (0, 1) and sg.SHUFFLES == ("mono", "dinucleotide")
    assert "THE DINUCLEOTIDE PERMUTATION" in raw
    bound = int(re.search(r"#define BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN (\d+)", raw).group(1))
    assert bound >= 30000
    assert "#define BIALIGN_ABI_VERSION 10" in raw and _lib.lib.bialign_abi_version() == 10


# ---- argument errors: raised before the library is loaded or called

PAIR = ("ACDE", "ACD", "HHEE", "HHE")
PARAMS = dict(type="Protein", simmatrix="BLOSUM62", structure_weight=800, gap_opening_cost=-150, gap_cost=-50,
              shift_cost=-150, max_shift=1, sequence_match_similarity=100, sequence_mismatch_similarity=0)
MOLS = [("ACGU", (np.zeros(4), np.zeros(4), np.ones(4)))] * 2
TABLE = [np.zeros((4, 3), np.int32)]


@pytest.mark.parametrize("bad", ["Mono", "di", "", None, 1, b"mono"])
def test_shuffle_argument_errors_before_any_library_call(bad, monkeypatch):
    import bialign_amd.batch as batch
    import bialign_amd.engine as engine

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    for mod, name in ((engine, "Batch"), (engine, "default_engine"), (batch, "make_batch"), (batch, "make_feature_batch"),
                      (batch, "encode_flat")):
        monkeypatch.setattr(mod, name, boom)
    for fn in (sg.null_batch, sg.zscores):
        with pytest.raises(ValueError, match="shuffle"):
            fn([PAIR], PARAMS, replicas=3, shuffle=bad)
    for fn in (sg.null_feature_batch, sg.zscores_features):
        with pytest.raises(ValueError, match="shuffle"):
            fn(MOLS, [(0, 1)], PARAMS, replicas=3, shuffle=bad)
    for fn in (sg.null_dense_batch, sg.zscores_dense):
        with pytest.raises(ValueError, match="shuffle"):
            fn([PAIR], PARAMS, replicas=3, mu2_dense=TABLE, shuffle=bad)
    with pytest.raises(ValueError, match="shuffle"):
        sg.shuffle_b(PAIR, 0, 0, 0, shuffle=bad)
    with pytest.raises(ValueError, match="shuffle"):
        sg.shuffle_features("ACGU", MOLS[0][1], 0, 0, 0, shuffle=bad)
    with pytest.raises(ValueError, match="shuffle"):
        sg.shuffle_tables(TABLE[0], 0, 0, 0, shuffle=bad, letters="ACD")


def test_mirror_argument_errors():
    for bad in (dict(seed=-1), dict(seed=2 ** 32), dict(pair=-1), dict(replica=-1), dict(letters=""),
                dict(tree_cap=-1), dict(tree_cap=4097)):
        kw = dict(dict(seed=0, pair=0, replica=0, letters="ACGU"), **bad)
        with pytest.raises(ValueError):
            sg.dinucleotide_permutation(**kw)


def test_batch_cli_zscore_shuffle_needs_zscore(tmp_path, capsys):
    from bialign_amd import batch_cli
    f = tmp_path / "pairs.tsv"
    f.write_text("a\tACGU\t....\tb\tACGU\t....\n")
    with pytest.raises(SystemExit) as e:
        batch_cli._main([str(f), "--zscore_shuffle", "dinucleotide"])
    assert e.value.code == 2 and "--zscore_shuffle needs --zscore" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        batch_cli._main([str(f), "--zscore", "5", "--zscore_shuffle", "trinucleotide"])
