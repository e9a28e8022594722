"""Shuffled-null significance, host side (no GPU): the Python mirror of the header's permutation, the added C-ABI
symbols and struct layouts, the z-score arithmetic, and argument errors raised before the library is called."""
import collections
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from bialign_amd import significance as sg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bialign.h")
M32 = 0xFFFFFFFF


def restated_permutation(seed, p, r, m):
    """include/bialign.h, THE PERMUTATION, as a literal loop (every operation reduced to uint32 by hand)."""
    def mix(x):
        x = x & M32
        x = x ^ (x >> 16)
        x = (x * 0x7FEB352D) % (1 << 32)
        x = x ^ (x >> 15)
        x = (x * 0x846CA68B) % (1 << 32)
        x = x ^ (x >> 16)
        return x
    h = mix(seed ^ 0x9E3779B9)
    h = mix((h + p) % (1 << 32))
    h = mix((h + r) % (1 << 32))
    perm = []
    for x in range(m):
        perm.append(x)
    t = m - 1
    while t >= 1:
        draw = (mix((h + t) % (1 << 32)) * (t + 1)) // (1 << 32)
        assert 0 <= draw <= t
        tmp = perm[t]
        perm[t] = perm[draw]
        perm[draw] = tmp
        t -= 1
    return perm


KEYS = [(0, 0, 0), (12345, 3, 7), (1, 0, 65534), (0xFFFFFFFF, 2 ** 31 - 2, 1), (2024, 31, 99)]


@pytest.mark.parametrize("m", [1, 2, 3, 17, 64, 65, 300])
def test_mirror_equals_restatement_and_is_a_permutation(m):
    for seed, p, r in KEYS:
        got = sg.permutation(seed, p, r, m)
        assert got.tolist() == restated_permutation(seed, p, r, m)
        assert sorted(got.tolist()) == list(range(m))
    assert sg.permutation(5, 6, 7, 1).tolist() == [0]


def test_known_answer():
    # computed once with the mirror; pins the mixer's constants and the order of the swaps
    assert sg.permutation(12345, 3, 7, 17).tolist() == [10, 5, 2, 8, 13, 1, 16, 0, 6, 9, 7, 4, 11, 3, 14, 15, 12]


def test_replicas_pairs_and_seeds_differ():
    base = sg.permutation(9, 4, 2, 64).tolist()
    assert sg.permutation(9, 4, 3, 64).tolist() != base
    assert sg.permutation(9, 5, 2, 64).tolist() != base
    assert sg.permutation(10, 4, 2, 64).tolist() != base
    assert len({tuple(sg.permutation(9, 4, r, 64).tolist()) for r in range(50)}) == 50


def test_mixer_is_not_broken():
    """A condition, not a quality claim: over 20 000 replicas of m = 5 all 120 permutations occur, each within
    +-40 % of 20 000 / 120."""
    counts = collections.Counter(tuple(sg.permutation(2024, 0, r, 5).tolist()) for r in range(20000))
    assert len(counts) == 120
    want = 20000 / 120
    assert 0.6 * want <= min(counts.values()) and max(counts.values()) <= 1.4 * want


def test_shuffle_b_moves_letter_and_structure_together():
    pair = ("ACDEF", "GHIKLMNPQR", "HHEEC", "HHHEEECCTT")
    sa, sb, ta, tb = sg.shuffle_b(pair, 7, 2, 5)
    perm = sg.permutation(7, 2, 5, 10).tolist()
    assert (sa, ta) == (pair[0], pair[2])
    assert sb == "".join(pair[1][x] for x in perm) and tb == "".join(pair[3][x] for x in perm)
    # RNA: the position's class travels (".": unpaired, "(": pairs to the right, ")": pairs to the left)
    rna = ("ACGU", "GGGAAACCCU", "....", "(((...))).")
    _, sb, _, tb = sg.shuffle_b(rna, 7, 2, 5, rna=True)
    assert tb == "".join("(((...)))."[x] for x in perm) and sb == "".join(rna[1][x] for x in perm)
    with pytest.raises(ValueError):
        sg.shuffle_b(("A", "AC", ".", "."), 0, 0, 0)


# ---- the C ABI: added symbols, struct layouts, ABI still 10

NEW_SYMBOLS = ["bialign_batch_create_null", "bialign_batch_dump_null_codes", "bialign_batch_get_null_info",
               "bialign_batch_get_null_scores", "bialign_batch_get_null_stats"]


def test_header_and_binding_declare_the_new_symbols():
    from bialign_amd import _lib
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    declared = set(re.findall(r"\b(bialign_[a-z_]+)\s*\(", text))
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in declared and name in bound
        assert hasattr(_lib.lib, name)
    assert "#define BIALIGN_ABI_VERSION 10" in text and _lib.ABI_VERSION == 10
    assert _lib.lib.bialign_abi_version() == 10


def test_struct_layouts_equal_the_headers(tmp_path):
    """sizeof / offsetof of the new structs as a C compiler lays the header out, against the ctypes mirrors."""
    from bialign_amd import _lib
    structs = {"bialign_null_spec": _lib.NullSpec, "bialign_null_stats": _lib.NullStats, "bialign_null_info": _lib.NullInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(out[cname]) == ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            assert int(out[f"{cname}.{field}"]) == getattr(cls, field).offset, (cname, field)
    assert ctypes.sizeof(_lib.NullStats) == 32 and ctypes.sizeof(_lib.NullSpec) == 8


# ---- z-score arithmetic from hand-made integer sums

def _stats(rows):
    keys = ("sum", "sumsq", "min", "max", "n_ge", "replicas")
    return {k: np.array([r[i] for r in rows], dtype=np.int64) for i, k in enumerate(keys)}


def test_zscores_arithmetic():
    # pair 0: replica scores 100, 200, 300, 400 (mean 250, sample variance 50000/3); pair 1: five times 70 (std 0)
    # pair 2: one replica
    st = _stats([(1000, 300000, 100, 400, 1, 4), (350, 24500, 70, 70, 5, 5), (42, 1764, 42, 42, 0, 1)])
    z = sg.zscores_from_stats([400, 70, 50], st)
    assert z["mean"].tolist() == [250.0, 70.0, 42.0]
    assert z["std"][0] == math.sqrt(50000 / 3) and z["std"][1] == 0.0 and math.isnan(z["std"][2])
    assert z["z"][0] == (400 - 250.0) / math.sqrt(50000 / 3)
    assert math.isnan(z["z"][1]) and math.isnan(z["z"][2])
    assert z["p_emp"].tolist() == [2 / 5, 6 / 6, 1 / 2]
    assert z["n_ge"].tolist() == [1, 5, 0] and z["replicas"].tolist() == [4, 5, 1] and z["score"].tolist() == [400, 70, 50]
    # sums near the engine's bounds stay exact: 65535 replicas of 11 000 000 and one of 11 000 001
    R, a = 65535, 11_000_000
    st = _stats([((R - 1) * a + a + 1, (R - 1) * a * a + (a + 1) ** 2, a, a + 1, 1, R)])
    z = sg.zscores_from_stats([a + 1], st)
    var = (1 - 1 / R) / (R - 1)   # one value off by one: sum of squared deviations = 1 - 1/R
    assert abs(z["std"][0] - math.sqrt(var)) < 1e-12
    with pytest.raises(ValueError):
        sg.zscores_from_stats([0], _stats([(10, 1, 0, 0, 0, 2)]))


# ---- argument errors: raised before the library is loaded or called

PAIR = ("ACDE", "ACD", "HHEE", "HHE")
PARAMS = dict(type="Protein", simmatrix="BLOSUM62", structure_weight=800, gap_opening_cost=-150, gap_cost=-50,
              shift_cost=-150, max_shift=1, sequence_match_similarity=100, sequence_mismatch_similarity=0)


@pytest.mark.parametrize("fn", [sg.null_batch, sg.zscores])
def test_argument_errors_before_any_library_call(fn, monkeypatch):
    import bialign_amd.engine as engine

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(engine, "Batch", boom)
    monkeypatch.setattr(engine, "default_engine", boom)
    for bad in (0, -1, 65536, 2.5, "7"):
        with pytest.raises((ValueError, TypeError)):
            fn([PAIR], PARAMS, replicas=bad)
    for bad_seed in (-1, 2 ** 32, 0.5):
        with pytest.raises(ValueError):
            fn([PAIR], PARAMS, replicas=3, seed=bad_seed)
    with pytest.raises(ValueError):
        fn([], PARAMS, replicas=3)
    with pytest.raises(ValueError):
        fn([PAIR] * 40000, PARAMS, replicas=65535)   # npairs * replicas above INT32_MAX
    with pytest.raises(ValueError):
        sg.zscores([PAIR], PARAMS, replicas=3, observed=[1, 2])
    with pytest.raises(ValueError):
        sg.permutation(-1, 0, 0, 4)
    with pytest.raises(ValueError):
        sg.permutation(0, 0, 0, 0)


def test_batch_refuses_null_with_other_forms(monkeypatch):
    """engine.Batch: a null batch excludes the dense / feature forms and the trace modes -- before the library call."""
    from bialign_amd import _lib, engine

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib.lib, "bialign_batch_create_null", boom, raising=False)
    mol = [(np.zeros(3, np.uint8), np.zeros(3, np.uint8))]
    s = np.zeros((1, 1), np.int32)
    for kw in (dict(mu2_dense=[np.zeros((3, 3), np.int32)]), dict(mu1_dense=[np.zeros((3, 3), np.int32)]),
               dict(lean_trace=True), dict(level_trace=True)):
        with pytest.raises(ValueError):
            engine.Batch(None, mol, mol, s, s, -1, -1, -1, 1, null=(3, 0), **kw)
    with pytest.raises(ValueError):
        engine.Batch(None, mol, mol, s, s, -1, -1, -1, 1, null=(0, 0))
