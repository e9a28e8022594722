"""What tests/test_gpu_fit.py and tests/test_gpu_local.py share: the parameter sets, seeded inputs of the dense and
FEATURE forms with the tables the oracle takes for them, and the statistics a null batch must reduce to."""
import math

import numpy as np

from bialign_amd import synth
from free_ends_expected import tables_of

COSTS = {"affine": {}, "one-layer": dict(gap_opening_cost=0), "beta>0": dict(gap_opening_cost=100)}
BASE = {"protein": synth.PROTEIN_PARAMS, "rna": synth.RNA_PARAMS}


def params_of(kind, cost, s):
    return dict(BASE[kind], max_shift=s, **COSTS[cost])


def pair_of(make_pair, seed0):
    """-> pair_of(kind, n, m, planted) of a module: ``make_pair`` with a seed from the shape, counted from ``seed0``."""
    return lambda kind, n, m, planted: make_pair(kind, seed0 + 31 * n + m + (500 if planted else 0), n, m, planted)


def feature_molecules(seed, lengths):
    """Two RNA molecules with real-valued features (A, then the longer B): three non-negative numbers per residue that
    sum to 1."""
    rng = np.random.default_rng(seed)
    mols = []
    for length in lengths:
        seq = "".join(rng.choice(list(synth.RNA_ALPHABET), size=length))
        f = rng.random((3, length))
        f /= f.sum(axis=0)
        mols.append((seq, tuple(np.ascontiguousarray(x) for x in f)))
    return mols


def feature_mu2(fa, fb, sw):
    """(n+1) x (m+1) table of the reference's expression (pyx:416-423), row and column 0 zero."""
    n, m = len(fa[0]), len(fb[0])
    tab = np.zeros((n + 1, m + 1), dtype=np.int32)
    for k in range(n):
        for l in range(m):
            tab[k + 1, l + 1] = int(sw * (math.sqrt(fa[0][k] * fb[0][l]) + math.sqrt(fa[1][k] * fb[1][l]) + math.sqrt(fa[2][k] * fb[2][l])))
    return tab


def seq_mu1(seq_a, seq_b, params):
    return tables_of((seq_a, seq_b, "." * len(seq_a), "." * len(seq_b)), dict(params, type="RNA"))[0]


def pad(tab):
    """An (n, m) dense table as the oracle's (n+1) x (m+1) table."""
    out = np.zeros((tab.shape[0] + 1, tab.shape[1] + 1), dtype=np.int32)
    out[1:, 1:] = tab
    return out


def form_tables(pair, params):
    """The dense tables of the forms' cases: mu1 and mu2 of ``pair`` with position-specific changes."""
    rng = np.random.default_rng(9)
    mu1, mu2 = tables_of(pair, params)
    shape = (len(pair[0]), len(pair[1]))
    d1 = (mu1[1:, 1:] + rng.integers(-150, 150, size=shape)).astype(np.int32)
    d2 = (mu2[1:, 1:] + rng.integers(-200, 200, size=shape)).astype(np.int32)
    return mu1, mu2, d1, d2


def stats_of(replica_scores, observed):
    arr = np.asarray(replica_scores, dtype=np.int64)
    return dict(sum=arr.sum(axis=1), sumsq=(arr * arr).sum(axis=1), min=arr.min(axis=1), max=arr.max(axis=1),
                n_ge=(arr >= np.asarray(observed)[:, None]).sum(axis=1), replicas=np.full(len(arr), arr.shape[1]))
