"""What the expectations of the free-ends modes share (tests/fit_expected.py: BIALIGN_BATCH_FIT, tests/local_expected.py:
BIALIGN_BATCH_LOCAL): the sentinels of the expected layers and their comparison with a dump, the cost model of the job
splitters, the spawn pool the oracle runs share, and the plain test inputs.  What a mode MEANS stays in its own module
(``fit_partial`` / ``fit_combine``, ``local_partial`` / ``local_combine``), each checked against the plain oracle on cut
windows by its host test."""
import numpy as np

from bialign_amd import synth
from oracle import oracle

NEG_INF = -(1 << 30)   # BIALIGN_NEG_INF
LOW = NEG_INF // 2     # layers are compared where the expectation is above this
NONE = -(1 << 40)      # "no such window" / "no run covers this cell"
NONE32 = -(1 << 31)    # ... in the int32 layers a pool worker hands back


def run_mask(n, mr, s):
    """[i, j, a, b] -> is (i, j, i+a-s, j+b-s) a cell of the n x mr lattice (the oracle leaves the others unwritten)."""
    w = 2 * s + 1
    i = np.arange(n + 1)[:, None, None, None]
    j = np.arange(mr + 1)[None, :, None, None]
    k = i + np.arange(w)[None, None, :, None] - s
    l = j + np.arange(w)[None, None, None, :] - s
    return (k >= 0) & (k <= n) & (l >= 0) & (l <= mr)


def compare_layers(got, want, n, m, s):
    """The engine's dump against an expectation's layers, over the in-band cells: equal where the expectation is above
    LOW, below LOW too elsewhere."""
    ok = run_mask(n, m, s)[None]
    want = np.where(ok, want, NONE)
    hi = ok & (want > LOW)
    np.testing.assert_array_equal(got[hi], want[hi])
    assert (got[ok & ~hi] <= LOW).all()


def tables_of(pair, params):
    sa, sb, ta, tb = pair
    return oracle.mu_tables(sa, sb, ta, tb, params)


def cell_seconds(params):
    """Oracle time per lattice point of a run: (2 s + 1)^2 band cells at 0.6 M affine band cells per second and core
    (measured); the one-layer recurrence takes a fifteenth."""
    return (2 * params["max_shift"] + 1) ** 2 * (1.0 if params["gap_opening_cost"] != 0 else 1 / 15) / 0.6e6


def pool_map(worker, jobs, procs=None):
    """``worker`` over ``jobs`` in one spawn pool (spawned: no GPU state), results in the jobs' order."""
    import multiprocessing as mp
    import os
    procs = procs or max(1, min(16, len(os.sched_getaffinity(0)), len(jobs)))
    oracle.lib()  # (built on first use: here, not by sixteen workers at once)
    with mp.get_context("spawn").Pool(procs) as pool:
        return pool.map(worker, jobs, chunksize=1)


def _mutate(rng, text, alphabet, rate=0.15):
    return "".join(rng.choice(alphabet) if rng.random() < rate else ch for ch in text)


def plain_pair(kind, seed, n, m):
    return synth.rna_pair(seed, n, m) if kind == "rna" else synth.protein_pair(seed, n, m)
