"""What a local alignment (BIALIGN_BATCH_LOCAL, include/bialign.h) must give, from the CPU oracle alone: free starts in
both molecules, where tests/fit_expected.py has them in B (tests/free_ends_expected.py holds what the two share).

A DP value depends only on prefixes: one oracle fill of (A[i0:], B[j0:]) holds, at its diagonal points
(i1 - i0, j1 - j0, i1 - i0, j1 - j0), the global score of A[i0:i1] against B[j0:j1] for every (i1, j1) at once.  So
n * m oracle fills give every window's global score, and with them the local score (their maximum; the empty windows
give 0), the smallest end that attains it, and the LOCAL layers: per state and cell the maximum over (i0, j0) of that
run's layer shifted by both offsets (a max-plus DP with several free sources is the maximum of the single-source DPs;
a path never moves left or up, so a run's source bounds its cells like the lattice's edge).  The oracle refuses empty
molecules: a window that is empty in A is row 0 of any run of the same j0 (it depends on B alone), one that is empty in
B column 0 of any run of the same i0.

One expectation costs about W^2 n^2 m^2 / 4 band cells, at about 0.6 M affine cells per second and core (the one-layer
recurrence: a fifteenth of that).

Also the test inputs of tests/test_gpu_local.py and tests/test_local_host.py: seeded pairs, the planted ones with a
mutated common core inside unrelated flanks in both molecules.
"""
import random

import numpy as np

from bialign_amd import synth
from free_ends_expected import NONE, NONE32, _mutate, cell_seconds, compare_layers, plain_pair, pool_map, run_mask, tables_of  # noqa: F401
from oracle import oracle


def cut_tables(mu1, mu2, i0, j0):
    """The (n-i0+1) x (m-j0+1) tables of A[i0:] against B[j0:] out of the pair's (n+1) x (m+1) tables (row and column 0
    stay)."""
    def cut(t):
        t = np.concatenate([t[:1], t[i0 + 1:]], axis=0)
        return np.ascontiguousarray(np.concatenate([t[:, :1], t[:, j0 + 1:]], axis=1))
    return cut(mu1), cut(mu2)


def window_global(params, mu1, mu2, i0, i1, j0, j1):
    """global(A[i0:i1], B[j0:j1]) by one plain oracle run on the explicitly cut window (both parts non-empty)."""
    c1, c2 = mu1[i0:i1 + 1, j0:j1 + 1].copy(), mu2[i0:i1 + 1, j0:j1 + 1].copy()
    c1[0] = c1[:, 0] = c2[0] = c2[:, 0] = 0
    return oracle.solve_tables(i1 - i0, j1 - j0, params, np.ascontiguousarray(c1), np.ascontiguousarray(c2), want_trace=False)["score"]


def local_partial(job):
    """Pool worker (spawned: no GPU state).  ``(key, n, m, params, mu1, mu2, lo, hi, want_layers, want_windows)``: the
    oracle runs of the starts i0 = lo..hi-1 (every j0 each; hi == n: the windows that start at i0 = n too) ->
    ``(key, lo, hi, ends, edge, layers, win)``.  ``ends[i1, j1]``: the best window that ends there among these runs;
    ``edge``: likewise among the starts with i0 == 0 or j0 == 0; ``layers``: the maximum of these runs' shifted layers as
    int32 (NONE32 where none has the cell), or None; ``win[i0 - lo, j0, i1, j1]`` int32 (rows lo..hi, hi included
    when hi == n), or None."""
    key, n, m, params, mu1, mu2, lo, hi, want_layers, want_windows = job
    s = params["max_shift"]
    nl, w = (9 if params["gap_opening_cost"] != 0 else 1), 2 * s + 1
    last = hi == n
    ends = np.full((n + 1, m + 1), NONE, dtype=np.int64)
    edge = np.full((n + 1, m + 1), NONE, dtype=np.int64)
    layers = np.full((nl, n + 1, m + 1, w, w), NONE32, dtype=np.int32) if want_layers else None
    win = np.full((hi - lo + (1 if last else 0), m + 1, n + 1, m + 1), NONE32, dtype=np.int32) if want_windows else None

    def take(i0, j0, diag, lay, ok):
        """One source (i0, j0): ``diag`` its windows' scores by end, ``lay`` its layers from (i0, j0) on, ``ok`` its cells."""
        ends[i0:i0 + diag.shape[0], j0:j0 + diag.shape[1]] = np.maximum(ends[i0:i0 + diag.shape[0], j0:j0 + diag.shape[1]], diag)
        if i0 == 0 or j0 == 0:
            edge[i0:i0 + diag.shape[0], j0:j0 + diag.shape[1]] = np.maximum(edge[i0:i0 + diag.shape[0], j0:j0 + diag.shape[1]], diag)
        if win is not None:
            win[i0 - lo, j0, i0:i0 + diag.shape[0], j0:j0 + diag.shape[1]] = diag
        if layers is not None:
            sl = (slice(None), slice(i0, i0 + lay.shape[1]), slice(j0, j0 + lay.shape[2]))
            layers[sl] = np.maximum(layers[sl], np.where(ok[None], lay, NONE32))

    for i0 in range(lo, hi):
        for j0 in range(m):
            c1, c2 = cut_tables(mu1, mu2, i0, j0)
            lay = oracle.solve_tables(n - i0, m - j0, params, c1, c2, want_trace=False)["layers"]
            take(i0, j0, lay[:, :, :, s, s].max(axis=0), lay, run_mask(n - i0, m - j0, s))
            if j0 == m - 1:  # the windows B[m:m]: column 0 of this run, standing at column m
                take(i0, m, lay[:, :, :1, s, s].max(axis=0), lay[:, :, :1], run_mask(n - i0, 0, s))
            if last and i0 == n - 1:  # the windows A[n:n]: row 0 of this run, standing at row n
                take(n, j0, lay[:, :1, :, s, s].max(axis=0), lay[:, :1], run_mask(0, m - j0, s))
                if j0 == m - 1:  # ... and the one that is empty in both: the origin
                    take(n, m, lay[:, :1, :1, s, s].max(axis=0), lay[:, :1, :1], run_mask(0, 0, s))
    return key, lo, hi, ends, edge, layers, win


def split_jobs(key, n, m, params, mu1, mu2, want_layers=True, want_windows=False, seconds=3.0):
    """The jobs of one pair for ``local_partial``: the starts i0 = 0..n-1 cut into ranges of about ``seconds`` of oracle
    time each (the runs of one i0 cost about (n - i0) m^2 / 2 lattice points)."""
    per_row = m * m / 2 * cell_seconds(params)
    jobs, lo, acc = [], 0, 0.0
    for i0 in range(n):
        acc += per_row * (n - i0)
        if acc >= seconds or i0 == n - 1:
            jobs.append((key, n, m, params, mu1, mu2, lo, i0 + 1, want_layers, want_windows))
            lo, acc = i0 + 1, 0.0
    return jobs


def local_combine(n, m, parts):
    """The parts of one pair (``local_partial`` results, any order) -> dict: ``score``; ``end`` = (end_a, end_b), the
    smallest i, then the smallest j, that attains it; ``ends`` int64 [n+1, m+1], the best window by end; ``edge`` likewise
    among the windows that start at A's or at B's first residue; ``inner``: the best end lies before both molecules' ends
    and no window that starts at a first residue attains the score there; ``layers`` int64 [NL, n+1, m+1, W, W], the
    expected LOCAL layers in the reference layout (NONE where no run has the cell), or None; ``windows`` int32
    [n+1, m+1, n+1, m+1] = [i0, j0, i1, j1] (NONE32: no such window), or None."""
    ends = np.full((n + 1, m + 1), NONE, dtype=np.int64)
    edge = np.full((n + 1, m + 1), NONE, dtype=np.int64)
    layers, windows = None, None
    for _, lo, hi, e, g, lay, win in parts:
        ends, edge = np.maximum(ends, e), np.maximum(edge, g)
        if lay is not None:
            layers = lay.copy() if layers is None else np.maximum(layers, lay)
        if win is not None:
            if windows is None:
                windows = np.full((n + 1, m + 1, n + 1, m + 1), NONE32, dtype=np.int32)
            windows[lo:lo + len(win)] = win
    if layers is not None:
        layers = np.where(layers == NONE32, NONE, layers.astype(np.int64))
    score = int(ends.max())
    end_a, end_b = (int(x) for x in np.argwhere(ends == score)[0])  # row-major: the smallest i, then the smallest j
    inner = 0 < end_a < n and 0 < end_b < m and int(edge[end_a, end_b]) < score
    return dict(score=score, end=(end_a, end_b), ends=ends, edge=edge, inner=inner, layers=layers, windows=windows)


def local_expected(n, m, params, mu1, mu2, want_layers=True, want_windows=True):
    """One pair, in this process."""
    return local_combine(n, m, [local_partial(j) for j in split_jobs(0, n, m, params, mu1, mu2, want_layers, want_windows, 1e9)])


def expected_many(cases, procs=None):
    """``cases``: {key: (n, m, params, mu1, mu2, want_layers)} -> {key: local_combine's dict}; the oracle runs of all
    cases share one spawn pool."""
    jobs = [j for key, c in cases.items() for j in split_jobs(key, *c)]
    jobs.sort(key=lambda j: -sum(j[1] - i0 for i0 in range(j[6], j[7])) * j[2] * j[2] * (2 * j[3]["max_shift"] + 1) ** 2 *
              (15 if j[3]["gap_opening_cost"] != 0 else 1))  # (roughly) the long ones first
    done = pool_map(local_partial, jobs, procs)
    return {key: local_combine(c[0], c[1], [d for d in done if d[0] == key]) for key, c in cases.items()}


def span_score(want, params, mu1, mu2, span):
    """The global score of the window ``span`` = (start_a, end_a, start_b, end_b): from ``want['windows']`` where the
    expectation kept them, else by one oracle run of the cut window (an empty part: from ``want['ends']`` alone, where
    the window is the only one that ends where it starts)."""
    i0, i1, j0, j1 = span
    if want.get("windows") is not None:
        return int(want["windows"][i0, j0, i1, j1])
    if i0 == i1 and j0 == j1:
        return 0
    assert i0 < i1 and j0 < j1, "a window that is empty in one molecule only: keep the windows to score it"
    return window_global(params, mu1, mu2, i0, i1, j0, j1)


def planted_pair(seed, n, m):
    """A protein pair with a mutated common core inside unrelated flanks in both molecules.  The core and B's flanks
    avoid W, Y and F; A's flanks are W with a structure letter of their own, so aligning a flank residue costs more
    than leaving it out.  Too short for a core with flanks on both sides (n or m below 5): a plain pair."""
    if min(n, m) < 5:
        return synth.protein_pair(seed, n, m)
    rng = random.Random(seed)
    c = max(2, min(n, m) // 2)
    wa, wb = rng.randint(1, n - c - 1), rng.randint(1, m - c - 1)
    alpha = "".join(ch for ch in synth.PROTEIN_ALPHABET if ch not in "WYF")
    core_seq, core_str = synth._draw(rng, alpha, c), synth._draw(rng, "HEC", c)
    seq_b = synth._draw(rng, alpha, wb) + core_seq + synth._draw(rng, alpha, m - wb - c)
    str_b = synth._draw(rng, "HEC", wb) + core_str + synth._draw(rng, "HEC", m - wb - c)
    seq_a = "W" * wa + _mutate(rng, core_seq, alpha) + "W" * (n - wa - c)
    str_a = "T" * wa + _mutate(rng, core_str, "HEC") + "T" * (n - wa - c)
    return seq_a, seq_b, str_a, str_b


def make_pair(kind, seed, n, m, planted):
    return planted_pair(seed, n, m) if planted else plain_pair(kind, seed, n, m)
