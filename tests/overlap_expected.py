"""What an overlap alignment (BIALIGN_BATCH_OVERLAP, include/bialign.h) must give, from the CPU oracle alone: the global
alignment whose end gaps are free in both molecules (tests/free_ends_expected.py holds what the free-ends modes share,
tests/local_expected.py the cut of a pair's tables to a start in both molecules).

A DP value depends only on prefixes: one oracle fill of (A[i0:], B[j0:]) holds, at its diagonal points, the global score
of A[i0:i1] against B[j0:j1] for every (i1, j1) at once.  An overlap alignment starts at A's first residue or at B's:
its sources are (i0, 0), i0 = 0..n, and (0, j0), j0 = 1..m -- n + m + 1 oracle fills per pair.  Together they give the
score (the best window that ends at A's or at B's last residue), the smallest end cell that attains it, every admissible
window's score, and the OVERLAP layers: per state and cell the maximum over the sources of that run's layer shifted by
its offset (a max-plus DP with several free sources is the maximum of the single-source DPs; a path never moves left or
up, so a run's source bounds its cells like the lattice's edge).  The oracle refuses empty molecules: the source (n, 0)
is row 0 of the run of (n - 1, 0), which depends on B alone, standing at row n; the source (0, m) is column 0 of the run
of (0, m - 1) standing at column m.

The end cells in position order: x < n -> (x, m), else (n, x - n), x = 0..n+m -- the order by (i, j).

Also the test inputs of tests/test_gpu_overlap.py and tests/test_overlap_host.py: seeded pairs of four planted kinds
(``planted_pair``) and plain ones.
"""
import random

import numpy as np

from bialign_amd import synth
from free_ends_expected import NONE, NONE32, _mutate, cell_seconds, compare_layers, plain_pair, pool_map, run_mask, tables_of  # noqa: F401
from local_expected import cut_tables, window_global  # noqa: F401
from oracle import oracle

KINDS = ("a_suffix_b_prefix", "b_suffix_a_prefix", "a_in_b", "b_in_a")


def sources(n, m):
    """The free starts (i0, j0) in the order of the jobs: A's, then B's."""
    return [(i0, 0) for i0 in range(n + 1)] + [(0, j0) for j0 in range(1, m + 1)]


def end_cells(n, m):
    """(i, j) int arrays of the end cells in position order."""
    x = np.arange(n + m + 1)
    return np.where(x < n, x, n), np.where(x < n, m, x - n)


def overlap_partial(job):
    """Pool worker (spawned: no GPU state).  ``(key, n, m, params, mu1, mu2, srcs, want_layers)``: the oracle runs of the
    sources ``srcs`` (non-empty in both molecules; the run of (n - 1, 0) also yields the source (n, 0), the run of
    (0, m - 1) the source (0, m)) -> ``(key, ends, layers, rows)``.  ``ends[i1, j1]``: the best window that ends there
    among these sources (NONE: none); ``layers``: the maximum of these runs' shifted layers as int32 (NONE32 where none has
    the cell), or None; ``rows``: [((i0, j0), scores by end position as int32, NONE32 where the window does not exist)]."""
    key, n, m, params, mu1, mu2, srcs, want_layers = job
    s = params["max_shift"]
    nl, w = (9 if params["gap_opening_cost"] != 0 else 1), 2 * s + 1
    ends = np.full((n + 1, m + 1), NONE, dtype=np.int64)
    layers = np.full((nl, n + 1, m + 1, w, w), NONE32, dtype=np.int32) if want_layers else None
    ei, ej = end_cells(n, m)
    rows = []

    def take(i0, j0, diag, lay, ok):
        """One source: ``diag`` its windows' scores by end, ``lay`` its layers from (i0, j0) on, ``ok`` its cells."""
        sl = (slice(i0, i0 + diag.shape[0]), slice(j0, j0 + diag.shape[1]))
        ends[sl] = np.maximum(ends[sl], diag)
        full = np.full((n + 1, m + 1), NONE32, dtype=np.int64)
        full[sl] = diag
        rows.append(((i0, j0), full[ei, ej].astype(np.int32)))
        if layers is not None:
            layers[(slice(None),) + sl] = np.maximum(layers[(slice(None),) + sl], np.where(ok[None], lay, NONE32))

    for i0, j0 in srcs:
        c1, c2 = cut_tables(mu1, mu2, i0, j0)
        lay = oracle.solve_tables(n - i0, m - j0, params, c1, c2, want_trace=False)["layers"]
        take(i0, j0, lay[:, :, :, s, s].max(axis=0), lay, run_mask(n - i0, m - j0, s))
        if j0 == 0 and i0 == n - 1:  # the source (n, 0): row 0 of this run, standing at row n
            take(n, 0, lay[:, :1, :, s, s].max(axis=0), lay[:, :1], run_mask(0, m, s))
        if i0 == 0 and j0 == m - 1:  # the source (0, m): column 0 of this run, standing at column m
            take(0, m, lay[:, :, :1, s, s].max(axis=0), lay[:, :, :1], run_mask(n, 0, s))
    return key, ends, layers, rows


def split_jobs(key, n, m, params, mu1, mu2, want_layers=True, seconds=3.0):
    """The jobs of one pair for ``overlap_partial``: the sources with a run of their own, cut into groups of about
    ``seconds`` of oracle time each (a run costs about (n - i0) (m - j0) lattice points)."""
    per_point = cell_seconds(params)
    jobs, group, acc = [], [], 0.0
    todo = [(i0, j0) for i0, j0 in sources(n, m) if i0 < n and j0 < m]
    for at, (i0, j0) in enumerate(todo):
        group.append((i0, j0))
        acc += per_point * (n - i0) * (m - j0)
        if acc >= seconds or at == len(todo) - 1:
            jobs.append((key, n, m, params, mu1, mu2, group, want_layers))
            group, acc = [], 0.0
    return jobs


def overlap_combine(n, m, parts):
    """The parts of one pair (``overlap_partial`` results, any order) -> dict: ``score``; ``end`` = (end_a, end_b), the end
    cell with the smallest i, then the smallest j, that attains it; ``ends`` int64 [n+1, m+1], the best admissible start
    by end (all cells, NONE: none); ``windows``: {(i0, j0): int32 scores by end position}, every admissible window;
    ``starts``: the sources whose window to ``end`` attains the score; ``layers`` int64 [NL, n+1, m+1, W, W], the expected
    OVERLAP layers in the reference layout (NONE where no run has the cell), or None."""
    ends = np.full((n + 1, m + 1), NONE, dtype=np.int64)
    layers, windows = None, {}
    for _, e, lay, rows in parts:
        ends = np.maximum(ends, e)
        if lay is not None:
            layers = lay.copy() if layers is None else np.maximum(layers, lay)
        windows.update(rows)
    assert sorted(windows) == sorted(sources(n, m))
    if layers is not None:
        layers = np.where(layers == NONE32, NONE, layers.astype(np.int64))
    ei, ej = end_cells(n, m)
    line = ends[ei, ej]
    score = int(line.max())
    x = int(np.argmax(line == score))  # position order = the order by (i, j)
    starts = sorted(src for src, row in windows.items() if int(row[x]) == score)
    return dict(score=score, end=(int(ei[x]), int(ej[x])), ends=ends, windows=windows, starts=starts, layers=layers)


def window_score(want, n, m, span):
    """The score of the window ``span`` = (start_a, end_a, start_b, end_b) if it is admissible, else None."""
    i0, i1, j0, j1 = span
    if not ((i0 == 0 or j0 == 0) and (i1 == n or j1 == m) and 0 <= i0 <= i1 <= n and 0 <= j0 <= j1 <= m):
        return None
    x = i1 if (j1 == m and i1 < n) else n + j1
    v = int(want["windows"][(i0, j0)][x])
    return None if v == NONE32 else v


def overlap_expected(n, m, params, mu1, mu2, want_layers=True):
    """One pair, in this process."""
    return overlap_combine(n, m, [overlap_partial(j) for j in split_jobs(0, n, m, params, mu1, mu2, want_layers, 1e9)])


def expected_many(cases, procs=None):
    """``cases``: {key: (n, m, params, mu1, mu2, want_layers)} -> {key: overlap_combine's dict}; the oracle runs of all
    cases share one spawn pool."""
    jobs = [j for key, c in cases.items() for j in split_jobs(key, *c)]
    jobs.sort(key=lambda j: -sum((j[1] - i0) * (j[2] - j0) for i0, j0 in j[6]) * cell_seconds(j[3]))  # the long ones first
    done = pool_map(overlap_partial, jobs, procs)
    return {key: overlap_combine(c[0], c[1], [d for d in done if d[0] == key]) for key, c in cases.items()}


def geometry(kind, want, n, m):
    """Do the expected spans of a planted pair have its kind's geometry?  (Every start that attains the score counts.)"""
    (ea, eb), starts = want["end"], want["starts"]
    if kind == "a_suffix_b_prefix":
        return ea == n and eb < m and all(i0 > 0 and j0 == 0 for i0, j0 in starts)
    if kind == "b_suffix_a_prefix":
        return ea < n and eb == m and all(i0 == 0 and j0 > 0 for i0, j0 in starts)
    if kind == "a_in_b":
        return ea == n and eb < m and all(i0 == 0 and j0 > 0 for i0, j0 in starts)
    if kind == "b_in_a":
        return ea < n and eb == m and all(i0 > 0 and j0 == 0 for i0, j0 in starts)
    raise ValueError(kind)


def planted_pair(kind, seed, n, m):
    """A protein pair of one of the four planted kinds.  The shared stretch is a mutated copy; what overhangs it is
    unrelated: in A tryptophans with a structure letter of their own, in B letters other than W, Y and F, so that aligning
    an overhanging residue costs more than leaving it out.
      a_suffix_b_prefix: A = overhang + core', B = core + overhang      b_suffix_a_prefix: A = core' + overhang, B = overhang + core
      a_in_b: A = core', B = overhang + core + overhang                 b_in_a: A = overhang + core' + overhang, B = core
    Too short for its kind: a plain pair."""
    rng = random.Random(seed)
    alpha = "".join(ch for ch in synth.PROTEIN_ALPHABET if ch not in "WYF")
    draw = lambda k: (synth._draw(rng, alpha, k), synth._draw(rng, "HEC", k))
    over_a = lambda k: ("W" * k, "T" * k)
    mut = lambda core: (_mutate(rng, core[0], alpha), _mutate(rng, core[1], "HEC"))
    cat = lambda *parts: ("".join(p[0] for p in parts), "".join(p[1] for p in parts))
    if kind in ("a_suffix_b_prefix", "b_suffix_a_prefix"):
        c = min(n, m) * 2 // 3
        if c < 2 or c >= min(n, m):
            return synth.protein_pair(seed, n, m)
        core = draw(c)
        if kind == "a_suffix_b_prefix":
            a, b = cat(over_a(n - c), mut(core)), cat(core, draw(m - c))
        else:
            a, b = cat(mut(core), over_a(n - c)), cat(draw(m - c), core)
    elif kind == "a_in_b":
        if m < n + 2:
            return synth.protein_pair(seed, n, m)
        w = rng.randint(1, m - n - 1)
        core = draw(n)
        a, b = mut(core), cat(draw(w), core, draw(m - n - w))
    elif kind == "b_in_a":
        if n < m + 2:
            return synth.protein_pair(seed, n, m)
        w = rng.randint(1, n - m - 1)
        core = draw(m)
        a, b = cat(over_a(w), mut(core), over_a(n - m - w)), core
    else:
        raise ValueError(kind)
    return a[0], b[0], a[1], b[1]


def make_pair(kind, seed, n, m, planted):
    """``planted``: one of KINDS, or a false value for a plain pair of ``kind`` ("protein" / "rna")."""
    return planted_pair(planted, seed, n, m) if planted else plain_pair(kind, seed, n, m)
