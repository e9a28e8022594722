"""What a fit alignment (BIALIGN_BATCH_FIT, include/bialign.h) must give, from the CPU oracle alone.

A DP value depends only on prefixes: one oracle fill of (A, B[j0:]) holds, at (n, j1 - j0, n, j1 - j0), the global
score of A against B[j0:j1] for every j1 at once.  So m oracle fills give every substring's global score, and with
them the fit score (their maximum, the empty substring included), the smallest end that attains it, and the FIT
layers: per state and cell the maximum over j0 of the j0-run's layer shifted by j0 in j and l (a max-plus DP with
several free sources is the maximum of the single-source DPs).

Also the test inputs of tests/test_gpu_fit.py and tests/test_fit_host.py: seeded pairs, half of them with A planted
as a mutated copy of a window of B.
"""
import random

import numpy as np

from bialign_amd import synth
from free_ends_expected import NONE, NONE32, _mutate, cell_seconds, compare_layers, plain_pair, pool_map, run_mask, tables_of  # noqa: F401
from oracle import oracle


def cut_tables(mu1, mu2, j0):
    """The (n+1) x (m-j0+1) tables of A against B[j0:] out of the pair's (n+1) x (m+1) tables (column 0 stays)."""
    cut = lambda t: np.ascontiguousarray(np.concatenate([t[:, :1], t[:, j0 + 1:]], axis=1))
    return cut(mu1), cut(mu2)


def fit_partial(job):
    """Pool worker (spawned: no GPU state).  ``(key, n, m, params, mu1, mu2, lo, hi, want_layers)``: the oracle runs of
    the starts j0 = lo..hi-1 -> ``(key, lo, rows, layers)``: ``rows[j0 - lo, j1]`` the global score of A against
    B[j0:j1] (NONE where j1 < j0), ``layers`` the maximum of these runs' shifted layers as int32 (NONE32 where none of
    them has the cell), or None."""
    key, n, m, params, mu1, mu2, lo, hi, want_layers = job
    s = params["max_shift"]
    nl, w = (9 if params["gap_opening_cost"] != 0 else 1), 2 * s + 1
    rows = np.full((hi - lo, m + 1), NONE, dtype=np.int64)
    layers = np.full((nl, n + 1, m + 1, w, w), NONE32, dtype=np.int32) if want_layers else None
    for j0 in range(lo, hi):
        c1, c2 = cut_tables(mu1, mu2, j0)
        lay = oracle.solve_tables(n, m - j0, params, c1, c2, want_trace=False)["layers"]
        rows[j0 - lo, j0:] = lay[:, n, :, s, s].max(axis=0)
        if want_layers:
            ok = run_mask(n, m - j0, s)[None]
            layers[:, :, j0:] = np.maximum(layers[:, :, j0:], np.where(ok, lay, NONE32))
            if j0 == 0:  # the empty substring B[m:m]: column 0 of any run, which depends on A alone, standing at column m
                col = np.where(run_mask(n, 0, s)[None], lay[:, :, :1], NONE32)
                layers[:, :, m:] = np.maximum(layers[:, :, m:], col)
    return key, lo, rows, layers


def split_jobs(key, n, m, params, mu1, mu2, want_layers=True, seconds=3.0):
    """The jobs of one pair for ``fit_partial``: the starts 0..m-1 cut into ranges of about ``seconds`` of oracle time
    each (a run of start j0 costs about n (m - j0) lattice points)."""
    per_col = n * cell_seconds(params)
    jobs, lo, acc = [], 0, 0.0
    for j0 in range(m):
        acc += per_col * (m - j0)
        if acc >= seconds or j0 == m - 1:
            jobs.append((key, n, m, params, mu1, mu2, lo, j0 + 1, want_layers))
            lo, acc = j0 + 1, 0.0
    return jobs


def fit_combine(n, m, s, parts):
    """The parts of one pair (``fit_partial`` results, any order) -> dict: ``score``; ``end_b`` (the smallest j that
    attains it); ``glob`` int64 [m+1, m+1], ``glob[j0, j1]`` the global score of A against B[j0:j1] (NONE below the
    diagonal; the empty substring's value on it); ``layers`` int64 [NL, n+1, m+1, W, W], the expected FIT layers in the
    reference layout (NONE where no run has the cell), or None."""
    glob = np.full((m + 1, m + 1), NONE, dtype=np.int64)
    layers = None
    for _, lo, rows, lay in parts:
        glob[lo:lo + len(rows)] = rows
        if lay is not None:
            layers = lay.copy() if layers is None else np.maximum(layers, lay)
    glob[m, m] = glob[0, 0]  # B[m:m] is empty like B[0:0]
    if layers is not None:
        layers = np.where(layers == NONE32, NONE, layers.astype(np.int64))
    ends = glob.max(axis=0)  # E(j1), the best start for every end
    score = int(ends.max())
    return dict(score=score, end_b=int(np.argmax(ends == score)), glob=glob, layers=layers)


def fit_expected(n, m, params, mu1, mu2, want_layers=True):
    """One pair, in this process."""
    return fit_combine(n, m, params["max_shift"], [fit_partial(j) for j in split_jobs(0, n, m, params, mu1, mu2, want_layers, 1e9)])


def expected_many(cases, procs=None):
    """``cases``: {key: (n, m, params, mu1, mu2, want_layers)} -> {key: fit_combine's dict}; the oracle runs of all
    cases share one spawn pool."""
    jobs = [j for key, c in cases.items() for j in split_jobs(key, *c)]
    jobs.sort(key=lambda j: -(j[7] - j[6]) * j[1] * (j[2] - j[6]))  # (roughly) the long ones first
    done = pool_map(fit_partial, jobs, procs)
    return {key: fit_combine(c[0], c[1], c[2]["max_shift"], [d for d in done if d[0] == key]) for key, c in cases.items()}


def planted_pair(kind, seed, n, m):
    """A pair whose A is a mutated copy of a window of B well inside B, so that the best substring starts after B's
    first residue and ends before its last.  Protein: B avoids W, Y and F, and (n >= 12) A carries three W at either end
    whose structure letters differ from everything near them -- gapping them is cheaper than aligning them, also where
    n == m.  RNA: B's structure is balanced hairpins, A's hairpins, balanced hairpins."""
    rng = random.Random(seed)
    if kind == "rna":
        if n > m - 2:  # (no room for a window inside B: a plain pair)
            return synth.rna_pair(seed, n, m)
        w = rng.randint(1, m - n - 1)
        seq_b = synth._draw(rng, synth.RNA_ALPHABET, m)
        str_a = synth.dotbracket(rng, n)
        seq_a = _mutate(rng, seq_b[w:w + n], synth.RNA_ALPHABET)
        return seq_a, seq_b, str_a, synth.dotbracket(rng, w) + str_a + synth.dotbracket(rng, m - w - n)
    f = 3 if n >= 12 else 0
    c = min(n - 2 * f, m - 2)
    w = rng.randint(1, m - c - 1)
    alpha_b = "".join(ch for ch in synth.PROTEIN_ALPHABET if ch not in "WYF")
    seq_b = synth._draw(rng, alpha_b, m)
    str_b = synth._draw(rng, "HEC", m)
    seq_a = "W" * f + _mutate(rng, seq_b[w:w + c], alpha_b) + "W" * f + synth._draw(rng, alpha_b, n - c - 2 * f)
    str_a = "T" * f + _mutate(rng, str_b[w:w + c], "HEC") + "T" * f + synth._draw(rng, "HEC", n - c - 2 * f)
    return seq_a[:n], seq_b, str_a[:n], str_b


def make_pair(kind, seed, n, m, planted):
    return planted_pair(kind, seed, n, m) if planted else plain_pair(kind, seed, n, m)
