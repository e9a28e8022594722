"""What the hit search of a FIT batch (include/bialign.h, "Hit search") must give, from the CPU oracle alone.

``fit_expected``'s ``glob[j0, j1]`` is the global score of A against B[j0:j1] for every substring.  Its column maxima are
the profile E.  Which start a walk reaches among the optimal ones is the walk's business (its tie-breaks), so the greedy
loop is not predicted but REPLAYED: ``replay`` follows the engine's walk log step by step on the oracle's profile and
asserts that every step is the one the model prescribes given the steps before it.

Also the inputs with several placements: ``multi_planted_pair``, and ``greedy``, the loop under a chosen start rule, with
which tests/test_fit_hits_host.py states the condition these inputs must meet.
"""
import random

import numpy as np

from bialign_amd import synth
from fit_expected import _mutate, tables_of  # (fit_expected is the base: its glob is what everything here reads)
from free_ends_gpu import params_of

STATUS = ("not_searched", "exhausted", "max_hits", "max_walks")


def resolve(spec):
    """(max_hits, min_score[, max_walks]) as ``Batch.set_hits`` takes it -> (max_hits, max_walks, min_score), 0 resolved."""
    max_hits, min_score = int(spec[0]), int(spec[1])
    max_walks = int(spec[2]) if len(spec) > 2 else 0
    return max_hits, max_walks or 4 * max_hits, min_score


def profile(glob):
    """E(j): the best start for every end."""
    return glob.max(axis=0)


def meets(span, other):
    """Half-open spans [s, e) and [s', e') intersect."""
    return span[0] < other[1] and other[0] < span[1]


def mask_after(masked, start, end, accepted):
    if accepted:
        masked[min(start + 1, end):end + 1] = True
    else:
        masked[end] = True


def next_end(E, masked, min_score):
    """The masked argmax: largest E, then smallest j; None when no candidate is left."""
    cand = np.flatnonzero(~masked & (E >= min_score))
    if not len(cand):
        return None
    return int(cand[np.argmax(E[cand])])  # (argmax: the first of the largest, cand is rising)


def replay(glob, spec, walks, hits, status):
    """Re-run the greedy loop on the oracle's profile along the engine's log.  ``spec``: (max_hits, max_walks, min_score);
    ``walks``: [(end, start, score, accepted)]; ``hits``: [(start, end, score, ...)]; ``status``: one of STATUS."""
    max_hits, max_walks, min_score = spec
    E = profile(glob)
    masked = np.zeros(len(E), dtype=bool)
    accepted = []
    for w, (end, start, score, acc) in enumerate(walks):
        assert len(accepted) < max_hits and w < max_walks, f"walk {w}: made after the search had to stop"
        want = next_end(E, masked, min_score)
        assert want is not None, f"walk {w}: made with no candidate left"
        if end != want:
            assert not masked[end] and E[end] == E[want], f"walk {w}: wrong end {end}, the masked argmax is {want}"
            raise AssertionError(f"walk {w}: wrong tie, end {end} where the smallest best end is {want}")
        assert score == E[end], f"walk {w}: score {score} is not E({end}) = {E[end]}"
        assert 0 <= start <= end and glob[start, end] == E[end], f"walk {w}: start {start} is no optimal start of end {end}"
        disjoint = not any(meets((start, end), a) for a in accepted)
        assert bool(acc) == disjoint, f"walk {w}: wrong acceptance {bool(acc)} of [{start}, {end}) against {accepted}"
        if acc:
            accepted.append((start, end))
        mask_after(masked, start, end, acc)
    if len(accepted) == max_hits:
        want_status = "max_hits"
    elif len(walks) == max_walks:
        want_status = "max_walks"
    else:
        assert next_end(E, masked, min_score) is None, "the search stopped with candidates left"
        want_status = "exhausted"
    assert status == want_status, f"wrong status {status}, the state implies {want_status}"
    assert [(h[0], h[1]) for h in hits] == accepted, "the hit records are not the accepted walks"
    assert [h[2] for h in hits] == [int(E[e]) for _, e in accepted]


def greedy(glob, spec, rule):
    """The loop on the oracle alone, every walk reaching the smallest (``rule=min``) or largest (``rule=max``) optimal
    start of its end -> (hits [(start, end, score)], walks, status)."""
    max_hits, max_walks, min_score = spec
    E = profile(glob)
    masked = np.zeros(len(E), dtype=bool)
    hits, walks = [], []
    while True:
        end = next_end(E, masked, min_score)
        if end is None:
            return hits, walks, "exhausted"
        start = rule(j0 for j0 in range(end + 1) if glob[j0, end] == E[end])
        acc = not any(meets((start, end), h) for h in hits)
        walks.append((end, start, int(E[end]), acc))
        if acc:
            hits.append((start, end, int(E[end])))
        mask_after(masked, start, end, acc)
        if len(hits) == max_hits:
            return hits, walks, "max_hits"
        if len(walks) == max_walks:
            return hits, walks, "max_walks"


def multi_planted_pair(kind, seed, n, m, copies):
    """-> ((seqA, seqB, strA, strB), windows): B is ``copies`` disjoint mutated copies of A between random flanks of at
    least two residues; ``windows`` the copies' starts w_k, so copy k is B[w_k : w_k + n]."""
    rng = random.Random(seed)
    spare = m - copies * n - 2 * (copies + 1)
    assert spare >= 0, "no room for the copies and their flanks"
    cuts = sorted(rng.randint(0, spare) for _ in range(copies))
    flanks = [2 + b - a for a, b in zip([0] + cuts, cuts + [spare])]
    if kind == "rna":
        alpha, struct = synth.RNA_ALPHABET, lambda length: synth.dotbracket(rng, length)
        seq_a, str_a = synth._draw(rng, alpha, n), synth.dotbracket(rng, n)
        copy_str = lambda: str_a
    else:
        alpha, struct = synth.PROTEIN_ALPHABET, lambda length: synth._draw(rng, "HEC", length)
        seq_a, str_a = synth._draw(rng, alpha, n), synth._draw(rng, "HEC", n)
        copy_str = lambda: _mutate(rng, str_a, "HEC")
    seq_b = str_b = ""
    windows = []
    for k in range(copies):
        seq_b += synth._draw(rng, alpha, flanks[k])
        str_b += struct(flanks[k])
        windows.append(len(seq_b))
        seq_b += _mutate(rng, seq_a, alpha)
        str_b += copy_str()
    seq_b += synth._draw(rng, alpha, flanks[copies])
    str_b += struct(flanks[copies])
    assert len(seq_b) == len(str_b) == m
    return (seq_a, seq_b, str_a, str_b), windows


# A 22 against B 150, three copies, max_shift 1, both recurrences.  The seed is the first, counting up from 100, for which
# tests/test_fit_hits_host.py's test_planted_inputs_hold_their_copies passes; nothing of it was tried against the GPU.
PLANTED = dict(kind="protein", seed=100, n=22, m=150, copies=3)
PLANTED_COSTS = ("affine", "one-layer")


def planted_case(cost):
    """-> (pair, windows, params, (n, m, params, mu1, mu2, want_layers)) of one recurrence."""
    pair, windows = multi_planted_pair(**PLANTED)
    params = params_of(PLANTED["kind"], cost, 1)
    return pair, windows, params, (PLANTED["n"], PLANTED["m"], params, *tables_of(pair, params), False)


def planted_spec(glob, windows):
    """(max_hits, max_walks, min_score): min_score the smallest score of a planted window, derived; room for more hits
    than copies and for a walk from every end."""
    n, m = PLANTED["n"], PLANTED["m"]
    return 2 * PLANTED["copies"], m + 1, int(min(glob[w, w + n] for w in windows))
