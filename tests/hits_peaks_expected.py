"""The hit search under the peak rule and per-pair thresholds (include/bialign.h, "Hit search": "Peak candidates",
"Thresholds"), from the CPU oracle alone.  ``replay`` and ``greedy`` are those of tests/hits_expected.py with two changes:
the initial mask is ``~peaks(E)`` when asked, and the candidates are the ends with ``E >= threshold``."""
import numpy as np

from hits_expected import mask_after, meets, next_end, planted_case, profile  # noqa: F401 (planted_case, meets: re-exported)


def peaks(E):
    """bool[m + 1]: end j is a peak when (j = 0 or E(j-1) < E(j)) and (j = m or E(j+1) <= E(j))."""
    E = np.asarray(E, dtype=np.int64)
    rise = np.ones(len(E), dtype=bool)
    rise[1:] = E[:-1] < E[1:]
    hold = np.ones(len(E), dtype=bool)
    hold[:-1] = E[1:] <= E[:-1]
    return rise & hold


_peaks = peaks   # (replay and greedy take a keyword of the function's name)


def threshold(E, base, min_permille=0):
    """T = max(base, Emax > 0 ? ceil(min_permille * Emax / 1000) : 0), in Python integers."""
    emax = int(np.max(E))
    return max(int(base), -(-int(min_permille) * emax // 1000) if emax > 0 else 0)


def initial_mask(E, use_peaks):
    return ~_peaks(E) if use_peaks else np.zeros(len(E), dtype=bool)


def replay(glob, spec, walks, hits, status, peaks=False, threshold=None):
    """``hits_expected.replay`` along the engine's log.  ``spec``: (max_hits, max_walks, min_score); ``peaks``: the peak
    rule is on; ``threshold``: the pair's T_p (None: spec's min_score)."""
    max_hits, max_walks, min_score = spec
    T = min_score if threshold is None else int(threshold)
    E = profile(glob)
    is_peak = _peaks(E)
    masked = initial_mask(E, peaks)
    accepted = []
    for w, (end, start, score, acc) in enumerate(walks):
        assert len(accepted) < max_hits and w < max_walks, f"walk {w}: made after the search had to stop"
        assert E[end] >= T, f"walk {w}: end {end} scores {E[end]}, below the threshold {T}"
        assert not peaks or is_peak[end], f"walk {w}: end {end} is no peak of the profile"
        want = next_end(E, masked, T)
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
        assert next_end(E, masked, T) is None, "the search stopped with candidates left"
        want_status = "exhausted"
    assert status == want_status, f"wrong status {status}, the state implies {want_status}"
    assert [(h[0], h[1]) for h in hits] == accepted, "the hit records are not the accepted walks"
    assert [h[2] for h in hits] == [int(E[e]) for _, e in accepted]


def greedy(glob, spec, rule, peaks=False, threshold=None):
    """``hits_expected.greedy`` under the peak rule and a threshold -> (hits [(start, end, score)], walks, status)."""
    max_hits, max_walks, min_score = spec
    T = min_score if threshold is None else int(threshold)
    E = profile(glob)
    masked = initial_mask(E, peaks)
    hits, walks = [], []
    while True:
        end = next_end(E, masked, T)
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
