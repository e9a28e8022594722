"""Batch front end: many independent (A, B) pairs under one parameter set.

The reference aligns one pair per ``BiAligner`` (reference bialign.py:11); the
engine is batch-first (a single pair is a batch of one).  ``make_batch`` turns
molecule strings into the LOOKUP form the C ABI takes; ``shard`` splits a batch
over the ranks of a one-process-per-GPU job.
"""
import bisect

import numpy as np

from .scoring import ScoreModel


class FlatBatch:
    """A batch's molecules as the C ABI wants them (include/bialign.h, bialign_pairs): one uint8 code array per
    side and kind, pair p's molecule A at ``seq_a[off_a[p] : off_a[p] + len_a[p]]``."""
    __slots__ = ("len_a", "len_b", "off_a", "off_b", "seq_a", "cls_a", "seq_b", "cls_b")

    def molecules(self, side):
        """[(sequence codes, class codes)] per pair -- views, nothing is copied."""
        ln, off = (self.len_a, self.off_a) if side == "a" else (self.len_b, self.off_b)
        seq, cls = (self.seq_a, self.cls_a) if side == "a" else (self.seq_b, self.cls_b)
        return [(seq[o:o + n], cls[o:o + n]) for o, n in zip(off.tolist(), ln.tolist())]


def _offsets(lens):
    off = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    return off


def encode_flat(pairs, params):
    """pairs: iterable of (seqA, seqB, strA, strB) -> (ScoreModel, FlatBatch).  The whole batch is encoded in one
    shot: all molecules of a kind joined into one ``bytes``, one table gather, offsets by cumsum -- no per-molecule
    numpy call (1024 pairs x len 1024: 45 ms -> 4 ms of host time in front of a 50 ms sweep)."""
    pairs = pairs if isinstance(pairs, list) else list(pairs)
    sa, sb, ta, tb = zip(*pairs) if pairs else ((), (), (), ())
    fb = FlatBatch()
    fb.len_a = np.fromiter(map(len, sa), dtype=np.int32, count=len(pairs))
    fb.len_b = np.fromiter(map(len, sb), dtype=np.int32, count=len(pairs))
    if not (np.array_equal(fb.len_a, np.fromiter(map(len, ta), dtype=np.int32, count=len(pairs))) and
            np.array_equal(fb.len_b, np.fromiter(map(len, tb), dtype=np.int32, count=len(pairs)))):
        raise ValueError("Provided structure and sequence must have the same length.")
    fb.off_a, fb.off_b = _offsets(fb.len_a), _offsets(fb.len_b)
    na = int(fb.len_a.sum())
    raw_seq = raw_str = None
    try:  # latin-1: one byte per letter, so byte offsets are letter offsets
        raw_seq = ("".join(sa) + "".join(sb)).encode("latin-1")
        raw_str = ("".join(ta) + "".join(tb)).encode("latin-1")
    except UnicodeEncodeError:
        pass
    if raw_seq is None:
        model = ScoreModel(params, sequences=sa + sb, structures=ta + tb)
        seq = cls = None
    else:
        model = ScoreModel(params, raw_sequences=raw_seq, raw_structures=raw_str)
        seq = model.encode_raw(raw_seq, model.seq_index)
        cls = None if model.is_rna else model.encode_raw(raw_str, model.cls_index)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    if seq is None:  # letters beyond latin-1 or an alphabet without a byte table: molecule by molecule
        seq = cat([model.encode_sequence(x) for x in sa + sb])
    if cls is None:  # RNA: classes come from the bracket structure (a stack per molecule); or the slow alphabet path
        cls = cat([model.encode_structure(x) for x in ta + tb])
    fb.seq_a, fb.seq_b = seq[:na], seq[na:]   # (contiguous slices of the two joined arrays)
    fb.cls_a, fb.cls_b = cls[:na], cls[na:]
    return model, fb


def encode_pairs(pairs, params):
    """pairs: iterable of (seqA, seqB, strA, strB) -> (model, mols_a, mols_b), the molecules as
    (sequence codes, class codes) per pair (views into the flat arrays of ``encode_flat``)."""
    model, fb = encode_flat(pairs, params)
    return model, fb.molecules("a"), fb.molecules("b")


def make_batch(pairs, params, engine=None, hbm_budget_bytes=0, recurrence=0, mu2_dense=None,
               score_only=False, lean_trace=False, mu1_dense=None, level_trace=False, null_dense=None, fit=False,
               local=False, overlap=False, hits=None):
    """``fit``: fit alignments, A inside a longer B with B's end gaps free (engine.Batch).
    ``hits``: ``(max_hits, min_score)`` or ``(max_hits, min_score, max_walks)``, or a dict of ``Batch.set_hits``'s keywords
    (``peaks``, ``min_scores``, ``min_permille`` among them), a shorthand for ``Batch.set_hits`` on a ``fit`` batch in full
    storage: every run also searches each pair for its disjoint placements of A in B.
    ``local``: local alignments, the best-scoring parts of A and B with the ends of both free (engine.Batch).
    ``overlap``: overlap alignments, the global alignment with the end gaps of both molecules free (engine.Batch).
    ``mu1_dense`` / ``mu2_dense``: optional lists of one (len A, len B) int table per pair (engine.Batch).
    ``level_trace``: full results from checkpointed levels, for bands beyond the tiled kernels (engine.Batch).
    ``null_dense``: ``(replicas, seed)``, a null batch of these pairs with their dense tables
    (``significance.null_dense_batch``): score-only, no ``lean_trace`` / ``level_trace``."""
    _check_storage(score_only, lean_trace, level_trace)
    if hits is not None:
        pairs = pairs if isinstance(pairs, list) else list(pairs)
        hits = check_hits_arg(hits, fit, score_only, null_dense, len(pairs))
    if null_dense is not None:
        from .significance import check_dense_args
        if lean_trace or level_trace:
            raise ValueError("a null batch is score-only: lean_trace / level_trace do not apply")
        pairs, replicas, seed = check_dense_args(pairs, null_dense, mu1_dense, mu2_dense)
        null_dense = (replicas, seed)
    from .engine import Batch, default_engine  # loads the HIP library (no CPU fallback)
    model, fb = encode_flat(pairs, params)
    b = Batch(engine or default_engine(), fb, None, model.s1, model.s2,
              params["gap_opening_cost"], params["gap_cost"], params["shift_cost"],
              params["max_shift"], hbm_budget_bytes=hbm_budget_bytes, recurrence=recurrence,
              mu2_dense=mu2_dense, score_only=score_only, lean_trace=lean_trace, mu1_dense=mu1_dense,
              level_trace=level_trace, fit=fit, local=local, overlap=overlap, **({} if null_dense is None else dict(null_dense=null_dense)))
    if isinstance(hits, dict):
        b.set_hits(**hits)
    elif hits is not None:
        b.set_hits(*hits)
    return b


def check_hit_spec(max_hits, min_score, max_walks=0):
    """The hit search's parameters as include/bialign.h states them -> ints; ValueError before the library is called."""
    try:
        max_hits, min_score, max_walks = int(max_hits), int(min_score), int(max_walks)
    except (TypeError, ValueError):
        raise ValueError("max_hits, min_score and max_walks must be integers") from None
    if not 1 <= max_hits <= 256:
        raise ValueError(f"max_hits must be 1..256, got {max_hits}")
    if min_score < 1:
        raise ValueError(f"min_score must be >= 1, got {min_score}")
    if max_walks != 0 and max_walks < max_hits:
        raise ValueError(f"max_walks must be 0 (4 * max_hits) or >= max_hits, got {max_walks}")
    return max_hits, min_score, max_walks


HIT_KEYWORDS = ("max_hits", "min_score", "max_walks", "peaks", "min_scores", "min_permille")


def check_hit_rules(peaks=False, min_scores=None, min_permille=0, npairs=None):
    """The peak rule and the thresholds of a hit search as include/bialign.h states them -> ``(peaks, min_scores,
    min_permille)``, ``min_scores`` an int32 array or None; ValueError before the library is called.  ``npairs`` given:
    ``min_scores`` must have that many entries."""
    if not isinstance(peaks, (bool, np.bool_)):
        raise ValueError(f"peaks must be a bool, got {peaks!r}")
    if isinstance(min_permille, (bool, np.bool_)) or not isinstance(min_permille, (int, np.integer)):
        raise ValueError(f"min_permille must be an int in 0..1000, got {min_permille!r}")
    if not 0 <= min_permille <= 1000:
        raise ValueError(f"min_permille must be an int in 0..1000, got {min_permille}")
    if min_scores is not None:
        try:
            arr = np.asarray(list(min_scores))
        except TypeError:
            raise ValueError("min_scores must be one int >= 1 per pair") from None
        if arr.ndim != 1 or (arr.size and not np.issubdtype(arr.dtype, np.integer)) or arr.dtype == np.bool_:
            raise ValueError("min_scores must be one int >= 1 per pair")
        if npairs is not None and arr.size != npairs:
            raise ValueError(f"min_scores must be one int >= 1 per pair: {arr.size} entries for {npairs} pairs")
        if arr.size and (arr.min() < 1 or arr.max() > 0x7fffffff):
            raise ValueError(f"min_scores must be one int >= 1 per pair (below 2^31), got {int(arr.min())}..{int(arr.max())}")
        min_scores = np.ascontiguousarray(arr, dtype=np.int32)
    return bool(peaks), min_scores, int(min_permille)


def check_hits_arg(hits, fit, score_only, null=None, npairs=None):
    """``hits=`` of ``make_batch`` -> ``(max_hits, min_score, max_walks)``, or for a dict of ``Batch.set_hits``'s keywords
    the checked dict: the search needs a fit batch in full storage."""
    if not fit:
        raise ValueError("hits= needs fit=True: the hit search walks the placements of A in B of a fit batch")
    if score_only or null is not None:
        raise ValueError("hits= excludes score_only and null batches: the hit search walks through the full layers")
    if isinstance(hits, dict):
        unknown = sorted(set(hits) - set(HIT_KEYWORDS))
        if unknown or "max_hits" not in hits or "min_score" not in hits:
            raise ValueError(f"hits as a dict takes max_hits, min_score and any of {', '.join(HIT_KEYWORDS[2:])}"
                             + (f"; not {', '.join(map(str, unknown))}" if unknown else ""))
        max_hits, min_score, max_walks = check_hit_spec(hits["max_hits"], hits["min_score"], hits.get("max_walks", 0))
        peaks, min_scores, min_permille = check_hit_rules(hits.get("peaks", False), hits.get("min_scores"),
                                                            hits.get("min_permille", 0), npairs)
        return dict(max_hits=max_hits, min_score=min_score, max_walks=max_walks, peaks=peaks, min_scores=min_scores,
                    min_permille=min_permille)
    try:
        hits = tuple(hits)
    except TypeError:
        raise ValueError("hits must be (max_hits, min_score) or (max_hits, min_score, max_walks)") from None
    if len(hits) not in (2, 3):
        raise ValueError("hits must be (max_hits, min_score) or (max_hits, min_score, max_walks)")
    return check_hit_spec(*hits)


def _check_storage(score_only, lean_trace, level_trace):
    """The storage modes that exclude each other, refused before the library is loaded or called."""
    if level_trace and (score_only or lean_trace):
        raise ValueError("level_trace excludes score_only and lean_trace")


def make_feature_batch(molecules, pair_index, params, engine=None, hbm_budget_bytes=0, recurrence=0,
                       score_only=False, lean_trace=False, mu1_dense=None, level_trace=False, null=None, fit=False,
                       local=False, overlap=False):
    """Batch with mu2 in FEATURE form (include/bialign.h, bialign_features): RNA molecules with real-valued
    structure features, e.g. from predicted base-pair probabilities.  ``molecules``: a list of
    ``(seq, (up, down, unp))``, three numbers per residue as ``scoring.rna_features`` makes them; ``pair_index``: a
    list of ``(ia, ib)`` into it.  Every molecule is encoded, checked and uploaded once and the pairs point into it,
    so an all-against-all batch costs O(sum of lengths) on the host; the GPU builds each chunk's score tables.
    The structure weight is ``params["structure_weight"]``.  Bad arguments raise ValueError before the library is
    called: an index outside ``molecules``, ragged or mis-sized feature arrays, a NaN or infinite feature, and
    ValueError("math domain error") for a negative one.
    ``null``: ``(replicas, seed)``, a FEATURE-form null batch (``significance.null_feature_batch``): every pair against
    ``replicas`` shuffles of its B molecule, a residue's three numbers moving with its letter; score-only, mu1 in
    LOOKUP form.
    ``fit``: fit alignments, A inside a longer B with B's end gaps free (engine.Batch).
    ``local``: local alignments, the best-scoring parts of A and B with the ends of both free (engine.Batch).
    ``overlap``: overlap alignments, the global alignment with the end gaps of both molecules free (engine.Batch)."""
    from .scoring import check_features
    _check_storage(score_only, lean_trace, level_trace)
    if null is not None:
        from .significance import check_null
        null = check_null(null)
        if lean_trace or level_trace or mu1_dense is not None:
            raise ValueError("a null batch is score-only and takes mu1 in LOOKUP form: no lean_trace / level_trace / mu1_dense")
    molecules = list(molecules)
    pair_index = [(int(ia), int(ib)) for ia, ib in pair_index]
    if not molecules or not pair_index:
        raise ValueError("need at least one molecule and one pair")
    for p, (ia, ib) in enumerate(pair_index):
        if not (0 <= ia < len(molecules) and 0 <= ib < len(molecules)):
            raise ValueError(f"pair {p}: molecule index ({ia}, {ib}) out of range (0..{len(molecules) - 1})")
    seqs = [str(seq) for seq, _ in molecules]
    feats = [check_features(f, len(seq), f"molecule {t}") for t, (seq, (_, f)) in enumerate(zip(seqs, molecules))]
    model = ScoreModel(params, sequences=seqs, structures=["."])
    lens = np.fromiter(map(len, seqs), dtype=np.int32, count=len(seqs))
    offs = _offsets(lens)
    ia, ib = (np.fromiter(x, dtype=np.int64, count=len(pair_index)) for x in zip(*pair_index))
    fb = FlatBatch()
    fb.len_a, fb.len_b = np.ascontiguousarray(lens[ia]), np.ascontiguousarray(lens[ib])
    fb.off_a, fb.off_b = np.ascontiguousarray(offs[ia]), np.ascontiguousarray(offs[ib])
    codes = [model.encode_sequence(x) for x in seqs]
    fb.seq_a = fb.seq_b = np.ascontiguousarray(np.concatenate(codes))
    fb.cls_a = fb.cls_b = np.zeros(len(fb.seq_a), dtype=np.uint8)  # (unused: the FEATURE form replaces the classes)
    flat = tuple(np.ascontiguousarray(np.concatenate([f[x] for f in feats])) for x in range(3))
    from .engine import Batch, default_engine  # loads the HIP library (no CPU fallback)
    return Batch(engine or default_engine(), fb, None, model.s1, model.s2,
                 params["gap_opening_cost"], params["gap_cost"], params["shift_cost"],
                 params["max_shift"], hbm_budget_bytes=hbm_budget_bytes, recurrence=recurrence,
                 score_only=score_only, lean_trace=lean_trace, mu1_dense=mu1_dense, level_trace=level_trace,
                 mu2_features=(int(params["structure_weight"]), flat, flat), null=null, fit=fit, local=local, overlap=overlap)


def shard(npairs, rank, world_size, costs=None):
    """Contiguous block of pair indices owned by ``rank`` (pairs are independent, so sharding
    needs no data-path collective).  Without ``costs`` the blocks hold equal numbers of pairs;
    with ``costs`` (one non-negative number per pair, e.g. lattice cells) block r ends where the
    running cost first reaches (r+1)/world of the total -- every rank computes the same cuts."""
    if costs is None:
        base, extra = divmod(npairs, world_size)
        start = rank * base + min(rank, extra)
        return range(start, start + base + (1 if rank < extra else 0))
    if len(costs) != npairs:
        raise ValueError("costs needs one entry per pair")
    return _cost_cuts(costs, world_size)[rank]


def _cost_cuts(costs, world_size):
    """world_size contiguous ranges; cut r sits where the running cost is nearest to
    (r+1)/world of the total (integer arithmetic, ties to the earlier cut)."""
    running = [0]
    for c in costs:
        if c < 0:
            raise ValueError("costs must be non-negative")
        running.append(running[-1] + int(c))
    total, n = running[-1], len(costs)
    cuts, start = [], 0
    for r in range(world_size):
        if r == world_size - 1:
            stop = n
        else:
            target = total * (r + 1)                      # compare running[x] * world with it
            stop = bisect.bisect_left(running, -(-target // world_size), lo=start)  # first reach
            stop = min(stop, n)
            if stop > start and 2 * target - (running[stop - 1] + running[stop]) * world_size <= 0:
                stop -= 1                                 # the cut before is at least as near
        cuts.append(range(start, stop))
        start = stop
    return cuts


def pair_cost(pair, max_shift):
    """Lattice cells of one (seqA, seqB, ...) pair: K(n,s) * K(m,s)."""
    s = int(max_shift)
    k = lambda x: (x + 1) * (2 * s + 1) - s * (s + 1)
    return k(len(pair[0])) * k(len(pair[1]))
