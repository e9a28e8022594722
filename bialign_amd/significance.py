"""Shuffled-null significance: z-scores of optimal scores against shuffles of molecule B made on the GPU.

A raw bi-alignment score grows with both lengths and with composition, so the scores of a long and a short pair do not
compare.  The standard remedy for pairwise aligners is a shuffled null: align A against R random shuffles of B and
report where the real score lies in that distribution.  A *null batch* (include/bialign.h, bialign_batch_create_null)
runs those npairs x R alignments as one score-only batch; B is uploaded once, the GPU writes the shuffles and reduces
every pair's R scores to exact integer sums, and ``zscores`` forms mean, standard deviation and z from them here.

RNA molecules with real-valued structure features (``batch.make_feature_batch``) have the same in FEATURE form:
``null_feature_batch`` / ``zscores_features`` (bialign_batch_create_null_features), a residue's three numbers moving
with its letter.  Pairs scored through dense tables -- a PSSM or profile as ``mu1_dense``, structure scores computed
outside as ``mu2_dense`` -- have it in DENSE form: ``null_dense_batch`` / ``zscores_dense``
(bialign_batch_create_null_dense), a residue of B carrying its column of every table.

``permutation``, ``shuffle_b``, ``shuffle_features`` and ``shuffle_tables`` restate the header's permutation in plain Python: the
documented way to reproduce any replica on the host.  ``shuffle="dinucleotide"`` on any of the functions below takes the
header's second null model, which keeps the count of every ordered pair of neighbouring letters of B
(``dinucleotide_permutation`` restates it); the default ``"mono"`` keeps single-letter composition only.  Nothing in this module loads the HIP library before its
arguments are checked.
"""
import numpy as np

MAX_REPLICAS = 65535  # bialign_null_spec.replicas: 1..65535
_M32 = 0xFFFFFFFF


def _mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def permutation(seed, pair, replica, m):
    """The permutation of 0..m-1 that replica ``replica`` of pair ``pair`` (its index in the batch) applies to a B
    molecule of length m under ``seed``: ``shuffled[x] = original[perm[x]]`` (include/bialign.h, THE PERMUTATION)."""
    seed, pair, replica, m = int(seed), int(pair), int(replica), int(m)
    if not 0 <= seed <= _M32:
        raise ValueError("seed must be in 0..2**32-1")
    if pair < 0 or replica < 0 or m < 1:
        raise ValueError("pair and replica must be >= 0, m >= 1")
    h = _mix((_mix((_mix(seed ^ 0x9E3779B9) + pair) & _M32) + replica) & _M32)
    perm = list(range(m))
    for t in range(m - 1, 0, -1):
        j = (_mix((h + t) & _M32) * (t + 1)) >> 32
        perm[t], perm[j] = perm[j], perm[t]
    return np.array(perm, dtype=np.int64)


SHUFFLES = ("mono", "dinucleotide")  # BIALIGN_NULL_MONO, BIALIGN_NULL_DINUCLEOTIDE
TREE_CAP = 4096  # CAP of THE DINUCLEOTIDE PERMUTATION: draws of step 2 per replica


def check_shuffle(shuffle):
    """``shuffle=`` of the functions below -> the model's number in the C ABI; anything but the two names: ValueError."""
    if not isinstance(shuffle, str) or shuffle not in SHUFFLES:
        raise ValueError(f"shuffle must be one of {SHUFFLES}, got {shuffle!r}")
    return SHUFFLES.index(shuffle)


def dinucleotide_permutation(seed, pair, replica, letters, tree_cap=TREE_CAP):
    """The permutation that replica ``replica`` of pair ``pair`` applies to a B molecule whose letters are ``letters``
    (a str or any sequence of hashable items) under ``seed`` in the dinucleotide model: ``shuffled[x] =
    original[perm[x]]`` has exactly the original's count of every ordered pair of neighbouring letters
    (include/bialign.h, THE DINUCLEOTIDE PERMUTATION).  ``tree_cap``: CAP, 0..4096."""
    return _dinucleotide(seed, pair, replica, letters, tree_cap)[0]


def _dinucleotide(seed, pair, replica, letters, tree_cap=TREE_CAP):
    """``dinucleotide_permutation`` -> (perm, draws of step 2, whether step 2 gave up); the comments name the header's steps."""
    seed, pair, replica, cap = int(seed), int(pair), int(replica), int(tree_cap)
    if not 0 <= seed <= _M32:
        raise ValueError("seed must be in 0..2**32-1")
    if pair < 0 or replica < 0 or len(letters) < 1:
        raise ValueError("pair and replica must be >= 0, letters must hold at least one")
    if not 0 <= cap <= TREE_CAP:
        raise ValueError(f"tree_cap must be in 0..{TREE_CAP}")
    h = _mix((_mix((_mix(seed ^ 0x9E3779B9) + pair) & _M32) + replica) & _M32)

    def uni(salt, bound):
        return (_mix((h + salt) & _M32) * bound) >> 32

    number = {}
    B = [number.setdefault(c, len(number)) for c in letters]  # letters renumbered by first occurrence
    m, K = len(B), len(number)
    if m <= 2:
        return np.arange(m, dtype=np.int64), 0, False
    # 1. edges
    cnt = [0] * K
    for e in range(m - 1):
        cnt[B[e]] += 1
    off = [sum(cnt[:x]) for x in range(K)]
    L = sorted(range(m - 1), key=lambda e: (B[e], e))
    z = B[m - 1]
    # 2. last exits
    tree, last, s, gave_up = {z}, [0] * K, 0, False
    for x in range(K):
        if cnt[x] == 0 or x in tree or gave_up:
            continue
        u = x
        while u not in tree:
            if s == cap:
                gave_up = True
                break
            last[u] = uni(0x80000000 + s, cnt[u])
            s += 1
            u = B[L[off[u] + last[u]] + 1]
        if not gave_up:
            u = x
            while u not in tree:
                tree.add(u)
                u = B[L[off[u] + last[u]] + 1]
    if gave_up:
        last = [cnt[x] - 1 for x in range(K)]
    # 3. order of exits
    for x in range(K):
        if cnt[x] == 0:
            continue
        o, r = off[x], cnt[x]
        if x != z:
            L[o:o + r] = L[o:o + last[x]] + L[o + last[x] + 1:o + r] + [L[o + last[x]]]
            r -= 1
        for t in range(r - 1, 0, -1):
            j = uni(o + t, t + 1)
            L[o + t], L[o + j] = L[o + j], L[o + t]
    # 4. walk
    perm, cur, ptr = [0] * m, B[0], [0] * K
    for pos in range(1, m):
        e = L[off[cur] + ptr[cur]]
        ptr[cur] += 1
        perm[pos] = e + 1
        cur = B[e + 1]
    return np.array(perm, dtype=np.int64), s, gave_up


def _perm(shuffle, seed, pair, replica, letters):
    """The permutation of a B molecule with these letters under either model."""
    if check_shuffle(shuffle):
        return dinucleotide_permutation(seed, pair, replica, letters)
    return permutation(seed, pair, replica, len(letters))


#: RNA: the letter a position's structure class is written with in a shuffled molecule (scoring.RNA_UNP, _DOWN, _UP)
_RNA_CLASS_LETTERS = ".()"


def shuffle_b(pair_tuple, seed, pair, replica, rna=False, shuffle="mono"):
    """``(seqA, seqB, strA, strB)`` -> the same with molecule B as replica ``replica`` of pair ``pair`` has it: the
    residues of B permuted, each with its structure annotation.  Proteins: the structure letter moves with the residue.
    ``rna=True``: what moves is the position's structure *class* (unpaired, pairs to the right, pairs to the left --
    ``scoring.rna_classes``), written ``.``, ``(``, ``)``; such a string lists classes per position and is in general
    no balanced dot-bracket structure.  ``shuffle="dinucleotide"``: the dinucleotide model, its letters B's sequence
    string (the structure letters travel with their positions and are no part of the letter)."""
    seq_a, seq_b, str_a, str_b = pair_tuple
    if len(seq_b) != len(str_b):
        raise ValueError("Provided structure and sequence must have the same length.")
    perm = _perm(shuffle, seed, pair, replica, seq_b).tolist()
    if rna:
        from .scoring import rna_classes
        str_b = "".join(_RNA_CLASS_LETTERS[c] for c in rna_classes(str_b).tolist())
    return seq_a, "".join(seq_b[x] for x in perm), str_a, "".join(str_b[x] for x in perm)


def shuffle_features(seq, feats, seed, pair, replica, shuffle="mono"):
    """``(seq, (up, down, unp))`` of a B molecule as replica ``replica`` of pair ``pair`` has it in a FEATURE-form null
    batch: a plain gather through ``permutation`` -- the letter and its three numbers land at the same index, and the
    numbers are moved, not recomputed (float64, bit for bit the source's).  -> ``(str, (up, down, unp))``.
    ``shuffle="dinucleotide"``: through ``dinucleotide_permutation`` of ``seq``."""
    check_shuffle(shuffle)
    seq = str(seq)
    try:
        up, down, unp = feats
    except (TypeError, ValueError):
        raise ValueError("features must be a triple (up, down, unp)") from None
    planes = tuple(np.asarray(f, dtype=np.float64) for f in (up, down, unp))
    if any(f.shape != (len(seq),) for f in planes):
        raise ValueError("every feature must hold one number per residue")
    perm = _perm(shuffle, seed, pair, replica, seq)
    return "".join(seq[x] for x in perm.tolist()), tuple(np.ascontiguousarray(f[perm]) for f in planes)


def shuffle_tables(table, seed, pair, replica, shuffle="mono", letters=None):
    """A pair's (len A, len B) table -- dense mu1 or mu2 -- as replica ``replica`` of pair ``pair`` has it in a
    DENSE-form null batch: ``table[:, permutation(seed, pair, replica, len B)]``, the columns moved with B's residues, the
    values untouched.  ``shuffle="dinucleotide"`` needs ``letters``, B's sequence: a table has no letters of its own."""
    dinucleotide = check_shuffle(shuffle)
    table = np.asarray(table)
    if table.ndim != 2 or table.shape[1] < 1:
        raise ValueError("table must have shape (len A, len B)")
    if dinucleotide and (letters is None or len(letters) != table.shape[1]):
        raise ValueError('shuffle="dinucleotide" needs letters=, B\'s sequence, one letter per column')
    return np.ascontiguousarray(table[:, _perm(shuffle, seed, pair, replica, letters if dinucleotide else range(table.shape[1]))])


def check_dense_tables(tables, lens_a, lens_b, name):
    """One integer table of shape (len A, len B) per pair, every value an int32 -- refused otherwise, where
    ``engine.Batch`` alone would cast."""
    if len(tables) != len(lens_a):
        raise ValueError(f"{name} needs one table per pair")
    for p, tab in enumerate(tables):
        try:
            tab = np.asarray(tab)
        except ValueError:
            raise ValueError(f"{name}[{p}] is ragged: it must have shape (len A, len B)") from None
        if tab.shape != (int(lens_a[p]), int(lens_b[p])):
            raise ValueError(f"{name}[{p}] must have shape (len A, len B) = ({int(lens_a[p])}, {int(lens_b[p])}), "
                             f"got {tab.shape}")
        if tab.dtype == np.bool_ or not np.issubdtype(tab.dtype, np.integer):
            raise ValueError(f"{name}[{p}] must be of an integer dtype, got {tab.dtype}")
        if tab.size and (int(tab.min()) < -2 ** 31 or int(tab.max()) > 2 ** 31 - 1):
            raise ValueError(f"{name}[{p}] holds values outside int32")


def check_dense_args(pairs, null, mu1_dense, mu2_dense):
    """The arguments of a DENSE-form null batch, checked as ``engine.Batch`` and the C ABI check them -- here, so that
    nothing is loaded for a call that cannot succeed.  -> (pairs, replicas, seed)."""
    replicas, seed = check_null(null)
    pairs, replicas, seed = _check_pairs(pairs, replicas, seed)
    if mu1_dense is None and mu2_dense is None:
        raise ValueError("a DENSE-form null batch needs mu1_dense and / or mu2_dense (the LOOKUP form is null_batch / zscores)")
    lens_a, lens_b = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    for tables, name in ((mu1_dense, "mu1_dense"), (mu2_dense, "mu2_dense")):
        if tables is not None:
            check_dense_tables(tables, lens_a, lens_b, name)
    return pairs, replicas, seed


def check_null(null):
    """``(replicas, seed)`` of a null batch -> two ints, refused as the C ABI refuses them (before it is called)."""
    try:
        replicas, seed = null
    except (TypeError, ValueError):
        raise ValueError("null must be (replicas, seed)") from None
    if isinstance(replicas, bool) or int(replicas) != replicas or not 1 <= int(replicas) <= MAX_REPLICAS:
        raise ValueError(f"replicas must be an integer in 1..{MAX_REPLICAS}, got {replicas!r}")
    if int(seed) != seed or not 0 <= int(seed) <= _M32:
        raise ValueError(f"seed must be an integer in 0..2**32-1, got {seed!r}")
    return int(replicas), int(seed)


def _check_mode(fit, local, overlap=False):
    """``fit``, ``local`` and ``overlap`` name three alignment modes: one batch has one of them."""
    if fit and local:
        raise ValueError("fit= and local= exclude each other")
    if overlap and (fit or local):
        raise ValueError("overlap= excludes fit= and local=")


def _check_pairs(pairs, replicas, seed):
    pairs = pairs if isinstance(pairs, list) else list(pairs)
    replicas, seed = check_null((replicas, seed))
    if not pairs:
        raise ValueError("need at least one pair")
    if len(pairs) * replicas > 2 ** 31 - 1:
        raise ValueError("npairs * replicas exceeds INT32_MAX")
    return pairs, replicas, seed


def null_batch(pairs, params, replicas, seed=0, engine=None, hbm_budget_bytes=0, recurrence=0, fit=False, local=False, overlap=False,
               shuffle="mono"):
    """A null batch of ``pairs`` (``(seqA, seqB, strA, strB)`` each, as ``batch.make_batch`` takes them): every pair
    against ``replicas`` shuffles of its B.  -> ``engine.Batch``; ``run()`` it, then ``null_scores()`` /
    ``null_stats()``.  ``fit``: the replicas are scored as fit alignments (engine.Batch) -- the mode the observed
    scores they are compared with must have been scored in.  ``local``: likewise, as local alignments; excludes ``fit``.
    ``overlap``: likewise, as overlap alignments; excludes both.  ``shuffle``: the null model, ``"mono"`` (THE
    PERMUTATION) or ``"dinucleotide"`` (THE DINUCLEOTIDE PERMUTATION; ``Batch.set_null_model``)."""
    null_model = check_shuffle(shuffle)
    _check_mode(fit, local, overlap)
    pairs, replicas, seed = _check_pairs(pairs, replicas, seed)
    from .batch import encode_flat
    from .engine import Batch, default_engine  # loads the HIP library (no CPU fallback)
    model, fb = encode_flat(pairs, params)
    return _with_model(Batch(engine or default_engine(), fb, None, model.s1, model.s2,
                             params["gap_opening_cost"], params["gap_cost"], params["shift_cost"], params["max_shift"],
                             hbm_budget_bytes=hbm_budget_bytes, recurrence=recurrence, null=(replicas, seed), fit=fit, local=local,
                             overlap=overlap), null_model)


def _with_model(batch, null_model):
    """A fresh null batch under the null model of that number (a batch that is refused the model is closed)."""
    if null_model:
        try:
            batch.set_null_model(null_model)
        except Exception:
            batch.close()
            raise
    return batch


def _null_moments(stats, p):
    """Pair p of ``Batch.null_stats``'s exact integers -> (mean, std, defined): the sample standard deviation (ddof = 1,
    nan where R is 1) and whether a z-score is defined (R > 1 and a variance above 0).  The variance's numerator
    R * sumsq - sum^2 is formed in Python integers, so the same integers always give the same doubles."""
    R, s1, s2 = int(stats["replicas"][p]), int(stats["sum"][p]), int(stats["sumsq"][p])
    num = R * s2 - s1 * s1  # = R * (R - 1) * variance, exact
    if num < 0:
        raise ValueError(f"pair {p}: sums are inconsistent (R * sumsq < sum^2)")
    std = (num / (R * (R - 1))) ** 0.5 if R > 1 else float("nan")
    return s1 / R, std, R > 1 and num > 0


def zscores_from_stats(score, stats):
    """Observed scores and the exact integer reductions of ``Batch.null_stats`` -> dict of arrays ``score``, ``mean``,
    ``std`` (sample standard deviation, ddof = 1), ``z`` (nan where std is 0 or R is 1), ``p_emp`` =
    (n_ge + 1) / (R + 1), ``n_ge``, ``replicas``.  The variance's numerator R * sumsq - sum^2 is formed in Python
    integers, so the same integers always give the same doubles."""
    score = np.asarray(score, dtype=np.int64)
    n = len(score)
    mean, std, z = np.empty(n), np.empty(n), np.empty(n)
    for p in range(n):
        mean[p], std[p], defined = _null_moments(stats, p)
        z[p] = (int(score[p]) - mean[p]) / std[p] if defined else float("nan")
    n_ge = np.asarray(stats["n_ge"], dtype=np.int64)
    reps = np.asarray(stats["replicas"], dtype=np.int64)
    return dict(score=score, mean=mean, std=std, z=z, p_emp=(n_ge + 1) / (reps + 1), n_ge=n_ge, replicas=reps)


def hit_zscores(hits, stats):
    """The hits of ``Batch.fit_hits()`` (per pair a list of ``(start_b, end_b, score, ...)``) and the exact integer
    reductions ``null_stats()`` of a FIT null batch of the same pairs -> per pair a float array, per hit
    ``z = (score - mean) / std`` in the arithmetic of ``zscores_from_stats`` (nan where std is 0 or R is 1).
    What the null is: a replica's score is the best placement of A in a shuffled B, the maximum over every end.  That is
    the null of hit 0, the pair's own fit score.  A hit beyond the first is not a maximum over all of B but is held to the
    same null, so its z is conservative: it understates the hit's significance, never overstates it."""
    if len(hits) != len(stats["replicas"]):
        raise ValueError("hits and stats need one entry per pair")
    out = []
    for p, found in enumerate(hits):
        mean, std, defined = _null_moments(stats, p)
        out.append(np.array([(int(h[2]) - mean) / std if defined else float("nan") for h in found], dtype=np.float64))
    return out


def hit_significance(batch, pairs, params, replicas=100, seed=0, shuffle="mono", engine=None, hbm_budget_bytes=0):
    """``hit_zscores`` for a hits batch that has run (``make_batch(pairs, params, fit=True, hits=...)``): makes the null
    batch of ``pairs`` with ``fit=True``, runs it once, and reduces it once per hit rank with that rank's scores as
    ``null_stats(observed=)``.  -> per pair a list with one dict per hit: ``score``, ``z``, ``mean``, ``std``, ``n_ge``,
    ``replicas`` and ``p_emp = (n_ge + 1) / (R + 1)``.  The null is the best placement of A in a shuffled B, conservative
    for hits beyond the first (``hit_zscores``).  The replicas are scored in the hits batch's recurrence (``batch.affine``)."""
    from . import _lib
    hits, _ = batch.fit_hits()
    if len(hits) != len(pairs):
        raise ValueError("pairs must be the pairs of the hits batch")
    ranks = max((len(h) for h in hits), default=0)
    nb = null_batch(pairs, params, replicas, seed=seed, engine=engine, hbm_budget_bytes=hbm_budget_bytes,
                    recurrence=_lib.REC_AFFINE if batch.affine else _lib.REC_LINEAR, fit=True, shuffle=shuffle)

    def per_rank(nb):
        # (a pair without a hit of this rank is reduced against INT32_MAX and its n_ge dropped)
        return [nb.null_stats(np.array([h[r][2] if r < len(h) else 2 ** 31 - 1 for h in hits], dtype=np.int32))
                for r in range(max(ranks, 1))]
    stats = _run_and_close(nb, per_rank)
    z = hit_zscores(hits, stats[0])
    out = []
    for p, found in enumerate(hits):
        mean, std, _ = _null_moments(stats[0], p)
        R = int(stats[0]["replicas"][p])
        out.append([dict(score=int(h[2]), z=float(z[p][r]), mean=mean, std=std, n_ge=int(stats[r]["n_ge"][p]), replicas=R,
                         p_emp=(int(stats[r]["n_ge"][p]) + 1) / (R + 1)) for r, h in enumerate(found)])
    return out


def _run_and_close(batch, result):
    try:
        batch.run()
        return result(batch)
    finally:
        batch.close()


def _zscores(npairs, observed, score_batch, null_batch):
    """What the three ``zscores*`` share once their arguments are checked: the observed scores (the caller's, or those
    of the score-only batch ``score_batch()`` makes), the null batch ``null_batch()`` makes, its reductions, the z-scores."""
    if observed is not None:
        observed = np.ascontiguousarray(observed, dtype=np.int32)
        if observed.shape != (npairs,):
            raise ValueError("observed needs one score per pair")
    else:
        observed = _run_and_close(score_batch(), lambda b: b.scores().copy())
    return zscores_from_stats(observed, _run_and_close(null_batch(), lambda nb: nb.null_stats(observed)))


def zscores(pairs, params, replicas=100, seed=0, observed=None, engine=None, hbm_budget_bytes=0, recurrence=0, fit=False, local=False, overlap=False,
            shuffle="mono"):
    """z-scores of the pairs' optimal scores against ``replicas`` shuffles of each pair's B (``zscores_from_stats``).
    ``observed``: the pairs' real scores if the caller has them; else a score-only batch computes them first.
    ``fit``: fit alignments (engine.Batch) -- observed scores and replicas alike (``observed``, if given, must be fit
    scores then).  ``local``: likewise, local alignments; excludes ``fit``.  ``overlap``: likewise, overlap alignments; excludes both.
    ``shuffle``: the null model of the replicas, as for ``null_batch``; the observed scores do not depend on it."""
    check_shuffle(shuffle)
    _check_mode(fit, local, overlap)
    pairs, replicas, seed = _check_pairs(pairs, replicas, seed)
    common = dict(engine=engine, hbm_budget_bytes=hbm_budget_bytes, recurrence=recurrence, fit=fit, local=local, overlap=overlap)

    def score_batch():
        from .batch import make_batch
        return make_batch(pairs, params, score_only=True, **common)
    return _zscores(len(pairs), observed, score_batch, lambda: null_batch(pairs, params, replicas, seed=seed, shuffle=shuffle, **common))


def _check_feature_args(molecules, pair_index, replicas, seed):
    """The arguments of a FEATURE-form null batch, checked as ``batch.make_feature_batch`` and the C ABI check them --
    here, so that nothing is loaded for a call that cannot succeed.  -> (molecules, pair_index, replicas, seed)."""
    from .scoring import check_features
    replicas, seed = check_null((replicas, seed))
    molecules = list(molecules)
    pair_index = [(int(ia), int(ib)) for ia, ib in pair_index]
    if not molecules or not pair_index:
        raise ValueError("need at least one molecule and one pair")
    for p, (ia, ib) in enumerate(pair_index):
        if not (0 <= ia < len(molecules) and 0 <= ib < len(molecules)):
            raise ValueError(f"pair {p}: molecule index ({ia}, {ib}) out of range (0..{len(molecules) - 1})")
    if len(pair_index) * replicas > 2 ** 31 - 1:
        raise ValueError("npairs * replicas exceeds INT32_MAX")
    for t, (seq, feats) in enumerate(molecules):
        check_features(feats, len(str(seq)), f"molecule {t}")
    return molecules, pair_index, replicas, seed


def null_feature_batch(molecules, pair_index, params, replicas, seed=0, engine=None, hbm_budget_bytes=0, recurrence=0,
                       fit=False, local=False, overlap=False, shuffle="mono"):
    """A FEATURE-form null batch: ``molecules`` (``(seq, (up, down, unp))`` each) and ``pair_index`` as
    ``batch.make_feature_batch`` takes them, every pair against ``replicas`` shuffles of its B -- letters and
    features, made on the GPU from the one uploaded copy of every molecule.  -> ``engine.Batch``; ``run()`` it, then
    ``null_scores()`` / ``null_stats()``.  ``fit``, ``local``, ``overlap``, ``shuffle``: as for ``null_batch`` (the
    dinucleotide model's letters are the sequence letters; the three numbers travel with their positions)."""
    null_model = check_shuffle(shuffle)
    _check_mode(fit, local, overlap)
    molecules, pair_index, replicas, seed = _check_feature_args(molecules, pair_index, replicas, seed)
    from .batch import make_feature_batch
    return _with_model(make_feature_batch(molecules, pair_index, params, engine=engine, hbm_budget_bytes=hbm_budget_bytes,
                                          recurrence=recurrence, score_only=True, null=(replicas, seed), fit=fit, local=local,
                                          overlap=overlap), null_model)


def zscores_features(molecules, pair_index, params, replicas=100, seed=0, observed=None, engine=None, hbm_budget_bytes=0,
                     recurrence=0, fit=False, local=False, overlap=False, shuffle="mono"):
    """``zscores`` for RNA molecules with real-valued structure features: z-scores of the pairs' optimal scores
    against ``replicas`` shuffles of each pair's B (``zscores_from_stats``).  ``observed``: the pairs' real scores if
    the caller has them; else ``make_feature_batch(score_only=True)`` computes them first.  ``fit``, ``local``, ``overlap``,
    ``shuffle``: as for ``zscores``."""
    check_shuffle(shuffle)
    _check_mode(fit, local, overlap)
    molecules, pair_index, replicas, seed = _check_feature_args(molecules, pair_index, replicas, seed)
    common = dict(engine=engine, hbm_budget_bytes=hbm_budget_bytes, recurrence=recurrence, fit=fit, local=local, overlap=overlap)

    def score_batch():
        from .batch import make_feature_batch
        return make_feature_batch(molecules, pair_index, params, score_only=True, **common)
    return _zscores(len(pair_index), observed, score_batch,
                    lambda: null_feature_batch(molecules, pair_index, params, replicas, seed=seed, shuffle=shuffle, **common))


def null_dense_batch(pairs, params, replicas, seed=0, mu1_dense=None, mu2_dense=None, engine=None, hbm_budget_bytes=0,
                     recurrence=0, fit=False, local=False, overlap=False, shuffle="mono"):
    """A DENSE-form null batch: ``pairs`` and their tables as ``batch.make_batch`` takes them (one integer table of shape
    (len A, len B) per pair in ``mu1_dense`` and / or ``mu2_dense``), every pair against ``replicas`` shuffles of its B --
    the tables' columns, and the codes of a form left in LOOKUP form, permuted on the GPU from the one uploaded copy.
    -> ``engine.Batch``; ``run()`` it, then ``null_scores()`` / ``null_stats()``.  ``fit``, ``local``, ``overlap``, ``shuffle``:
    as for ``null_batch``.  The dinucleotide model's letters are B's sequence codes, so it needs mu1 in LOOKUP form: a dense
    mu1 has no letters, and the library refuses (E_UNSUPPORTED)."""
    null_model = check_shuffle(shuffle)
    _check_mode(fit, local, overlap)
    pairs, replicas, seed = check_dense_args(pairs, (replicas, seed), mu1_dense, mu2_dense)
    from .batch import make_batch
    return _with_model(make_batch(pairs, params, engine=engine, hbm_budget_bytes=hbm_budget_bytes, recurrence=recurrence,
                                  score_only=True, mu1_dense=mu1_dense, mu2_dense=mu2_dense, null_dense=(replicas, seed), fit=fit,
                                  local=local, overlap=overlap), null_model)


def zscores_dense(pairs, params, replicas=100, seed=0, mu1_dense=None, mu2_dense=None, observed=None, engine=None,
                  hbm_budget_bytes=0, recurrence=0, fit=False, local=False, overlap=False, shuffle="mono"):
    """``zscores`` for pairs scored through dense tables (a PSSM as ``mu1_dense``, structure scores as ``mu2_dense``):
    z-scores of the pairs' optimal scores against ``replicas`` shuffles of each pair's B (``zscores_from_stats``).
    ``observed``: the pairs' real scores if the caller has them; else ``make_batch(score_only=True)`` with the same
    tables computes them first.  ``fit``, ``local``, ``overlap``, ``shuffle``: as for ``zscores``."""
    check_shuffle(shuffle)
    _check_mode(fit, local, overlap)
    pairs, replicas, seed = check_dense_args(pairs, (replicas, seed), mu1_dense, mu2_dense)
    common = dict(mu1_dense=mu1_dense, mu2_dense=mu2_dense, engine=engine, hbm_budget_bytes=hbm_budget_bytes,
                  recurrence=recurrence, fit=fit, local=local, overlap=overlap)

    def score_batch():
        from .batch import make_batch
        return make_batch(pairs, params, score_only=True, **common)
    return _zscores(len(pairs), observed, score_batch, lambda: null_dense_batch(pairs, params, replicas, seed=seed, shuffle=shuffle, **common))
