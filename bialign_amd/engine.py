"""Python face of the C ABI: Engine (device + stream) and Batch (pairs in HBM).

Thin by design -- argument marshalling only.  All DP work happens in
libbialign_hip.so on the GPU; nothing here computes alignments.
"""
import ctypes
import weakref

import numpy as np

from . import _lib
from ._lib import lib, check
from .batch import check_hit_rules, check_hit_spec
from .significance import check_dense_tables, check_null

STATES = [(0, 1, 0, 1), (0, 1, 1, 0), (0, 1, 1, 1), (1, 0, 0, 1), (1, 0, 1, 0),
          (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 1)]  # pyx:61-65


def device_count():
    n = lib.bialign_device_count()
    if n < 0:
        check(n)
    return n


def _ptr(arr, ctype):
    return arr.ctypes.data_as(ctypes.POINTER(ctype))


class Engine:
    """One HIP device + stream.  Single-owner, not thread-safe."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        self._batches = weakref.WeakSet()  # live batches: closed before the engine goes away
        check(lib.bialign_engine_create(int(device), ctypes.byref(self._h)))
        self.device = int(device)

    def reserve(self, nbytes, tries=4):
        """Pre-allocate the layer buffer kept between batches and pick the best-placed of up to
        ``tries`` candidate allocations (bialign_engine_reserve); returns its probe rate in GB/s."""
        rate = ctypes.c_double()
        check(lib.bialign_engine_reserve(self._h, int(nbytes), int(tries), ctypes.byref(rate)))
        return rate.value

    def trim(self):
        """Release the layer buffer the engine keeps between batches (tens of GB after a large batch)."""
        check(lib.bialign_engine_trim(self._h))

    def close(self):
        if getattr(self, "_h", None):
            for batch in list(self._batches):
                batch.close()
            lib.bialign_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


_default_engines = {}


def default_engine(device=0):
    if device not in _default_engines:
        _default_engines[device] = Engine(device)
    return _default_engines[device]


class Batch:
    """A set of independent pairs sharing one parameter set, resident in HBM.

    ``mols_a`` / ``mols_b``: lists of ``(seq_codes uint8[n], class_codes uint8[n])`` -- or ``mols_a`` a
    ``batch.FlatBatch`` (the whole batch's code arrays, as ``batch.encode_flat`` makes them) and ``mols_b`` None.
    ``s1`` / ``s2``: int32 score tables (k1 x k1, k2 x k2).
    ``mu2_dense``: optional list of int32 arrays, pair p's of shape (n_p, m_p) with entry
    [k-1, l-1] = mu2(k, l); replaces the class codes / ``s2`` (DENSE form of include/bialign.h).
    ``mu1_dense``: likewise for the sequence scores, entry [i-1, j-1] = mu1(i, j) (position-specific
    scores, e.g. a PSSM: ``scoring.dense_mu1_from_pssm``); replaces the sequence codes / ``s1``.
    ``score_only``: the batch will never be traced back (BIALIGN_BATCH_SCORE_ONLY): the sweep keeps
    only the rows the next strip needs; ``traces()`` / ``dump_layers()`` raise.
    ``lean_trace``: scores AND traces from that reduced storage (BIALIGN_BATCH_LEAN_TRACE): the
    traceback re-sweeps one strip at a time; for pairs whose full layers would not fit in HBM.
    ``level_trace``: the same for bands beyond ``_lib.MAX_SHIFT_TILED`` (BIALIGN_BATCH_LEVEL_TRACE): the sweep
    leaves checkpoints of five anti-diagonal levels, the traceback re-sweeps one segment of levels at a time.
    Excludes ``score_only`` and ``lean_trace``; the engine takes it by itself when a wide-band pair's layers
    exceed the HBM budget (``info["storage"] == _lib.BATCH_LEVEL_TRACE``).
    ``mu2_features``: ``(structure_weight, feats_a, feats_b)``, mu2 in FEATURE form (include/bialign.h,
    bialign_features): the RNA structure score of real-valued per-residue features (predicted structures), whose
    n x m tables the GPU builds itself, chunk by chunk.  With molecule lists ``feats_a[p]`` / ``feats_b[p]`` is
    pair p's ``(up, down, unp)`` (``scoring.rna_features``); with a ``batch.FlatBatch`` they are triples of flat
    float64 arrays indexed like ``seq_a`` / ``seq_b``, so that pairs may share molecules
    (``batch.make_feature_batch``).  Replaces the class codes / ``s2``; excludes ``mu2_dense``.
    ``null``: ``(replicas, seed)``, a null batch (bialign_batch_create_null; ``significance.null_batch``): every pair
    against ``replicas`` shuffles of its B molecule, made on the GPU from the one uploaded copy of B, as one score-only
    batch.  Results come from ``null_scores()`` / ``null_stats()``; ``scores()`` raises.  mu1 in LOOKUP form; mu2 in
    LOOKUP form or, together with ``mu2_features``, in FEATURE form (bialign_batch_create_null_features;
    ``significance.null_feature_batch``): a residue's three numbers then move with its letter.
    ``null_dense``: ``(replicas, seed)``, a null batch with ``mu1_dense`` and / or ``mu2_dense``
    (bialign_batch_create_null_dense; ``significance.null_dense_batch``): a residue of B carries its column of every
    table, and the GPU permutes the columns of the one uploaded copy of the tables per replica, chunk by chunk.  The other
    of mu1 / mu2 may stay in LOOKUP form.  Excludes ``null``, ``mu2_features``, ``lean_trace`` and ``level_trace``; the
    tables must be of an integer dtype.  Results as for ``null``; ``null_tables()`` shows a replica's tables.
    ``fit``: fit alignments (BIALIGN_BATCH_FIT): A inside a longer B, B's end gaps free.  ``scores()`` is the best
    global score of A against any substring of B, ``traces()`` that alignment, ``fit_spans()`` the substring.  Bands
    up to ``_lib.MAX_SHIFT_TILED``, full storage or ``score_only`` (and so null batches: the replicas are scored in
    the same mode); not with ``lean_trace`` / ``level_trace``.  In full storage ``set_hits()`` adds a search for every
    placement of A in B: ``fit_hits()``, ``hit_profile()``, ``fit_hit_walks()``, ``hit_thresholds()``.
    ``local``: local alignments (BIALIGN_BATCH_LOCAL): the best-scoring parts of A and B, the ends of both free.
    ``scores()`` is the best global score of any substring of A against any substring of B (>= 0), ``traces()`` that
    alignment, ``local_spans()`` the two substrings.  Bands up to ``_lib.MAX_SHIFT_TILED``, ``gap_opening_cost <= 0``
    in the affine recurrence, full storage or ``score_only`` (and so null batches); not with ``fit``, ``lean_trace``
    or ``level_trace``.
    ``overlap``: overlap alignments (BIALIGN_BATCH_OVERLAP): the global alignment whose end gaps cost nothing in either
    molecule.  ``scores()`` is the best global score of A[i0:i1] against B[j0:j1] over the windows that start at the
    beginning of A or of B and end at the end of A or of B (>= 0), ``traces()`` that alignment, ``overlap_spans()`` the
    window.  Bands up to ``_lib.MAX_SHIFT_TILED``, full storage or ``score_only`` (and so null batches); not with
    ``fit``, ``local``, ``lean_trace`` or ``level_trace``.
    """

    def __init__(self, engine, mols_a, mols_b, s1, s2, gap_opening_cost, gap_cost, shift_cost,
                 max_shift, hbm_budget_bytes=0, recurrence=0, mu2_dense=None, score_only=False,
                 lean_trace=False, mu1_dense=None, mu2_features=None, level_trace=False, null=None, null_dense=None,
                 fit=False, local=False, overlap=False):
        null_kind = "dense" if null_dense is not None else ("lookup" if null is not None else None)
        if null_dense is not None:
            if mu1_dense is None and mu2_dense is None:
                raise ValueError("null_dense needs mu1_dense and / or mu2_dense (a LOOKUP null batch is null=)")
            if null is not None or mu2_features is not None:
                raise ValueError("null_dense excludes null and mu2_features")
        elif null is not None:
            replicas, seed = check_null(null)
            if mu2_dense is not None or mu1_dense is not None:
                raise ValueError("a null batch takes mu1 in LOOKUP form and mu2 in LOOKUP or FEATURE form "
                                 "(no mu1_dense / mu2_dense)")
        if null_kind:
            if lean_trace or level_trace:
                raise ValueError("a null batch is score-only: lean_trace / level_trace do not apply")
            if null_dense is not None:
                replicas, seed = check_null(null_dense)
        if mu2_features is not None and mu2_dense is not None:
            raise ValueError("mu2_features and mu2_dense exclude each other")
        if level_trace and (score_only or lean_trace):
            raise ValueError("level_trace excludes score_only and lean_trace")
        flat = mols_b is None and hasattr(mols_a, "seq_a")
        if mols_b is None and hasattr(mols_a, "seq_a"):  # a batch.FlatBatch: the arrays are the ABI's already
            fb = mols_a
            if not len(fb.len_a):
                raise ValueError("need the same, non-zero number of A and B molecules")
            self.len_a, self.len_b, off_a, off_b = fb.len_a, fb.len_b, fb.off_a, fb.off_b
            seq_a, cls_a, seq_b, cls_b = fb.seq_a, fb.cls_a, fb.seq_b, fb.cls_b
        else:
            if len(mols_a) != len(mols_b) or not mols_a:
                raise ValueError("need the same, non-zero number of A and B molecules")
            self.len_a = np.array([len(x[0]) for x in mols_a], dtype=np.int32)
            self.len_b = np.array([len(x[0]) for x in mols_b], dtype=np.int32)
            off_a = np.zeros(len(mols_a), dtype=np.int64)
            off_b = np.zeros(len(mols_a), dtype=np.int64)
            off_a[1:] = np.cumsum(self.len_a[:-1])
            off_b[1:] = np.cumsum(self.len_b[:-1])
            seq_a = np.ascontiguousarray(np.concatenate([np.asarray(x[0], dtype=np.uint8) for x in mols_a]))
            cls_a = np.ascontiguousarray(np.concatenate([np.asarray(x[1], dtype=np.uint8) for x in mols_a]))
            seq_b = np.ascontiguousarray(np.concatenate([np.asarray(x[0], dtype=np.uint8) for x in mols_b]))
            cls_b = np.ascontiguousarray(np.concatenate([np.asarray(x[1], dtype=np.uint8) for x in mols_b]))
        self.engine = engine
        self.npairs = len(self.len_a)
        self.max_shift = int(max_shift)
        if len(seq_a) != len(cls_a) or len(seq_b) != len(cls_b):
            raise ValueError("sequence and structure codes must have equal length")
        s1 = np.ascontiguousarray(s1, dtype=np.int32)
        s2 = np.ascontiguousarray(s2, dtype=np.int32)
        if seq_a.size and (seq_a.max() >= s1.shape[0] or seq_b.max() >= s1.shape[0]):
            raise ValueError("sequence code outside the S1 table")
        if cls_a.size and (cls_a.max() >= s2.shape[0] or cls_b.max() >= s2.shape[0]):
            raise ValueError("structure class outside the S2 table")
        feat = None if mu2_features is None else self._features(mu2_features, flat, len(seq_a), len(seq_b), off_a, off_b)
        if null_dense is not None:  # (stricter than a plain batch: no silent cast of floats or of values beyond int32)
            for tables, name in ((mu1_dense, "mu1_dense"), (mu2_dense, "mu2_dense")):
                if tables is not None:
                    check_dense_tables(tables, self.len_a, self.len_b, name)
        mu2_flat, mu2_off = self._dense_tables(mu2_dense, "mu2_dense")
        mu1_flat, mu1_off = self._dense_tables(mu1_dense, "mu1_dense")
        mu2_ptr = mu2_off_ptr = mu1_ptr = mu1_off_ptr = None
        if mu2_flat is not None:
            mu2_ptr, mu2_off_ptr = _ptr(mu2_flat, ctypes.c_int32), _ptr(mu2_off, ctypes.c_int64)
        if mu1_flat is not None:
            mu1_ptr, mu1_off_ptr = _ptr(mu1_flat, ctypes.c_int32), _ptr(mu1_off, ctypes.c_int64)
        prm = _lib.Params(int(gap_opening_cost), int(gap_cost), int(shift_cost), int(max_shift),
                          int(recurrence), (_lib.BATCH_SCORE_ONLY if score_only else 0) |
                          (_lib.BATCH_LEAN_TRACE if lean_trace else 0) |
                          (_lib.BATCH_LEVEL_TRACE if level_trace else 0) | (_lib.BATCH_FIT if fit else 0) |
                          (_lib.BATCH_LOCAL if local else 0) | (_lib.BATCH_OVERLAP if overlap else 0))
        sc = _lib.Scoring(s1.shape[0], _ptr(s1, ctypes.c_int32), s2.shape[0], _ptr(s2, ctypes.c_int32))
        pr = _lib.Pairs(self.npairs, _ptr(self.len_a, ctypes.c_int32), _ptr(self.len_b, ctypes.c_int32),
                        _ptr(off_a, ctypes.c_int64), _ptr(off_b, ctypes.c_int64),
                        _ptr(seq_a, ctypes.c_uint8), _ptr(cls_a, ctypes.c_uint8),
                        _ptr(seq_b, ctypes.c_uint8), _ptr(cls_b, ctypes.c_uint8), mu2_ptr, mu2_off_ptr,
                        mu1_ptr, mu1_off_ptr)
        self._h = ctypes.c_void_p()
        self.replicas = None
        self.fit = bool(fit)
        self.local = bool(local)
        self.overlap = bool(overlap)
        self.hit_spec = None   # set_hits: (max_hits, max_walks, min_score)
        self._null_forms = (mu1_flat is not None, mu2_flat is not None) if null_dense is not None else None
        args = [engine._h, ctypes.byref(prm), ctypes.byref(sc), ctypes.byref(pr)]
        if feat is not None:
            sw, fa, fb = feat
            ft = _lib.Features(sw, *(_ptr(x, ctypes.c_double) for x in fa + fb))
            args.append(ctypes.byref(ft))
        if null_kind:
            if self.npairs * replicas > 2 ** 31 - 1:
                raise ValueError("npairs * replicas exceeds INT32_MAX")
            self.replicas = replicas
            spec = _lib.NullSpec(replicas, seed)
            args.append(ctypes.byref(spec))
        create = {(None, False): lib.bialign_batch_create, (None, True): lib.bialign_batch_create_features,
                  ("lookup", False): lib.bialign_batch_create_null, ("lookup", True): lib.bialign_batch_create_null_features,
                  ("dense", False): lib.bialign_batch_create_null_dense}[null_kind, feat is not None]
        check(create(*args, int(hbm_budget_bytes), ctypes.byref(self._h)))
        engine._batches.add(self)
        self.info = self.current_info()
        self.affine = bool(self.info["affine"])

    def _features(self, mu2_features, flat, tot_a, tot_b, off_a, off_b):
        """``mu2_features`` -> (int structure weight, three flat float64 arrays for side A, three for side B),
        validated as the C ABI validates them (scoring.check_features) before the library is called."""
        from .scoring import check_features
        try:
            sw, feats_a, feats_b = mu2_features
        except (TypeError, ValueError):
            raise ValueError("mu2_features must be (structure_weight, feats_a, feats_b)") from None
        if int(sw) != sw:
            raise ValueError("structure_weight must be an integer")
        sides = []
        for side, feats, tot, lens in (("A", feats_a, tot_a, self.len_a), ("B", feats_b, tot_b, self.len_b)):
            if flat:
                sides.append(check_features(feats, tot, f"molecules {side}"))
                continue
            if len(feats) != self.npairs:
                raise ValueError(f"mu2_features needs one (up, down, unp) per pair for side {side}")
            per = [check_features(f, int(lens[p]), f"pair {p}, molecule {side}") for p, f in enumerate(feats)]
            sides.append(tuple(np.ascontiguousarray(np.concatenate([f[x] for f in per])) for x in range(3)))
        return int(sw), sides[0], sides[1]

    def _dense_tables(self, tables, name):
        """One (len A, len B) integer table per pair -> (flat int32 array, int64 offsets), or (None, None)."""
        if tables is None:
            return None, None
        if len(tables) != self.npairs:
            raise ValueError(f"{name} needs one table per pair")
        flat = []
        for p, tab in enumerate(tables):
            tab = np.asarray(tab)
            if tab.shape != (int(self.len_a[p]), int(self.len_b[p])):
                raise ValueError(f"{name}[{p}] must have shape (len A, len B) = "
                                 f"({int(self.len_a[p])}, {int(self.len_b[p])}), got {tab.shape}")
            flat.append(np.ascontiguousarray(tab, dtype=np.int32).ravel())
        off = np.zeros(self.npairs, dtype=np.int64)
        off[1:] = np.cumsum([f.size for f in flat[:-1]])
        return np.ascontiguousarray(np.concatenate(flat)), off

    def current_info(self):
        """bialign_batch_get_info now (``info`` is the answer at creation; a fallback to full records may re-chunk)."""
        info = _lib.BatchInfo()
        check(lib.bialign_batch_get_info(self._h, ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def feature_info(self):
        """bialign_batch_get_feature_info: the form mu2 came in ("lookup", "dense", "feature"), the table bytes (of the
        largest chunk in FEATURE form), and the table builder's kernel time and launches of the last run."""
        fi = _lib.FeatureInfo()
        check(lib.bialign_batch_get_feature_info(self._h, ctypes.byref(fi)))
        return dict(form=("lookup", "dense", "feature")[fi.form], table_bytes=fi.table_bytes,
                    build_ms=fi.build_ms, build_launches=fi.build_launches)

    def null_scores(self):
        """Null batch: the replica scores of the last run, int32 of shape (npairs, replicas)."""
        self._need_null()
        out = np.empty((self.npairs, self.replicas), dtype=np.int32)
        check(lib.bialign_batch_get_null_scores(self._h, _ptr(out, ctypes.c_int32)))
        return out

    def null_stats(self, observed=None):
        """Null batch: every pair's replica scores reduced on the GPU to exact integers -- a dict of arrays ``sum``,
        ``sumsq`` (int64), ``min``, ``max``, ``n_ge``, ``replicas`` (int32).  ``observed``: the real pairs' scores, for
        ``n_ge`` = replicas scoring at least that much (0 everywhere when None)."""
        self._need_null()
        obs_ptr = None
        if observed is not None:
            observed = np.ascontiguousarray(observed, dtype=np.int32)
            if observed.shape != (self.npairs,):
                raise ValueError("observed needs one score per pair")
            obs_ptr = _ptr(observed, ctypes.c_int32)
        out = (_lib.NullStats * self.npairs)()
        check(lib.bialign_batch_get_null_stats(self._h, obs_ptr, out))
        arr = np.frombuffer(out, dtype=np.dtype([("sum", "<i8"), ("sumsq", "<i8"), ("min", "<i4"), ("max", "<i4"),
                                                  ("n_ge", "<i4"), ("replicas", "<i4")]))
        return {k: arr[k].copy() for k in arr.dtype.names}

    def null_info(self):
        """Null batch: kernel times of the shuffle (last run) and of the last ``null_stats`` reduction, and the bytes of
        the replicas' codes (FEATURE form: and feature planes) in HBM."""
        self._need_null()
        ni = _lib.NullInfo()
        check(lib.bialign_batch_get_null_info(self._h, ctypes.byref(ni)))
        return dict(shuffle_ms=ni.shuffle_ms, stats_ms=ni.stats_ms, replica_bytes=ni.replica_bytes)

    def set_null_model(self, model):
        """Null batch: the null model of the replicas from the next run on -- ``"mono"`` / 0 (THE PERMUTATION) or
        ``"dinucleotide"`` / 1 (THE DINUCLEOTIDE PERMUTATION of include/bialign.h).  A refused model (BialignError)
        leaves the batch as it was."""
        self._need_null()
        from .significance import SHUFFLES
        number = SHUFFLES.index(model) if model in SHUFFLES else model
        check(lib.bialign_batch_set_null_model(self._h, int(number)))

    @property
    def null_model(self):
        """Null batch: the name of the null model in force, ``"mono"`` or ``"dinucleotide"``."""
        self._need_null()
        from .significance import SHUFFLES
        model = ctypes.c_int32()
        check(lib.bialign_batch_get_null_model(self._h, ctypes.byref(model)))
        return SHUFFLES[model.value]

    def dump_null_codes(self, pair, replica):
        """Null batch, test hook: (sequence codes, class codes) of one replica of one pair's B as the sweep reads them."""
        self._need_null()
        m = int(self.len_b[pair])
        seq, cls = np.empty(m, dtype=np.uint8), np.empty(m, dtype=np.uint8)
        check(lib.bialign_batch_dump_null_codes(self._h, int(pair), int(replica), _ptr(seq, ctypes.c_uint8),
                                                _ptr(cls, ctypes.c_uint8)))
        return seq, cls

    def dump_null_features(self, pair, replica):
        """FEATURE-form null batch, test hook: ``(up, down, unp)`` of one replica of one pair's B as the table builder
        reads them, float64 arrays of len B."""
        self._need_null()
        m = int(self.len_b[pair])
        out = tuple(np.empty(m, dtype=np.float64) for _ in range(3))
        check(lib.bialign_batch_dump_null_features(self._h, int(pair), int(replica),
                                                   *(_ptr(x, ctypes.c_double) for x in out)))
        return out

    def null_tables(self, pair, replica):
        """DENSE-form null batch, test hook: ``(mu1, mu2)`` of one replica of one pair as the sweep reads them, int32
        arrays of shape (len A, len B); None for a form the batch holds in LOOKUP form."""
        self._need_null()
        if self._null_forms is None:
            raise ValueError("not a DENSE-form null batch (create it with null_dense=(replicas, seed))")
        shape = (int(self.len_a[pair]), int(self.len_b[pair]))
        out = [np.empty(shape, dtype=np.int32) if have else None for have in self._null_forms]
        check(lib.bialign_batch_dump_null_tables(self._h, int(pair), int(replica),
                                                 *(None if x is None else _ptr(x, ctypes.c_int32) for x in out)))
        return tuple(out)

    def _need_null(self):
        if self.replicas is None:
            raise ValueError("not a null batch (create it with null=(replicas, seed) or null_dense=(replicas, seed))")

    def dump_mu2(self, pair):
        """The (len A, len B) int32 mu2 table of one pair as the sweep reads it (DENSE or FEATURE form)."""
        fn = getattr(lib, "bialign_batch_dump_mu2", None)
        if fn is None:
            raise _lib.BialignError(_lib.E_UNSUPPORTED, "this build of the library has no bialign_batch_dump_mu2")
        out = np.empty((int(self.len_a[pair]), int(self.len_b[pair])), dtype=np.int32)
        check(fn(self._h, int(pair), _ptr(out, ctypes.c_int32)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib.bialign_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def run(self, fill_only=False, wait=True):
        """Fill (+ traceback).  ``wait=False`` only enqueues the kernels (BIALIGN_RUN_ASYNC): the host
        may encode / create the next batch meanwhile; ``wait()`` or any result getter completes the run."""
        check(lib.bialign_batch_run(self._h, (_lib.RUN_FILL_ONLY if fill_only else 0) | (0 if wait else _lib.RUN_ASYNC)))

    def wait(self):
        check(lib.bialign_batch_wait(self._h))

    def timing(self):
        t = _lib.Timing()
        check(lib.bialign_batch_get_timing(self._h, ctypes.byref(t)))
        return dict(fill_ms=t.fill_ms, traceback_ms=t.traceback_ms,
                    fill_launches=t.fill_launches, traceback_launches=t.traceback_launches,
                    waves_per_pair=t.waves_per_pair, cross_cu=bool(t.cross_cu), recovered_runs=t.recovered_runs,
                    packed_records=bool(t.packed_records))

    def scores(self):
        out = np.empty(self.npairs, dtype=np.int32)
        check(lib.bialign_batch_get_scores(self._h, _ptr(out, ctypes.c_int32)))
        return out

    def traces(self):
        """-> (list of uint8 arrays of column codes start->end, complete flags)."""
        buf = np.empty(max(1, self.info["trace_bytes"]), dtype=np.uint8)
        off = np.empty(self.npairs, dtype=np.int64)
        ln = np.empty(self.npairs, dtype=np.int32)
        ok = np.empty(self.npairs, dtype=np.int32)
        check(lib.bialign_batch_get_traces(self._h, _ptr(buf, ctypes.c_uint8), _ptr(off, ctypes.c_int64),
                                           _ptr(ln, ctypes.c_int32), _ptr(ok, ctypes.c_int32)))
        return [buf[off[p]:off[p] + ln[p]].copy() for p in range(self.npairs)], ok.astype(bool)

    def fit_spans(self):
        """Fit batch: ``(start_b, end_b)`` as int32 arrays -- pair p's alignment is that of A with
        ``B[start_b[p]:end_b[p]]``.  After a score-only or fill-only run ``start_b`` is -1."""
        start, end = np.empty(self.npairs, dtype=np.int32), np.empty(self.npairs, dtype=np.int32)
        check(lib.bialign_batch_get_fit_spans(self._h, _ptr(start, ctypes.c_int32), _ptr(end, ctypes.c_int32)))
        return start, end

    def set_hits(self, max_hits, min_score=None, max_walks=0, peaks=False, min_scores=None, min_permille=0):
        """Fit batch, full storage: search every later run for up to ``max_hits`` disjoint placements of A in B that
        score at least ``min_score`` (bialign_batch_set_hits; the model is stated in include/bialign.h).  ``max_walks``
        bounds the walks a pair may cost, 0 means ``4 * max_hits``.  ``peaks``: only the peaks of a pair's end-score
        profile are candidates (BIALIGN_HITS_PEAKS), which reaches the farther copies without a discarded walk from every
        end behind a hit.  ``min_scores`` (one int >= 1 per pair) and ``min_permille`` (0..1000, of the pair's fit score)
        give every pair its own threshold (bialign_batch_set_hit_thresholds; ``hit_thresholds()`` reports them).
        ``set_hits(None)`` removes the search again."""
        if max_hits is None:
            check(lib.bialign_batch_set_hits(self._h, None))
            self.hit_spec = None
            return
        if min_score is None:
            raise ValueError("set_hits needs min_score (set_hits(None) removes the search)")
        max_hits, min_score, max_walks = check_hit_spec(max_hits, min_score, max_walks)
        peaks, min_scores, min_permille = check_hit_rules(peaks, min_scores, min_permille, self.npairs)
        spec = _lib.HitSpec(max_hits, max_walks, min_score, _lib.HITS_PEAKS if peaks else 0)
        self.hit_spec = None
        check(lib.bialign_batch_set_hits(self._h, ctypes.byref(spec)))
        self.hit_spec = (max_hits, max_walks or 4 * max_hits, min_score)
        if min_scores is not None or min_permille:
            check(lib.bialign_batch_set_hit_thresholds(
                self._h, None if min_scores is None else _ptr(min_scores, ctypes.c_int32), min_permille))

    def hit_thresholds(self):
        """int32 ``T[p]``: the least score a candidate end of pair p had to reach in the last run (include/bialign.h,
        "Thresholds"); -1 before a run and after a fill-only run."""
        self._need_hits()
        out = np.empty(self.npairs, dtype=np.int32)
        check(lib.bialign_batch_get_hit_thresholds(self._h, _ptr(out, ctypes.c_int32)))
        return out

    def _need_hits(self):
        if self.hit_spec is None:
            raise ValueError("no hit search is set on this batch (set_hits, or make_batch(..., fit=True, hits=(K, min_score)))")
        return self.hit_spec

    def hit_profile(self, pair):
        """The end-score profile of one pair: int32 ``E[0..len B]``, ``E[j]`` the score of the best placement of A that
        ends at j.  -2^30 everywhere before a run."""
        self._need_hits()
        out = np.empty(int(self.len_b[pair]) + 1, dtype=np.int32)
        check(lib.bialign_batch_get_hit_profile(self._h, int(pair), _ptr(out, ctypes.c_int32)))
        return out

    def fit_hits(self):
        """-> (hits, status): per pair a list of ``(start_b, end_b, score, trace)`` in order of acceptance -- the global
        alignment of A with ``B[start_b:end_b]``, trace as ``traces()`` gives it -- and one of ``_lib.HIT_STATUS``."""
        k, _, _ = self._need_hits()
        nh, st = (np.empty(self.npairs, dtype=np.int32) for _ in range(2))
        start, end, score, tlen = (np.empty((self.npairs, k), dtype=np.int32) for _ in range(4))
        buf = np.empty(max(1, k * self.info["trace_bytes"]), dtype=np.uint8)
        off = np.empty((self.npairs, k), dtype=np.int64)
        check(lib.bialign_batch_get_hits(self._h, *(_ptr(x, ctypes.c_int32) for x in (nh, st, start, end, score, tlen)),
                                         _ptr(buf, ctypes.c_uint8), _ptr(off, ctypes.c_int64)))
        hits = [[(int(start[p, h]), int(end[p, h]), int(score[p, h]), buf[off[p, h]:off[p, h] + tlen[p, h]].copy())
                 for h in range(int(nh[p]))] for p in range(self.npairs)]
        return hits, [_lib.HIT_STATUS[int(x)] for x in st]

    def fit_hit_walks(self):
        """The search's log: per pair a list of ``(end_b, start_b, score, accepted)``, one entry per walk in the order
        the walks were made."""
        _, k, _ = self._need_hits()
        nw = np.empty(self.npairs, dtype=np.int32)
        end, start, score, acc = (np.empty((self.npairs, k), dtype=np.int32) for _ in range(4))
        check(lib.bialign_batch_get_hit_walks(self._h, *(_ptr(x, ctypes.c_int32) for x in (nw, end, start, score, acc))))
        return [[(int(end[p, w]), int(start[p, w]), int(score[p, w]), bool(acc[p, w])) for w in range(int(nw[p]))]
                for p in range(self.npairs)]

    def hit_info(self):
        """bialign_batch_get_hit_info: the spec with its flags, the result buffers' bytes, the search kernels' time of the last run."""
        self._need_hits()
        hi = _lib.HitInfo()
        check(lib.bialign_batch_get_hit_info(self._h, ctypes.byref(hi)))
        return dict(max_hits=hi.spec.max_hits, max_walks=hi.spec.max_walks, min_score=hi.spec.min_score,
                    flags=hi.spec.flags, peaks=bool(hi.spec.flags & _lib.HITS_PEAKS), buffer_bytes=hi.buffer_bytes, search_ms=hi.search_ms)

    def local_spans(self):
        """Local batch: ``(start_a, end_a, start_b, end_b)`` as int32 arrays -- pair p's alignment is that of
        ``A[start_a[p]:end_a[p]]`` with ``B[start_b[p]:end_b[p]]``.  After a score-only or fill-only run the starts
        are -1."""
        out = [np.empty(self.npairs, dtype=np.int32) for _ in range(4)]
        check(lib.bialign_batch_get_local_spans(self._h, *[_ptr(x, ctypes.c_int32) for x in out]))
        return tuple(out)

    def overlap_spans(self):
        """Overlap batch: ``(start_a, end_a, start_b, end_b)`` as int32 arrays -- pair p's alignment is that of
        ``A[start_a[p]:end_a[p]]`` with ``B[start_b[p]:end_b[p]]``.  After a score-only or fill-only run the starts
        are -1."""
        out = [np.empty(self.npairs, dtype=np.int32) for _ in range(4)]
        check(lib.bialign_batch_get_overlap_spans(self._h, *[_ptr(x, ctypes.c_int32) for x in out]))
        return tuple(out)

    def dump_layers(self, pair):
        """Layers of one pair in the reference layout [layer][i][j][k-i+s][l-j+s]."""
        n, m, w = int(self.len_a[pair]), int(self.len_b[pair]), 2 * self.max_shift + 1
        nl = 9 if self.affine else 1
        out = np.empty((nl, n + 1, m + 1, w, w), dtype=np.int32)
        check(lib.bialign_batch_dump_layers(self._h, int(pair), _ptr(out, ctypes.c_int32)))
        return out


def trace_codes_to_columns(codes, as_tuples=False):
    """Column codes -> the reference's trace entries (lists for the affine
    recurrence, pyx:568; tuples for the non-affine one, pyx:526)."""
    cols = [[(c >> 3) & 1, (c >> 2) & 1, (c >> 1) & 1, c & 1] for c in codes.tolist()]
    return [tuple(c) for c in cols] if as_tuples else cols
