#!/usr/bin/env python3
"""A/B of the two ways a shuffled null reaches the engine, for each of the three forms a null batch has (--kind):

  lookup    HOST: Python builds npairs x R shuffled B strings, make_batch encodes and uploads them, an ordinary
            SCORE_ONLY batch scores them.  NULL: significance.null_batch.
  features  RNA molecules with real-valued structure features.  HOST: numpy builds npairs x R shuffled copies of every
            B molecule -- letters and three planes of doubles --, make_feature_batch(score_only=True) checks, encodes
            and uploads them all.  NULL: significance.null_feature_batch.
  dense     pairs scored through dense tables (a PSSM as mu1_dense, structure scores computed outside as mu2_dense).
            HOST: numpy permutes the columns of every pair's tables R times -- and the letters of a form left in LOOKUP
            form --, make_batch(score_only=True, mu1_dense=, mu2_dense=) uploads all R x sum(n * m) entries and keeps
            them resident.  NULL: significance.null_dense_batch.

HOST shuffles with the permutation of include/bialign.h and reduces the scores with numpy; NULL uploads every B once,
and the GPU shuffles and reduces.  One form per process.  The HOST form restates the permutation itself (vectorised
over all replicas with numpy) and needs nothing newer than its kind's base feature (SCORE_ONLY, the FEATURE form, the
DENSE forms), so it also runs from a checkout of an older commit (copy this file there) or against an older build of
the library (BIALIGN_LIB_OVERRIDE): that is the baseline.  Per shape one JSON line: medians over --reps cycles (after a
small warm-up batch) of host preparation, upload + batch creation, shuffle / build / fill / stats kernel ms, the whole
cycle's wall ms, and hashes of the replica scores and of the per-pair sums (equal between the forms).

    python tools/ab_null.py [--kind lookup|features|dense] --form host|null [--shape a|b|all] [--reps 5] [--replicas R]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bialign_amd import synth  # noqa: E402

M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """include/bialign.h, mix(), on a uint64 array holding uint32 values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def permutations(seed, npairs, replicas, m):
    """perm[p * replicas + r] for all pairs and replicas at once (all B molecules of length m)."""
    p = np.repeat(np.arange(npairs, dtype=np.uint64), replicas)
    r = np.tile(np.arange(replicas, dtype=np.uint64), npairs)
    h = mix((mix((mix(np.uint64(seed ^ 0x9E3779B9)[None]) + p) & M32) + r) & M32)
    perm = np.tile(np.arange(m, dtype=np.int64), (npairs * replicas, 1))
    rows = np.arange(npairs * replicas)
    for t in range(m - 1, 0, -1):
        j = ((mix((h + np.uint64(t)) & M32) * np.uint64(t + 1)) >> np.uint64(32)).astype(np.int64)
        at_t, at_j = perm[:, t].copy(), perm[rows, j]
        perm[rows, j] = at_t
        perm[:, t] = at_j
    return perm


def digest(x):
    return hashlib.sha256(np.asarray(x, dtype=np.int64).tobytes()).hexdigest()[:16]


def letters(s):
    return np.frombuffer(s.encode("latin-1"), dtype=np.uint8)


def text(codes):
    return codes.tobytes().decode("latin-1")


# ---- per kind: the shapes -- name: (description, pairs, length, max_shift, replicas, what the kind adds) --, the inputs
# of a shape -> (params, one item per pair, what all pairs share), and the HOST / NULL constructor pair.  host_*:
# -> a callable that creates the batch from the shuffles prepared here; null_*: -> the batch.

LOOKUP_SHAPES = {
    "a": ("256 protein pairs x len 512, s=1", 256, 512, 1, 100, False),
    "b": ("64 RNA pairs x len 300, s=2", 64, 300, 2, 100, True),
}


def lookup_inputs(form, npairs, length, s, rna):
    if not rna:
        return dict(synth.PROTEIN_PARAMS, max_shift=s), synth.protein_batch(npairs, length), rna
    pairs = synth.rna_batch(npairs, length)
    if form == "host":   # the structure as per-position class letters: what a shuffle moves (significance.shuffle_b, rna=True)
        from bialign_amd.scoring import rna_classes
        cls = lambda structure: "".join(".()"[c] for c in rna_classes(structure).tolist())  # noqa: E731
        pairs = [(sa, sb, cls(ta), cls(tb)) for sa, sb, ta, tb in pairs]
    return dict(synth.RNA_PARAMS, max_shift=s), pairs, rna


def host_lookup(pairs, rna, params, replicas, seed):
    from bialign_amd import batch
    perm = permutations(seed, len(pairs), replicas, len(pairs[0][1]))
    virtual = []
    for p, (sa, sb, ta, tb) in enumerate(pairs):
        rows = perm[p * replicas:(p + 1) * replicas]
        for sq, cl in zip(letters(sb)[rows], letters(tb)[rows]):
            virtual.append((sa, text(sq), ta, text(cl)))
    if rna:   # (a shuffled class string is no structure: the classes go in as a protein-style alphabet of three letters)
        params = dict(params, type="Protein", simmatrix=None)
    return lambda: batch.make_batch(virtual, params, score_only=True)


def null_lookup(significance, pairs, rna, params, replicas, seed):
    return significance.null_batch(pairs, params, replicas, seed=seed)


FEATURE_SHAPES = {
    "a": ("64 RNA pairs x len 300, s=2, R=100", 64, 300, 2, 100, None),
    "b": ("256 RNA pairs x len 512, s=1, R=20", 256, 512, 1, 20, None),
}


def molecule(seed, n):
    """(sequence, (up, down, unp)): a probability split per residue, some entries exactly 0."""
    rng = np.random.default_rng(seed)
    raw = rng.dirichlet([0.6, 0.6, 0.9], size=n)
    kind = rng.integers(0, 6, size=n)
    up, down = raw[:, 0].copy(), raw[:, 1].copy()
    up[kind == 0] = 0.0
    down[kind == 1] = 0.0
    up[kind == 2], down[kind == 2] = 0.0, 0.0
    return "".join(rng.choice(list("ACGU"), size=n)), (up, down, 1.0 - up - down)


def feature_inputs(form, npairs, length, s, _):
    mols = [molecule(9000 + t, length) for t in range(2 * npairs)]
    return dict(synth.RNA_PARAMS, max_shift=s), [(2 * t, 2 * t + 1) for t in range(npairs)], mols


def host_features(index, mols, params, replicas, seed):
    from bialign_amd import batch
    perm = permutations(seed, len(index), replicas, len(mols[index[0][1]][0]))
    ext, idx = list(mols), []
    for p, (ia, ib) in enumerate(index):
        rows = perm[p * replicas:(p + 1) * replicas]
        seqs = letters(mols[ib][0])[rows]
        planes = [f[rows] for f in mols[ib][1]]
        for r in range(replicas):
            ext.append((text(seqs[r]), (planes[0][r], planes[1][r], planes[2][r])))
            idx.append((ia, len(ext) - 1))
    return lambda: batch.make_feature_batch(ext, idx, params, score_only=True)


def null_features(significance, index, mols, params, replicas, seed):
    return significance.null_feature_batch(mols, index, params, replicas, seed=seed)


DENSE_SHAPES = {
    "a": ("64 protein pairs x len 300, s=2, mu1 and mu2 dense, R=100", 64, 300, 2, 100, ("mu1", "mu2")),
    "b": ("256 protein pairs x len 512, s=1, mu1 dense, R=20", 256, 512, 1, 20, ("mu1",)),
}


def tables_of(seed, n, m):
    """(mu1, mu2) of one pair: a PSSM-like table in the x100 scale of the score tables, structure scores >= 0."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-400, 1100, size=(n, m), dtype=np.int32), rng.integers(0, 800, size=(n, m), dtype=np.int32))


def dense_inputs(form, npairs, length, s, forms):
    items = [(synth.protein_pair(9100 + t, length), tables_of(9100 + t, length, length)) for t in range(npairs)]
    return dict(synth.PROTEIN_PARAMS, max_shift=s), items, forms


def dense_tables(items, forms):
    return {name: [tabs[i] for _, tabs in items] for i, name in enumerate(("mu1", "mu2")) if name in forms}


def host_dense(items, forms, params, replicas, seed):
    from bialign_amd import batch
    dense = dense_tables(items, forms)
    perm = permutations(seed, len(items), replicas, len(items[0][0][1]))
    ext, ext_tabs = [], {name: [] for name in dense}
    for p, ((sa, sb, ta, tb), _) in enumerate(items):
        rows = perm[p * replicas:(p + 1) * replicas]
        seqs, strs = letters(sb)[rows], letters(tb)[rows]
        for r in range(replicas):
            ext.append((sa, text(seqs[r]), ta, text(strs[r])))
            for name in dense:
                ext_tabs[name].append(dense[name][p][:, rows[r]])
    return lambda: batch.make_batch(ext, params, score_only=True, mu1_dense=ext_tabs.get("mu1"), mu2_dense=ext_tabs.get("mu2"))


def null_dense(significance, items, forms, params, replicas, seed):
    dense = dense_tables(items, forms)
    return significance.null_dense_batch([pair for pair, _ in items], params, replicas, seed=seed,
                                         mu1_dense=dense.get("mu1"), mu2_dense=dense.get("mu2"))


TIMES = ("prepare_ms", "create_ms", "shuffle_ms", "build_ms", "fill_ms", "stats_ms", "run_wall_ms", "end_to_end_ms")
KINDS = {  # kind: (shapes, inputs, HOST, NULL, the times reported, those reported with min and max)
    "lookup": (LOOKUP_SHAPES, lookup_inputs, host_lookup, null_lookup, [k for k in TIMES if k != "build_ms"],
               ("fill_ms", "shuffle_ms", "stats_ms")),
    "features": (FEATURE_SHAPES, feature_inputs, host_features, null_features, TIMES,
                 ("fill_ms", "shuffle_ms", "build_ms", "stats_ms")),
    "dense": (DENSE_SHAPES, dense_inputs, host_dense, null_dense, TIMES, TIMES),
}


def cycle(kind, form, items, shared, params, replicas, seed):
    """One prepare + create + run + reduce; -> (times in ms, replica scores [npairs, R], (sums, sumsq), chunks)."""
    from bialign_amd import batch  # noqa: F401  (loaded ahead of the clock)
    _, _, host, null, times, _ = KINDS[kind]
    npairs = len(items)
    t0 = time.perf_counter()
    ms = dict(shuffle_ms=0.0, stats_ms=0.0)
    if form == "host":
        create = host(items, shared, params, replicas, seed)
        t1 = time.perf_counter()
        b = create()
        t2 = time.perf_counter()
        b.run()
        scores = b.scores().reshape(npairs, replicas)
        sums = scores.astype(np.int64).sum(axis=1)
        sumsq = (scores.astype(np.int64) ** 2).sum(axis=1)
    else:
        from bialign_amd import significance
        t1 = time.perf_counter()
        b = null(significance, items, shared, params, replicas, seed)
        t2 = time.perf_counter()
        b.run()
        st = b.null_stats()
        sums, sumsq = st["sum"], st["sumsq"]
    t3 = time.perf_counter()
    if form == "null":
        scores = b.null_scores()   # (for the hash only: not part of the timed cycle)
        ni = b.null_info()
        ms.update(shuffle_ms=ni["shuffle_ms"], stats_ms=ni["stats_ms"])
    ms.update(prepare_ms=(t1 - t0) * 1e3, create_ms=(t2 - t1) * 1e3, fill_ms=b.timing()["fill_ms"],
              run_wall_ms=(t3 - t2) * 1e3, end_to_end_ms=(t3 - t0) * 1e3)
    if "build_ms" in times:
        ms["build_ms"] = b.feature_info()["build_ms"]
    nchunks = b.info["nchunks"]
    b.close()
    return {k: ms[k] for k in times}, scores, (sums, sumsq), nchunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=list(KINDS), default="lookup")
    ap.add_argument("--form", choices=["host", "null"], required=True)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replicas", type=int, default=0, help="default: the shape's")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    shapes, inputs, _, _, _, with_min_max = KINDS[args.kind]
    for key in (shapes if args.shape == "all" else [args.shape]):
        name, npairs, length, s, replicas, extra = shapes[key]
        replicas = args.replicas or replicas
        params, items, shared = inputs(args.form, npairs, length, s, extra)
        cycle(args.kind, args.form, items[:4], shared, params, 4, args.seed)  # warm-up: library, kernels, buffers
        rows, scores, sums = [], None, None
        for _ in range(args.reps):
            row, got, sums, nchunks = cycle(args.kind, args.form, items, shared, params, replicas, args.seed)
            assert scores is None or np.array_equal(scores, got)
            rows.append(row)
            scores = got
        out = dict(shape=name, form=args.form, pairs=npairs, replicas=replicas, nchunks=nchunks, reps=args.reps)
        for k in rows[0]:
            vals = [r[k] for r in rows]
            out[k] = round(float(np.median(vals)), 3)
            if k in with_min_max:
                out[k + "_min_max"] = [round(min(vals), 3), round(max(vals), 3)]
        out["scores_sha"] = digest(scores)
        out["sums_sha"] = digest(np.concatenate(sums))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
