#!/usr/bin/env python3
"""A/B of the two ways a shuffled null reaches the engine: HOST (Python builds npairs x R shuffled B strings with the
permutation of include/bialign.h, make_batch encodes and uploads them, an ordinary SCORE_ONLY batch scores them, numpy
reduces the scores) and NULL (significance.null_batch: B uploaded once, the GPU shuffles and reduces).  One form per
process.  The HOST form restates the permutation itself (vectorised over all replicas with numpy) and needs nothing
newer than SCORE_ONLY, so it also runs from a checkout of an older commit (copy this file there) or against an older
build of the library (BIALIGN_LIB_OVERRIDE).  Per shape one JSON line: medians over --reps cycles (after a small
warm-up batch) of host preparation, batch creation, shuffle / fill / stats kernel ms, the whole cycle's wall ms, and
hashes of the replica scores and of the per-pair sums (equal between the forms).

    python tools/ab_null.py --form host [--shape a|b|all] [--reps 5] [--replicas 100]
    python tools/ab_null.py --form null [--shape a|b|all] [--reps 5] [--replicas 100]
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

SHAPES = {  # name: (description, pairs, length, max_shift, RNA)
    "a": ("256 protein pairs x len 512, s=1", 256, 512, 1, False),
    "b": ("64 RNA pairs x len 300, s=2", 64, 300, 2, True),
}
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


def rna_class_letters(structure):
    """A dot-bracket string as per-position class letters: what a shuffle moves (significance.shuffle_b, rna=True)."""
    from bialign_amd.scoring import rna_classes
    return "".join(".()"[c] for c in rna_classes(structure).tolist())


def cycle(form, pairs, params, replicas, seed, rna):
    """One prepare + create + run + reduce; -> (times in ms, replica scores [npairs, R], per-pair sums)."""
    from bialign_amd import batch
    npairs, m = len(pairs), len(pairs[0][1])
    t0 = time.perf_counter()
    shuffle_ms = stats_ms = 0.0
    if form == "host":
        perm = permutations(seed, npairs, replicas, m)
        virtual = []
        for p, (sa, sb, ta, tb) in enumerate(pairs):
            seq, cls = np.frombuffer(sb.encode("latin-1"), dtype=np.uint8), np.frombuffer(tb.encode("latin-1"), dtype=np.uint8)
            rows = perm[p * replicas:(p + 1) * replicas]
            for sq, cl in zip(seq[rows], cls[rows]):
                virtual.append((sa, sq.tobytes().decode("latin-1"), ta, cl.tobytes().decode("latin-1")))
        t1 = time.perf_counter()
        if rna:   # (a shuffled class string is no structure: the classes go in as a protein-style alphabet of three letters)
            params = dict(params, type="Protein", simmatrix=None)
        b = batch.make_batch(virtual, params, score_only=True)
        t2 = time.perf_counter()
        b.run()
        scores = b.scores().reshape(npairs, replicas)
        sums = scores.astype(np.int64).sum(axis=1)
        sumsq = (scores.astype(np.int64) ** 2).sum(axis=1)
    else:
        from bialign_amd import significance
        t1 = time.perf_counter()
        b = significance.null_batch(pairs, params, replicas, seed=seed)
        t2 = time.perf_counter()
        b.run()
        st = b.null_stats()
        sums, sumsq = st["sum"], st["sumsq"]
    t3 = time.perf_counter()
    if form == "null":
        scores = b.null_scores()   # (for the hash only: not part of the timed cycle)
        ni = b.null_info()
        shuffle_ms, stats_ms = ni["shuffle_ms"], ni["stats_ms"]
    t = b.timing()
    nchunks = b.info["nchunks"]
    b.close()
    return dict(prepare_ms=(t1 - t0) * 1e3, create_ms=(t2 - t1) * 1e3, shuffle_ms=shuffle_ms, fill_ms=t["fill_ms"],
                stats_ms=stats_ms, run_wall_ms=(t3 - t2) * 1e3, end_to_end_ms=(t3 - t0) * 1e3), scores, (sums, sumsq), nchunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["host", "null"], required=True)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replicas", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    for key in (SHAPES if args.shape == "all" else [args.shape]):
        name, npairs, length, s, rna = SHAPES[key]
        if rna:
            params = dict(synth.RNA_PARAMS, max_shift=s)
            pairs = synth.rna_batch(npairs, length)
            if args.form == "host":   # the structure as class letters, as the shuffles will carry it
                pairs = [(sa, sb, rna_class_letters(ta), rna_class_letters(tb)) for sa, sb, ta, tb in pairs]
        else:
            params = dict(synth.PROTEIN_PARAMS, max_shift=s)
            pairs = synth.protein_batch(npairs, length)
        cycle(args.form, pairs[:4], params, 4, args.seed, rna)  # warm-up: library, kernels, buffers
        rows, scores, sums = [], None, None
        for _ in range(args.reps):
            row, got, sums, nchunks = cycle(args.form, pairs, params, args.replicas, args.seed, rna)
            assert scores is None or np.array_equal(scores, got)
            rows.append(row)
            scores = got
        out = dict(shape=name, form=args.form, pairs=npairs, replicas=args.replicas, nchunks=nchunks, reps=args.reps)
        for k in rows[0]:
            vals = [r[k] for r in rows]
            out[k] = round(float(np.median(vals)), 3)
            if k in ("fill_ms", "shuffle_ms", "stats_ms"):
                out[k + "_min_max"] = [round(min(vals), 3), round(max(vals), 3)]
        out["scores_sha"] = digest(scores)
        out["sums_sha"] = digest(np.concatenate(sums))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
