#!/usr/bin/env python3
"""A/B of the two ways a shuffled null of RNA molecules with real-valued structure features reaches the engine: HOST
(numpy builds npairs x R shuffled copies of every B molecule -- letters and three planes of doubles -- with the
permutation of include/bialign.h, make_feature_batch(score_only=True) checks, encodes and uploads them all, numpy
reduces the scores) and NULL (significance.null_feature_batch: every molecule uploaded once, the GPU shuffles, builds
the tables and reduces).  One form per process.  The HOST form restates the permutation itself (vectorised over all
replicas with numpy) and needs nothing newer than the FEATURE form, so it also runs from a checkout of an older commit
(copy this file there): that is the baseline.  Per shape one JSON line: medians over --reps cycles (after a small
warm-up batch) of host preparation, upload + batch creation, shuffle / build / fill / stats kernel ms, the whole
cycle's wall ms, and hashes of the replica scores and of the per-pair sums (equal between the forms).

    python tools/ab_null_features.py --form host [--shape a|b|all] [--reps 5]
    python tools/ab_null_features.py --form null [--shape a|b|all] [--reps 5]
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

SHAPES = {  # name: (description, pairs, length, max_shift, replicas)
    "a": ("64 RNA pairs x len 300, s=2, R=100", 64, 300, 2, 100),
    "b": ("256 RNA pairs x len 512, s=1, R=20", 256, 512, 1, 20),
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


def digest(x):
    return hashlib.sha256(np.asarray(x, dtype=np.int64).tobytes()).hexdigest()[:16]


def cycle(form, mols, index, params, replicas, seed):
    """One prepare + create + run + reduce; -> (times in ms, replica scores [npairs, R], (sums, sumsq), chunks)."""
    from bialign_amd import batch
    npairs = len(index)
    t0 = time.perf_counter()
    shuffle_ms = stats_ms = 0.0
    if form == "host":
        m = len(mols[index[0][1]][0])
        perm = permutations(seed, npairs, replicas, m)
        ext, idx = list(mols), []
        for p, (ia, ib) in enumerate(index):
            letters = np.frombuffer(mols[ib][0].encode("latin-1"), dtype=np.uint8)
            rows = perm[p * replicas:(p + 1) * replicas]
            seqs = letters[rows]
            planes = [f[rows] for f in mols[ib][1]]
            for r in range(replicas):
                ext.append((seqs[r].tobytes().decode("latin-1"), (planes[0][r], planes[1][r], planes[2][r])))
                idx.append((ia, len(ext) - 1))
        t1 = time.perf_counter()
        b = batch.make_feature_batch(ext, idx, params, score_only=True)
        t2 = time.perf_counter()
        b.run()
        scores = b.scores().reshape(npairs, replicas)
        sums = scores.astype(np.int64).sum(axis=1)
        sumsq = (scores.astype(np.int64) ** 2).sum(axis=1)
    else:
        from bialign_amd import significance
        t1 = time.perf_counter()
        b = significance.null_feature_batch(mols, index, params, replicas, seed=seed)
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
    build_ms = b.feature_info()["build_ms"]
    nchunks = b.info["nchunks"]
    b.close()
    return dict(prepare_ms=(t1 - t0) * 1e3, create_ms=(t2 - t1) * 1e3, shuffle_ms=shuffle_ms, build_ms=build_ms,
                fill_ms=t["fill_ms"], stats_ms=stats_ms, run_wall_ms=(t3 - t2) * 1e3,
                end_to_end_ms=(t3 - t0) * 1e3), scores, (sums, sumsq), nchunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["host", "null"], required=True)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    for key in (SHAPES if args.shape == "all" else [args.shape]):
        name, npairs, length, s, replicas = SHAPES[key]
        params = dict(synth.RNA_PARAMS, max_shift=s)
        mols = [molecule(9000 + t, length) for t in range(2 * npairs)]
        index = [(2 * t, 2 * t + 1) for t in range(npairs)]
        cycle(args.form, mols, index[:4], params, 4, args.seed)  # warm-up: library, kernels, buffers
        rows, scores, sums = [], None, None
        for _ in range(args.reps):
            row, got, sums, nchunks = cycle(args.form, mols, index, params, replicas, args.seed)
            assert scores is None or np.array_equal(scores, got)
            rows.append(row)
            scores = got
        out = dict(shape=name, form=args.form, pairs=npairs, replicas=replicas, nchunks=nchunks, reps=args.reps)
        for k in rows[0]:
            vals = [r[k] for r in rows]
            out[k] = round(float(np.median(vals)), 3)
            if k in ("fill_ms", "shuffle_ms", "build_ms", "stats_ms"):
                out[k + "_min_max"] = [round(min(vals), 3), round(max(vals), 3)]
        out["scores_sha"] = digest(scores)
        out["sums_sha"] = digest(np.concatenate(sums))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
