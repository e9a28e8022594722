#!/usr/bin/env python3
"""A/B of the two ways a shuffled null of pairs scored through dense tables (a PSSM as mu1_dense, structure scores
computed outside as mu2_dense) reaches the engine: HOST (numpy permutes the columns of every pair's tables R times with the
permutation of include/bialign.h -- and the letters of a form left in LOOKUP form --, make_batch(score_only=True,
mu1_dense=, mu2_dense=) uploads all R x sum(n * m) entries and keeps them resident, numpy reduces the scores) and NULL
(significance.null_dense_batch: every table uploaded once, the GPU shuffles, permutes the columns chunk by chunk and
reduces).  One form per process.  The HOST form restates the permutation itself (vectorised over all replicas with numpy)
and needs nothing newer than the DENSE forms, so it also runs from a checkout of an older commit (copy this file there):
that is the baseline.  Per shape one JSON line: medians over --reps cycles (after a small warm-up batch) of host
preparation, upload + batch creation, shuffle / build / fill / stats kernel ms, the whole cycle's wall ms -- each with the
min and max of the cycles --, and hashes of the replica scores and of the per-pair sums (equal between the forms).

    python tools/ab_null_dense.py --form host [--shape a|b|all] [--reps 5]
    python tools/ab_null_dense.py --form null [--shape a|b|all] [--reps 5]
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

SHAPES = {  # name: (description, pairs, length, max_shift, replicas, dense forms)
    "a": ("64 protein pairs x len 300, s=2, mu1 and mu2 dense, R=100", 64, 300, 2, 100, ("mu1", "mu2")),
    "b": ("256 protein pairs x len 512, s=1, mu1 dense, R=20", 256, 512, 1, 20, ("mu1",)),
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


def tables_of(seed, n, m):
    """(mu1, mu2) of one pair: a PSSM-like table in the x100 scale of the score tables, structure scores >= 0."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-400, 1100, size=(n, m), dtype=np.int32), rng.integers(0, 800, size=(n, m), dtype=np.int32))


def digest(x):
    return hashlib.sha256(np.asarray(x, dtype=np.int64).tobytes()).hexdigest()[:16]


def cycle(form, pairs, tabs, forms, params, replicas, seed):
    """One prepare + create + run + reduce; -> (times in ms, replica scores [npairs, R], (sums, sumsq), chunks)."""
    from bialign_amd import batch
    npairs = len(pairs)
    dense = {name: [t[i] for t in tabs] for i, name in enumerate(("mu1", "mu2")) if name in forms}
    t0 = time.perf_counter()
    shuffle_ms = stats_ms = 0.0
    if form == "host":
        m = len(pairs[0][1])
        perm = permutations(seed, npairs, replicas, m)
        ext, ext_tabs = [], {name: [] for name in dense}
        for p, (sa, sb, ta, tb) in enumerate(pairs):
            rows = perm[p * replicas:(p + 1) * replicas]
            seqs = np.frombuffer(sb.encode("latin-1"), dtype=np.uint8)[rows]
            strs = np.frombuffer(tb.encode("latin-1"), dtype=np.uint8)[rows]
            for r in range(replicas):
                ext.append((sa, seqs[r].tobytes().decode("latin-1"), ta, strs[r].tobytes().decode("latin-1")))
                for name in dense:
                    ext_tabs[name].append(dense[name][p][:, rows[r]])
        t1 = time.perf_counter()
        b = batch.make_batch(ext, params, score_only=True, mu1_dense=ext_tabs.get("mu1"), mu2_dense=ext_tabs.get("mu2"))
        t2 = time.perf_counter()
        b.run()
        scores = b.scores().reshape(npairs, replicas)
        sums = scores.astype(np.int64).sum(axis=1)
        sumsq = (scores.astype(np.int64) ** 2).sum(axis=1)
    else:
        from bialign_amd import significance
        t1 = time.perf_counter()
        b = significance.null_dense_batch(pairs, params, replicas, seed=seed, mu1_dense=dense.get("mu1"),
                                          mu2_dense=dense.get("mu2"))
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
        name, npairs, length, s, replicas, forms = SHAPES[key]
        params = dict(synth.PROTEIN_PARAMS, max_shift=s)
        pairs = [synth.protein_pair(9100 + t, length) for t in range(npairs)]
        tabs = [tables_of(9100 + t, length, length) for t in range(npairs)]
        cycle(args.form, pairs[:4], tabs[:4], forms, params, 4, args.seed)  # warm-up: library, kernels, buffers
        rows, scores, sums = [], None, None
        for _ in range(args.reps):
            row, got, sums, nchunks = cycle(args.form, pairs, tabs, forms, params, replicas, args.seed)
            assert scores is None or np.array_equal(scores, got)
            rows.append(row)
            scores = got
        out = dict(shape=name, form=args.form, pairs=npairs, replicas=replicas, nchunks=nchunks, reps=args.reps)
        for k in rows[0]:
            vals = [r[k] for r in rows]
            out[k] = round(float(np.median(vals)), 3)
            out[k + "_min_max"] = [round(min(vals), 3), round(max(vals), 3)]
        out["scores_sha"] = digest(scores)
        out["sums_sha"] = digest(np.concatenate(sums))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
