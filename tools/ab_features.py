#!/usr/bin/env python3
"""A/B of the two ways real-valued RNA structure features reach the engine: DENSE (the host computes one int32 n x m
table per pair, scoring.dense_mu2_from_features, and uploads it through make_batch(mu2_dense=)) and FEATURE (three
doubles per residue through make_feature_batch, the GPU builds the tables).  One form per process, so that both sides
have the same process layout; the DENSE form needs nothing newer than dense mu2 and so also runs from a checkout of an
older commit (copy this file there).  Per shape one JSON line: medians over --reps cycles (after a small warm-up batch)
of host preparation, batch creation, table build, fill and traceback kernel ms, the whole cycle's wall ms, and a hash
of the scores (equal between the forms).

    python tools/ab_features.py --form dense   [--shape a|b|c|all] [--reps 5]
    python tools/ab_features.py --form feature [--shape a|b|c|all] [--reps 5]

Shape c (all-against-all, score-only) has 32 640 pairs; the DENSE form would prepare and upload 11.7 GB of tables, so
it runs on the first --dense-pairs pairs only (the line says how many; per-pair figures scale).  The FEATURE form
prints the hash of that subset too.
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

SHAPES = {  # name: (description, molecules, length, max_shift, all-against-all score-only)
    "a": ("256 pairs x len 512, s=1", 512, 512, 1, False),
    "b": ("64 pairs x len 2000, s=2", 128, 2000, 2, False),
    "c": ("all-against-all of 256 x len 300, s=1, score-only", 256, 300, 1, True),
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


def digest(scores):
    return hashlib.sha256(np.asarray(scores, dtype=np.int64).tobytes()).hexdigest()[:16]


def cycle(form, mols, index, params, score_only):
    """One prepare + create + run + read-back; -> (times in ms, scores)."""
    from bialign_amd import batch, scoring
    t0 = time.perf_counter()
    tabs = None
    if form == "dense":
        one_based = lambda f: dict(zip(("up", "down", "unp"), (np.concatenate([[0.0], x]) for x in f)))  # noqa: E731
        feats = [one_based(f) for _, f in mols]
        tabs = [scoring.dense_mu2_from_features(feats[a], feats[b], params["structure_weight"]) for a, b in index]
    t1 = time.perf_counter()
    if form == "dense":
        pairs = [(mols[a][0], mols[b][0], "." * len(mols[a][0]), "." * len(mols[b][0])) for a, b in index]
        b = batch.make_batch(pairs, params, mu2_dense=tabs, score_only=score_only)
    else:
        b = batch.make_feature_batch(mols, index, params, score_only=score_only)
    t2 = time.perf_counter()
    b.run()
    scores = b.scores()
    t3 = time.perf_counter()
    t = b.timing()
    build_ms = b.feature_info()["build_ms"] if form == "feature" else 0.0
    nchunks = b.info["nchunks"]
    b.close()
    return dict(prepare_ms=(t1 - t0) * 1e3, create_ms=(t2 - t1) * 1e3, build_ms=build_ms, fill_ms=t["fill_ms"],
                traceback_ms=t["traceback_ms"], run_wall_ms=(t3 - t2) * 1e3, end_to_end_ms=(t3 - t0) * 1e3), scores, nchunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["dense", "feature"], required=True)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-pairs", type=int, default=2048, help="shape c, DENSE form: pairs of the subset it runs on")
    args = ap.parse_args()
    for key in (SHAPES if args.shape == "all" else [args.shape]):
        name, nmol, length, s, all_pairs = SHAPES[key]
        params = dict(synth.RNA_PARAMS, max_shift=s)
        mols = [molecule(7000 + t, length) for t in range(nmol)]
        index = ([(a, b) for a in range(nmol) for b in range(a + 1, nmol)] if all_pairs
                 else [(2 * t, 2 * t + 1) for t in range(nmol // 2)])
        subset = min(len(index), args.dense_pairs) if all_pairs else len(index)
        if args.form == "dense":
            index = index[:subset]
        cycle(args.form, mols, index[:8], params, all_pairs)  # warm-up: library, kernels, buffers
        rows, scores = [], None
        for _ in range(args.reps):
            row, got, nchunks = cycle(args.form, mols, index, params, all_pairs)
            assert scores is None or np.array_equal(scores, got)
            rows.append(row)
            scores = got
        out = dict(shape=name, form=args.form, pairs=len(index), nchunks=nchunks, reps=args.reps)
        for k in rows[0]:
            vals = [r[k] for r in rows]
            out[k] = round(float(np.median(vals)), 3)
            if k in ("fill_ms", "traceback_ms", "build_ms"):
                out[k + "_min_max"] = [round(min(vals), 3), round(max(vals), 3)]
        out["scores_sha"] = digest(scores[:subset])
        out["subset_pairs"] = subset
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
