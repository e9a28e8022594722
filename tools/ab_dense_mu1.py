#!/usr/bin/env python3
"""A/B of the score forms on the same pairs: LOOKUP, dense mu2, dense mu1, and both dense.  The dense tables hold
exactly the LOOKUP scores, so all four must give the same scores (asserted).  Prints fill and traceback kernel ms
(median of --reps runs after one warm-up) per shape and form as JSON lines.

    python tools/ab_dense_mu1.py [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bialign_amd import synth  # noqa: E402
from bialign_amd.batch import encode_flat, make_batch  # noqa: E402

SHAPES = [  # (name, kind, pairs, length, max_shift)
    ("protein 256 x len 512, s=1", "protein", 256, 512, 1),
    ("rna 64 x len 2000, s=2", "rna", 64, 2000, 2),
    ("protein 1 x 300x300, s=6", "protein", 1, 300, 6),
]


def tables(pairs, params):
    model, fb = encode_flat(pairs, params)
    mu1, mu2 = [], []
    for (sa, ca), (sb, cb) in zip(fb.molecules("a"), fb.molecules("b")):
        mu1.append(model.s1[np.ix_(sa, sb)].astype(np.int32))
        mu2.append(model.s2[np.ix_(ca, cb)].astype(np.int32))
    return mu1, mu2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for name, kind, npairs, length, s in SHAPES:
        gen = synth.protein_pair if kind == "protein" else synth.rna_pair
        base = synth.PROTEIN_PARAMS if kind == "protein" else synth.RNA_PARAMS
        params = dict(base, max_shift=s)
        pairs = [gen(1000 + p, length, length) for p in range(npairs)]
        mu1, mu2 = tables(pairs, params)
        forms = {"lookup": {}, "dense_mu2": dict(mu2_dense=mu2), "dense_mu1": dict(mu1_dense=mu1),
                 "both": dict(mu1_dense=mu1, mu2_dense=mu2)}
        scores, row = None, dict(shape=name)
        for form, kw in forms.items():
            b = make_batch(pairs, params, **kw)
            fill, tb = [], []
            for rep in range(args.reps + 1):
                b.run()
                t = b.timing()
                if rep:
                    fill.append(t["fill_ms"])
                    tb.append(t["traceback_ms"])
            got = [int(v) for v in b.scores()]
            row[form] = dict(fill_ms=float(np.median(fill)), traceback_ms=float(np.median(tb)),
                             waves_per_pair=t["waves_per_pair"], cross_cu=t["cross_cu"],
                             packed_records=t["packed_records"])
            b.close()
            assert scores is None or got == scores, (name, form)
            scores = got
        row["scores_equal"] = True
        row["dense_mu1_over_dense_mu2_fill"] = row["dense_mu1"]["fill_ms"] / row["dense_mu2"]["fill_ms"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
