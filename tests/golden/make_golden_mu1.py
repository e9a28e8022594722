#!/usr/bin/env python3
"""Golden vectors for position-specific sequence scores (dense mu1, include/bialign.h ABI 10).

The reference's recurrence treats mu1 as an arbitrary function of (i, j): ``BiAligner.mu1`` calls
the plain ``def`` method ``_sequence_similarity`` per cell (bialignment.pyx:435-436, 228, 260).  A
Python subclass of the compiled reference's ``BiAligner`` overrides that method with a seeded
integer table; the reference's own fill and traceback then run unchanged.  Recorded: the table,
parameters, score, trace, completeness and (small cases) all layers.

    python tests/golden/make_golden_mu1.py     # dev container only (the reference builds under /tmp)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from bialign_amd import synth  # noqa: E402


def seeded_table(seed, n, m, lo=-300, hi=900):
    return np.random.default_rng(seed).integers(lo, hi, size=(n, m)).astype(np.int64)


def main():
    ba = mg.build_reference()
    table = {}

    class TableAligner(ba.BiAligner):
        def _sequence_similarity(self, i, j):
            return int(table["t"][i - 1, j - 1])

    out = []
    linear = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
    grid = [  # (kind, seed, n, m, overrides, layers)
        ("rna", 61, 4, 4, dict(max_shift=1), True),
        ("rna", 62, 5, 6, dict(max_shift=2, **linear), True),
        ("rna", 64, 6, 6, dict(max_shift=0), True),
        ("protein", 65, 9, 8, dict(max_shift=1), False),
        ("rna", 63, 14, 13, dict(max_shift=2), False),
        ("protein", 66, 12, 9, dict(max_shift=3, **linear), False),
        ("rna", 67, 30, 24, dict(max_shift=1), False),
        ("rna", 68, 20, 26, dict(max_shift=3), False),
        ("protein", 69, 28, 25, dict(max_shift=2), False),
        ("protein", 70, 22, 18, dict(max_shift=0, **linear), False),
        ("protein", 71, 25, 27, dict(max_shift=1, **linear), False),
        ("rna", 72, 16, 15, dict(max_shift=6), False),
    ]
    for kind, seed, n, m, ov, layers in grid:
        sa, sb, ta, tb = synth.rna_pair(seed, n, m) if kind == "rna" else synth.protein_pair(seed, n, m)
        base = synth.RNA_PARAMS if kind == "rna" else synth.PROTEIN_PARAMS
        params = dict(base, **ov, nameA="A", nameB="B")
        tab = seeded_table(seed, n, m)
        table["t"] = tab
        b = TableAligner(sa, sb, ta, tb, **params)
        rec = dict(name=f"{kind}_mu1_s{seed}_{n}x{m}", seqA=sa, seqB=sb, strA=ta, strB=tb, params=params,
                   mu1=tab.tolist())
        rec["score"] = int(b.optimize())
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            trace = b.traceback()
        rec["trace"] = [[int(v) for v in col] for col in trace]
        rec["complete"] = "WARNING" not in buf.getvalue()
        if layers:
            rec["layers"] = mg.dump_layers(b, n, m, params["max_shift"], params["gap_opening_cost"] != 0)
        out.append(rec)
        print(rec["name"], rec["score"], len(rec["trace"]), rec["complete"])
    with open(os.path.join(HERE, "dense_mu1.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
