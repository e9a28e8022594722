"""Times of the hit search ("What it costs"): one process, one workload, one JSON line.

    python tools/hit_search_times.py --workload {uniform,planted} [--peaks] [--permille N] [--runs 3]

``uniform``: 1024 protein pairs x len 1024, max_shift 1, affine, FIT, ``max_hits`` 4, ``max_walks`` 16, ``min_score`` nine
tenths of the batch's smallest fit score.  ``planted``: A 256 against B 1024 with three planted copies, 1024 pairs,
``min_score`` half the smallest fit score.  The line holds ``search_ms`` of every timed run behind a warm-up run, hits and
walks per pair, the stop reasons' counts, and a hash of every hit record and walk log.  Without ``--peaks`` and
``--permille`` only what the first hit search had is called, so the script also runs against an older checkout of the
package (``PYTHONPATH``) to compare libraries.
"""
import argparse
import collections
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.append(REPO)   # (behind PYTHONPATH: another checkout of the package named there wins)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("uniform", "planted"), required=True)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--peaks", action="store_true")
    ap.add_argument("--permille", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import bialign_amd
    from bialign_amd import synth
    from bialign_amd.batch import make_batch
    params = dict(synth.PROTEIN_PARAMS, max_shift=1)
    if args.workload == "uniform":
        pairs, tenths = synth.protein_batch(args.pairs, 1024, seed0=1000), 9
    else:
        from hits_expected import multi_planted_pair
        pairs, tenths = [multi_planted_pair("protein", 7000 + t, 256, 1024, 3)[0] for t in range(args.pairs)], 5
    b = make_batch(pairs, params, fit=True)
    b.run()
    min_score = max(1, int(b.scores().min()) * tenths // 10)
    new = dict(peaks=True) if args.peaks else {}
    if args.permille:
        new["min_permille"] = args.permille
    b.set_hits(4, min_score, 16, **new)
    b.run()   # the warm-up run
    times = []
    for _ in range(args.runs):
        b.run()
        times.append(round(b.hit_info()["search_ms"], 3))
    hits, status = b.fit_hits()
    walks = b.fit_hit_walks()
    t = b.timing()
    b.close()
    h = hashlib.sha256()
    for p in range(len(pairs)):
        h.update(repr(([x[:3] for x in hits[p]], [bytes(x[3]) for x in hits[p]], walks[p], status[p])).encode())
    print(json.dumps(dict(label=args.label, package=os.path.dirname(bialign_amd.__file__), workload=args.workload, peaks=args.peaks,
                          permille=args.permille, min_score=min_score, search_ms=times, fill_ms=round(t["fill_ms"], 2),
                          traceback_ms=round(t["traceback_ms"], 3), hits_per_pair=round(sum(map(len, hits)) / len(pairs), 3),
                          walks_per_pair=round(sum(map(len, walks)) / len(pairs), 3), status=dict(collections.Counter(status)),
                          sha256=h.hexdigest()[:16])))


if __name__ == "__main__":
    main()
