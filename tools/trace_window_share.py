"""Share of the affine traceback's columns that its LDS window serves (TraceWindow, bialign_trace_fast.hpp), at the headline
shape: run on a BIALIGN_EXP=10 build (tools/exp_build.sh <so> BIALIGN_EXP=10, loaded through BIALIGN_LIB_OVERRIDE with
BIALIGN_ALLOW_EXPERIMENT_BUILD=10), whose short-chain kernel reports the number of columns read from the window in place
of the pair's score.  WS_PAIRS / WS_LEN."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bialign_amd import synth
from bialign_amd.batch import make_batch
pairs = synth.protein_batch(int(os.environ.get("WS_PAIRS", 1024)), int(os.environ.get("WS_LEN", 1024)))
b = make_batch(pairs, dict(synth.PROTEIN_PARAMS))
b.run()
hits = np.array(b.scores(), dtype=np.int64)
traces, _ = b.traces()
cols = np.array([len(t) for t in traces], dtype=np.int64)
print(f"pairs {len(pairs)} columns {cols.sum()} (mean {cols.mean():.0f}) served from the window {hits.sum()} = {hits.sum() / cols.sum():.4f}"
      f"   per pair min {(hits / cols).min():.4f} max {(hits / cols).max():.4f}")
b.close()
