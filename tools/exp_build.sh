#!/bin/bash
# Timing-experiment builds of the engine (results are WRONG by construction; never shipped).
# usage: tools/exp_build.sh <output .so> [DEFINE[=value] ...]     e.g.  tools/exp_build.sh /tmp/x.so BIALIGN_EXP=1
# A/B builds with RIGHT results (load with BIALIGN_LIB_OVERRIDE): BIALIGN_SLIM_DPP=0, BIALIGN_BLK_OVERRIDE=<n>,
# BIALIGN_FEED_FAST=0 (the ghost feed without its steady-block fast path: every block recomputes its source addresses),
# BIALIGN_STEP_SCALAR=0 (the three-wave sweep's interior steps with per-lane store and ghost addresses, clamped code
# fetches and the interior test read out of lane 0).
set -e
cd "$(dirname "$0")/.."
out="$1"; shift
python - "$out" "$@" <<'PY'
import sys
from bialign_amd.build import build
print(build(force=True, out=sys.argv[1], defines=sys.argv[2:]))
PY
