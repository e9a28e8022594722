"""The ghost feed's steady-block fast path (GhostFeed::steady / steady_base_dword / lane_offset, bialign_feed.hpp) addresses
exactly what the general path addresses -- proven on the CPU, from the kernels' own headers, before anything runs on a GPU.

tests/feed_fastpath_check.hip is a stand-alone host program: for max_shift 1, 2, 3 (and the half-length blocks of the
s=2 DIET ring), teams of 1, 2, 3 and 6 waves, every wave, and every block its sweep prefetches, it compares base + lane offset
with the factored general source dword for all 64 lanes of every DMA round wherever steady() holds, and checks that the
unpack's per-entry test agrees that the whole block is packed.  It prints the steady share per case; the shares are
asserted here.  The same program is built once more with AddressSanitizer and UBSan and must print the same."""
import os

import pytest

import plan_host as ph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "feed_fastpath_check.hip")
# the small shapes of tests/test_gpu_feed_fastpath.py and the largest team each admits (T * 72 + 64 <= P, two strips a wave)
GPU_SHAPES = {(61, 256): 2, (110, 280): 3, (221, 500): 6}


def _build_and_run(tmp, name, extra):
    return ph.run(ph.build(tmp, SRC, extra, name), "")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("feedfast"), "check", [])


def _rows(out):
    rows = {}
    for ln in out.splitlines():
        s, blk, t, n, m, blocks, steady, steady_hi, unsteady_hi = map(int, ln.split())
        rows[(s, blk, t, n, m)] = dict(blocks=blocks, steady=steady, steady_hi=steady_hi, unsteady_hi=unsteady_hi)
    return rows


def test_fast_path_equals_general_path_everywhere(plain):
    rows = _rows(plain)
    # every case ran: 8 shapes x 4 teams x (s=1, s=2, s=2 DIET, s=3)
    assert len(rows) == 8 * 4 * 4
    for (s, blk, t, n, m), r in sorted(rows.items()):
        print(f"s={s} BLK={blk} T={t} n={n} m={m}: {r['steady']}/{r['blocks']} steady = {r['steady'] / r['blocks']:.3f}")
    for shape in [(110, 280), (61, 256), (221, 500), (1024, 1024)]:
        for s, blk in ((1, 8), (2, 4), (2, 2), (3, 4)):
            for t in (1, 2, 3, 6):
                assert rows[(s, blk, t, *shape)]["steady"] > 0


def test_steady_share_at_the_headline(plain):
    r = _rows(plain)[(1, 8, 3, 1024, 1024)]
    share = r["steady"] / r["blocks"]
    print(f"headline (1024 x 1024, max_shift 1, teams of 3): {r['steady']}/{r['blocks']} = {share:.4f}")
    assert share >= 0.85


def test_gpu_shapes_take_both_paths_beyond_the_first_strips(plain):
    rows = _rows(plain)
    for (n, m), tmax in GPU_SHAPES.items():
        for t in (1, 2, 3, 4, 6):
            if t > tmax or (1, 8, t, n, m) not in rows:
                continue
            r = rows[(1, 8, t, n, m)]
            assert r["steady_hi"] >= 1 and r["unsteady_hi"] >= 1, (n, m, t, r)
    # ... and the shape that must have no steady block at all has none
    for t in (1, 2, 3, 6):
        assert rows[(1, 8, t, 61, 46)]["steady"] == 0


def test_same_under_address_and_ub_sanitizers(plain, tmp_path):
    out = _build_and_run(tmp_path, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert out == plain
