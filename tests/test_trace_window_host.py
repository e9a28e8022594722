"""The LDS window of the affine traceback's short-chain kernel (TraceWindow, bialign_trace_fast.hpp) serves a column only
with dwords that a DMA has brought, from the very addresses the global path would load, after a wait that covers that DMA --
proven on the CPU, from the kernels' own headers, before anything runs on a GPU.

tests/trace_window_check.hip is a stand-alone host program: it steps the window the way the kernel does, along oracle-like
and adversarial walks and through every sequence of legal moves of bounded length from sampled points, at the GPU tests'
shapes, with the full ring and with the shortest one.  It prints, per shape and ring length, what it walked and how much of
it the window served; the coverage is asserted here.  The same program is built once more with AddressSanitizer and UBSan
and must print the same."""
import os

import pytest

import plan_host as ph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "trace_window_check.hip")
SHAPES = [(1, 45, 70), (1, 64, 64), (1, 41, 130), (1, 130, 41), (1, 130, 97), (1, 70, 140), (2, 100, 100)]


def _build_and_run(tmp, name, extra):
    return ph.run(ph.build(tmp, SRC, extra, name), "")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("tracewindow"), "check", [])


def _rows(out):
    rows = {}
    for ln in out.splitlines():
        s, n, m, k, columns, fast, hits, issued, nodes, dfs_hits = map(int, ln.split())
        rows[(s, n, m, k)] = dict(columns=columns, fast=fast, hits=hits, issued=issued, nodes=nodes, dfs_hits=dfs_hits)
    return rows


def test_every_case_ran_with_both_ring_lengths(plain):
    rows = _rows(plain)
    assert sorted(rows) == sorted([(s, n, m, k) for s, n, m in SHAPES for k in (4, 8)] + [(3, 100, 100, 0)])
    for key, r in sorted(rows.items()):
        print(key, r)
        if key[3]:
            assert r["columns"] > 0 and r["issued"] > 0 and r["nodes"] > 7 ** 5


def test_the_window_serves_columns_and_misses_some(plain):
    """Hits on the walks wherever fast columns exist, hits in the exhaustive search, and fast columns the window does not
    serve (lane row 1, the columns after a strip change) where the walks meet them."""
    rows = _rows(plain)
    for (s, n, m, k), r in rows.items():
        if not k:
            continue
        assert r["hits"] <= r["fast"] <= r["columns"]
        assert (r["hits"] > 0) == (r["fast"] > 0)
        if (n, m) != (130, 41):   # m = 41 < LO + 3: no column is fast at max_shift 1, nothing may be claimed
            assert r["hits"] > 0 and r["dfs_hits"] > 0
        else:
            assert r["fast"] == 0 and r["dfs_hits"] == 0
    assert rows[(1, 130, 97, 8)]["hits"] < rows[(1, 130, 97, 8)]["fast"]
    assert rows[(2, 100, 100, 4)]["hits"] < rows[(2, 100, 100, 4)]["fast"]


def test_no_window_at_max_shift_3(plain):
    """The slot drift of D + 3 records does not fit 32 slots there (TraceWindow::lead_max() < 0)."""
    assert _rows(plain)[(3, 100, 100, 0)]["columns"] == 0


def test_same_under_address_and_ub_sanitizers(plain, tmp_path):
    out = _build_and_run(tmp_path, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert out == plain
