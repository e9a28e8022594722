"""The affine traceback's short-chain kernel (bialign_trace_fast.hpp) computes what the generic kernel computes and reads
where the generic kernel reads -- proven on the CPU, from the kernels' own headers, before anything runs on a GPU.

tests/trace_fast_check.hip is a stand-alone host program: it compares every entry of the candidate table with the generic
kernel's per-column expressions (9 states x 15 candidates x every band column, four parameter sets); at every lattice
point of eleven shapes (max_shift 1, 2, 3, n != m, one strip only) and along random walks stepped the way the kernel
steps, the carried row and the 32-bit offsets with packed_addr(), packed_cell's address arithmetic on its own; and
packed_load(packed_addr()) with packed_cell on every in-band cell.  It prints, per shape, how many loads it checked and
how many took the fast path; the coverage is asserted here.  The same program is built once more with AddressSanitizer
and UBSan and must print the same."""
import os

import pytest

import plan_host as ph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "trace_fast_check.hip")
RR = {1: 20, 2: 11, 3: 8}


def _build_and_run(tmp, name, extra):
    return ph.run(ph.build(tmp, SRC, extra, name), "")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("tracefast"), "check", [])


def _rows(out):
    rows = {}
    for ln in out.splitlines():
        s, n, m, points, loads, fast, codes, steps, cells = map(int, ln.split())
        rows[(s, n, m)] = dict(points=points, loads=loads, fast=fast, codes=codes, steps=steps, cells=cells)
    return rows


def test_every_case_ran_and_agreed(plain):
    rows = _rows(plain)
    assert len(rows) == 11
    for key, r in sorted(rows.items()):
        print(key, r)
        assert r["loads"] > 0 and r["steps"] > 0


def test_every_offset_code_from_every_row_on_the_fast_path(plain):
    """15 offset codes x RR lane rows (the wrap at il = 1 among them), per max_shift."""
    rows = _rows(plain)
    for s, n, m in ((1, 130, 97), (1, 70, 140), (2, 41, 120), (3, 37, 90)):
        assert rows[(s, n, m)]["codes"] == 15 * RR[s], (s, n, m, rows[(s, n, m)])


def test_side_path_only_shapes_claim_nothing(plain):
    rows = _rows(plain)
    for key in ((1, 45, 45), (1, 12, 40), (2, 25, 30), (3, 20, 26)):
        assert rows[key]["fast"] == 0
    assert rows[(1, 47, 61)]["fast"] > 0 and rows[(2, 60, 41)]["fast"] > 0


def test_packed_cell_checked_on_every_inband_cell(plain):
    rows = _rows(plain)
    for (s, n, m), r in rows.items():
        if r["cells"]:
            w = 2 * s + 1
            assert r["cells"] <= 2 * 9 * (n + 1) * (m + 1) * w * w and r["cells"] >= 2 * 9 * (n - 2 * s) * (m - 2 * s) * w * w


def test_same_under_address_and_ub_sanitizers(plain, tmp_path):
    out = _build_and_run(tmp_path, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert out == plain
