"""The scalar addressing of fill_affine_slim_kernel's interior steps (StepAddr, bialign_types.hpp; GhostSrc,
bialign_feed.hpp; the scalar mirrors of lane 0's column and strip) addresses exactly what the per-lane bookkeeping
addresses -- proven on the CPU, from the kernels' own headers, before anything runs on a GPU.

tests/step_addr_check.hip is a stand-alone host program: for (n, m) in (41, 46), (64, 300), (300, 64), (1024, 1024),
(1025, 1023), teams of 1, 2, 3, 6 and 12 waves wherever T * lag + 64 <= P, pair storage on both sides of a 4 GiB boundary,
packed and LEAN records, it walks every wave through its sweep and compares, at every interior step and for all 64 lanes,
scalar base + lane offset + immediate with the per-lane store address, the one-instruction ghost source with the ring entry,
and, at every step, the mirrors with lane 0.  It prints the step counts per case; they are asserted here.  The same program
is built once more with AddressSanitizer and UBSan and must print the same."""
import os

import pytest

import plan_host as ph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "step_addr_check.hip")
SHAPES = [(41, 46), (64, 300), (300, 64), (1024, 1024), (1025, 1023)]
LAG, RR = 72, 20               # max_shift 1: 2 (R - 1) + 2 BLK + 16; lattice rows per strip
LO, Q0 = 44, 1                 # Pack<1>: first interior phase, first strip with interior steps


def _build_and_run(tmp, name, extra):
    return ph.run(ph.build(tmp, SRC, extra, name), "")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("stepaddr"), "check", [])


def _rows(out):
    rows = {}
    for ln in out.splitlines():
        lean, t, n, m, off, steps, interior, runs = map(int, ln.split())
        rows[(lean, t, n, m, off)] = dict(steps=steps, interior=interior, runs=runs)
    return rows


def _teams(m):
    p = max(m + 2, 64)
    return [t for t in (1, 2, 3, 6, 12) if t == 1 or t * LAG + 64 <= p]


def test_scalar_addresses_equal_per_lane_addresses_everywhere(plain):
    rows = _rows(plain)
    offs = sorted({k[4] for k in rows})
    assert len(offs) == 4 and offs[0] == 0 and any(o * 4 < 2 ** 32 < o * 4 + 2 ** 20 for o in offs) \
        and any(2 ** 32 <= o * 4 < 2 ** 32 + 2 ** 20 for o in offs)
    want = {(lean, t, n, m, off) for (n, m) in SHAPES for t in _teams(m) for off in offs for lean in (0, 1)}
    assert set(rows) == want
    assert [len(_teams(m)) for _, m in SHAPES] == [1, 3, 1, 5, 5]
    for (lean, t, n, m, off), r in sorted(rows.items()):
        # every strip from Q0 on holds one interior run, phases LO .. m - 1, whatever the team
        ns = (n + 1 + RR - 1) // RR
        per_strip = max(m - 1 - LO + 1, 0)
        expect = max(ns - Q0, 0) * per_strip
        print(f"lean={lean} T={t} n={n} m={m} off={off}: {r['interior']}/{r['steps']} interior steps in {r['runs']} runs")
        assert r["interior"] == expect, (lean, t, n, m, r, expect)
        assert r["runs"] == (max(ns - Q0, 0) if per_strip else 0)


def test_first_interior_run_is_two_steps(plain):
    """m = 46 is the first m with an interior step (LO = 44 <= m - 1); n = 41 has three strips."""
    rows = _rows(plain)
    r = rows[(0, 1, 41, 46, 0)]
    assert r["runs"] == 2 and r["interior"] == 2 * 2


def test_same_under_address_and_ub_sanitizers(plain, tmp_path):
    out = _build_and_run(tmp_path, "check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert out == plain
