"""Packed layer records where the 16-bit range check decides: one lane record sits exactly at a limit of the range
contract (tests/pack_boundary.py; the case list is verified from the oracle alone by test_pack_boundary_host.py), on
either side of it, at the edges of the interior region and at chosen distances from the sweep's periodic check.
Every case: score, trace, ``complete`` and every in-band cell of all nine dumped layers equal the oracle; the batch
falls back to full records exactly when the verdict says a record of an interior step does not fit.

Dense mu1 is the exception the engine makes on purpose: a batch with mu1 tables is never packed (bialign_plan.hpp, decide_pack:
``!b.dense1`` in the packing policy; fill_affine_kernel: static_assert(!DENSE1 || !PACK)).  Its cases run the same
spikes through full records: results equal the oracle, nothing is packed and nothing needs recovering."""
import functools

import numpy as np
import pytest

import pack_boundary as pb
from pack_boundary import BOTH_SIDES, CASES, CONFINED, CROSS_CU, GHOST_ROW, reference

pytestmark = pytest.mark.gpu

#: kernel shapes at max_shift 1: environment, waves per pair and cross-CU flag that timing() must report
SHAPES = {
    "slim3": (dict(BIALIGN_TEAM="3"), 3, False),                       # fill_affine_slim_kernel (the only one with teams of 3)
    "twowave1": (dict(BIALIGN_TEAM="1", BIALIGN_SLIM="0"), 1, False),  # fill_affine_kernel, one wave
    "x3": (dict(BIALIGN_TEAM="x3"), 3, True),                          # fill_affine_kernel, three one-wave workgroups
    "one": (dict(BIALIGN_TEAM="1"), 1, False),                         # s = 2, 3: fill_affine_kernel, one wave per pair
    "x2": (dict(BIALIGN_TEAM="x2"), 2, True),                          # s = 2, 3: two one-wave workgroups
}


@functools.lru_cache(maxsize=None)
def band_index(n, m, s):
    i, j, a, b = np.meshgrid(np.arange(n + 1), np.arange(m + 1), np.arange(2 * s + 1), np.arange(2 * s + 1), indexing="ij")
    k, l = i + a - s, j + b - s
    return (k >= 0) & (k <= n) & (l >= 0) & (l <= m)


def check_results(b, pair_index, case):
    from oracle import oracle
    from bialign_amd.engine import trace_codes_to_columns
    ref = reference(case)
    traces, ok = b.traces()
    assert int(b.scores()[pair_index]) == ref["score"]
    assert trace_codes_to_columns(traces[pair_index]) == oracle.trace_to_lists(ref["trace"])
    assert bool(ok[pair_index]) == ref["complete"]
    band = band_index(case.n, case.m, case.s)
    got = b.dump_layers(pair_index)
    for st in range(9):
        np.testing.assert_array_equal(got[st][band], ref["layers"][st][band], err_msg=f"layer {st}")


def run_case(case, monkeypatch, shape=None):
    monkeypatch.setenv("BIALIGN_PACK", "1")
    env, waves, xcu = SHAPES[shape] if shape else ({}, None, None)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    verdict = reference(case)["verdict"]
    b = case.make_batch()
    try:
        b.run()
        t = b.timing()
        print(case, shape, dict(recovered_runs=t["recovered_runs"], packed=t["packed_records"], waves=t["waves_per_pair"],
                                xcu=t["cross_cu"]), "expected fallback:", pb.falls_back(verdict))
        if shape and t["packed_records"]:
            # (after a fall-back timing() describes the repeat with full records, whose team the engine picks anew --
            #  the slim kernel does not exist for them; the sibling cases that stay packed pin the shape of the first run)
            assert (t["waves_per_pair"], t["cross_cu"]) == (waves, xcu)
        check_results(b, 0, case)
        if case.family == "mu1":          # never packed (module docstring): nothing to fall back from
            assert not t["packed_records"] and t["recovered_runs"] == 0
        elif pb.falls_back(verdict):      # the hard direction: an overflow the sweep must not miss
            assert t["recovered_runs"] >= 1 and not t["packed_records"]
        else:
            assert t["recovered_runs"] == 0 and t["packed_records"]
    finally:
        b.close()


def shapes_of(case):
    if case.family == "mu1":
        return [None]                                   # never packed: the engine's own choice of a dense-mu1 sweep
    if case.s > 1:
        return ["x2"] if case in CROSS_CU else ["one"]  # (a cross-CU team needs a period of 256 columns: CROSS_CU)
    if case.family == "lookup":
        return ["slim3", "twowave1", "x3"]
    return ["twowave1", "x3"]                           # the slim kernel takes the LOOKUP form only


@pytest.mark.parametrize("name,shape", [(c.name, sh) for c in BOTH_SIDES + CROSS_CU for sh in shapes_of(c)])
def test_both_sides_of_both_limits(name, shape, monkeypatch):
    run_case(CASES[name], monkeypatch, shape)


@pytest.mark.parametrize("name,shape", [(c.name, sh) for c in GHOST_ROW
                                        for sh in (("twowave1", "x3", "slim3") if c.s == 1 else ("one",))])
def test_ghost_row_at_an_extreme_offset_feeds_the_strip_below(name, shape, monkeypatch):
    """Section d, one limit at a time: a bottom-row record holding offset 0xfffe or 0x0000 (two of the four with -2^30
    marks beside it) stays packed and is replayed by the strip below -- cooperative unpack at s = 1, per-lane at s = 2;
    every cell of that strip, like every other, equals the oracle."""
    run_case(CASES[name], monkeypatch, shape)


def confined_shapes(case):
    """Sections b and c run on both s = 1 sweeps: fill_affine_slim_kernel as a team of three (timing() tells it from
    the other kernel by that team size alone) and fill_affine_kernel as one wave.  A case placed in a wave's step count
    (``team``) runs with that team only."""
    return [sh for sh, team in (("slim3", 3), ("twowave1", 1)) if case.tags.get("team", team) == team]


@pytest.mark.parametrize("name,shape", [(c.name, sh) for c in CONFINED for sh in confined_shapes(c)])
def test_one_record_at_the_edges_and_around_the_check(name, shape, monkeypatch):
    """Sections b and c of the case list: the one record that misses by one lies at the first / last interior column,
    in the first interior strip, in row n of the partly filled last strip, in the step before and after a periodic
    check, in the sweep's last interior step, in the first interior step of the last strip, and in a lane row that
    leaves the lattice with the next strip change (where the sweep clears its accumulator); or the spike is oversize
    but lies in steps that store full records, and the batch stays packed."""
    run_case(CASES[name], monkeypatch, shape)


def test_one_pair_of_several_overflows_in_a_chunked_batch(monkeypatch):
    """Three pairs of equal size u (packed) under a budget of 1.75 u: no two fit a chunk, the full records of one pair
    (about 1.5 u) do, so the batch is packed in three chunks of one pair each, in pair order -- the middle pair, the only
    one with a record that misses (by one), is the second chunk.  The batch is re-planned and repeated once; all three
    equal the oracle, traces and dumped layers included."""
    monkeypatch.setenv("BIALIGN_PACK", "1")
    bad = CASES["a-mu2-s1-lo-margin-1"]
    quiet = [pb.Case(f"quiet{seed}", "mu2", 1, seed, bad.n, bad.m, bad.pos, 0) for seed in (5, 6)]
    cases = [quiet[0], bad, quiet[1]]
    assert [pb.falls_back(reference(c)["verdict"]) for c in cases] == [False, True, False]
    probe = pb.make_batch(cases)
    one_chunk = probe.info["hbm_layer_bytes"]
    assert probe.info["nchunks"] == 1
    probe.close()
    b = pb.make_batch(cases, hbm_budget_bytes=int(one_chunk / 3 * 1.75))
    try:
        assert b.info["nchunks"] == 3 and b.info["hbm_layer_bytes"] <= one_chunk / 3 * 1.01   # one pair per chunk
        b.run()
        t = b.timing()
        assert t["recovered_runs"] == 1 and not t["packed_records"]
        for p, case in enumerate(cases):
            check_results(b, p, case)
    finally:
        b.close()
