"""Every instantiated sweep and walk, launched once and compared with the oracle: one test per case of
tests/variant_cases.py (tests/test_variant_cases_host.py shows on the CPU that the cases' variants are exactly the ones
bialign_host.hpp instantiates, and that the planner plans each case as it claims).

What launched is asserted from what the library reports: waves per pair, cross-CU, packed records, the storage mode, and no
recovered run (a cross-CU or packed case that fell back would have tested another kernel).  What it computed is compared
exactly: full storage -- score, trace, completeness flag and every band cell of the dumped layers; score-only -- the score;
the lean and level tracebacks -- score, trace and flag; LOCAL with one wave -- score, spans and layers against
tests/local_expected.py; LOCAL with four waves, whose shapes are out of that expectation's reach (10^9 oracle cells) --
bit for bit the one-wave launch of the same inputs, and the score one oracle run of the returned window gives.

A case with a traceback runs a second time, at max_shift >= 1, with shift_cost 0 on planted inputs, where nearly every
column of the trace has several candidates and the reference's tie rule decides every step (the density is a test of
tests/test_variant_cases_host.py).  Oracle runs are cached per (inputs, parameters)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_expected as le
import variant_cases as vc

pytestmark = pytest.mark.gpu

GLOBAL_CASES = [c for c in vc.CASES if not c.local]
LOCAL_ONE = [c for c in vc.CASES if c.local and c.team == "1"]
LOCAL_TEAM = [c for c in vc.CASES if c.local and c.team != "1"]


def ties_of(c):
    return (False, True) if c.tie_dense() else (False,)


def batch_of(c, tie):
    from bialign_amd.batch import make_batch
    t1, t2 = vc.tables_of(c.shape, c.form, tie)
    return make_batch([vc.pair_of(c.shape, c.kind, tie)], c.params(tie), mu1_dense=None if t1 is None else [t1],
                      mu2_dense=None if t2 is None else [t2], score_only=c.storage == "score_only",
                      lean_trace=c.storage == "lean_trace", level_trace=c.storage == "level_trace", local=c.local)


def set_env(monkeypatch, c):
    for name in vc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in c.env:
        monkeypatch.setenv(name, value)


def check_launch(c, b):
    """The launch was the case's: team, records, storage; nothing fell back."""
    t, plan = b.timing(), c.plan()
    print(c.id, {k: t[k] for k in ("waves_per_pair", "cross_cu", "packed_records", "recovered_runs")})
    assert b.current_info()["storage"] == plan["storage"]
    assert t["recovered_runs"] == 0
    assert bool(t["packed_records"]) == bool(plan["pack"])
    if c.wide:
        if "BIALIGN_WIDE_PARTS" in c.environ:
            assert t["cross_cu"] == (c.environ["BIALIGN_WIDE_PARTS"] != "1")
    else:
        assert t["waves_per_pair"] == plan["tw"] * plan["gw"] and t["cross_cu"] == (plan["gw"] > 1)


def same_band_cells(got, want, shape, s):
    ok = le.run_mask(*shape, s)
    assert got.shape == want.shape
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g)[ok], np.asarray(w)[ok])


# ---- global alignments -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def heavy_oracle_runs():
    """The few oracle runs of 5 to 10 s (the largest teams' shapes) start here, on threads beside the tests that come first."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as pool:
        vc.solve_ahead(pool, vc.heavy_runs())
        yield
        vc.drop_ahead()


@pytest.mark.parametrize("c", GLOBAL_CASES, ids=[c.id for c in GLOBAL_CASES])
def test_global_variant(c, monkeypatch):
    from oracle import oracle
    from bialign_amd.engine import trace_codes_to_columns
    set_env(monkeypatch, c)
    for tie in ties_of(c):
        params = c.params(tie)
        ref = vc.oracle_ref(c.inputs(tie), vc.frozen(params))
        b = batch_of(c, tie)
        try:
            b.run(fill_only=c.fill_only)
            check_launch(c, b)
            assert int(b.scores()[0]) == ref["score"], tie
            if c.has_walk():
                traces, ok = b.traces()
                assert trace_codes_to_columns(traces[0]) == oracle.trace_to_lists(ref["trace"]), tie
                assert bool(ok[0]) == ref["complete"], tie
            if c.storage == "full":
                same_band_cells(b.dump_layers(0), ref["layers"], c.shape, c.s)
        finally:
            b.close()


@pytest.mark.parametrize("team", ["2", "x2"])
@pytest.mark.parametrize("form", ["mu2", "mu12"])
@pytest.mark.parametrize("s", [4, 5])
def test_dense_mu2_window_of_a_waves_first_strip(s, form, team, monkeypatch):
    """A lane's window of dense mu2 values starts at column max_shift - 2 il - aa: at max_shift 4 and 5 the first row of a
    wave whose first strip is not strip 0 needs columns 1 (and 2) ahead of its feed.  The cells that read them sit at the
    band's edge of column 1, where random tables seldom let them show: here the first columns of mu2 stand 2000 above the
    rest, so every such cell takes them.  (Before the fix: linear-s4-mu2-...-team2 of the matrix, four cells 100 too low.)"""
    c = vc.case("linear", s, form, team=team)
    set_env(monkeypatch, c)
    from bialign_amd.batch import make_batch
    from oracle import oracle
    t1, t2 = (None if t is None else t.copy() for t in vc.tables_of(c.shape, form))
    t2[:, :3] += 2000
    mu1, mu2 = (np.array(t) for t in oracle.mu_tables(*vc.pair_of(c.shape), c.params()))
    mu2[1:, 1:] = t2
    if t1 is not None:
        mu1[1:, 1:] = t1
    ref = oracle.solve_tables(*c.shape, c.params(), mu1, mu2)
    b = make_batch([vc.pair_of(c.shape)], c.params(), mu1_dense=None if t1 is None else [t1], mu2_dense=[t2])
    try:
        b.run()
        check_launch(c, b)
        assert int(b.scores()[0]) == ref["score"]
        same_band_cells(b.dump_layers(0), ref["layers"], c.shape, s)
    finally:
        b.close()


# ---- local alignments --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def local_ref():
    """{(inputs, parameters): local_expected's dict, windows kept} for every one-wave LOCAL case, in one spawn pool."""
    todo = {}
    for c in LOCAL_ONE:
        for tie in ties_of(c):
            key = (c.inputs(tie), vc.frozen(c.params(tie)))
            todo[key] = (*c.shape, c.params(tie), *vc.mu_tables(*key))
    jobs = [j for key, t in todo.items() for j in le.split_jobs(key, *t, True, True)]
    done = le.pool_map(le.local_partial, jobs)
    return {key: le.local_combine(t[0], t[1], [d for d in done if d[0] == key]) for key, t in todo.items()}


def run_local(c, tie):
    """-> dict(scores, spans, traces, complete, layers) of the case's batch; full storage: the walk and the dump too."""
    b = batch_of(c, tie)
    try:
        b.run()
        check_launch(c, b)
        out = dict(score=int(b.scores()[0]), span=tuple(int(x[0]) for x in b.local_spans()))
        if c.storage == "full":
            traces, ok = b.traces()
            out.update(trace=traces[0].tolist(), complete=bool(ok[0]), layers=b.dump_layers(0).astype(np.int64))
        return out
    finally:
        b.close()


def check_local_window(c, tie, got, score):
    """The span of a full-storage walk is a window inside the molecules whose global score is the local score."""
    n, m = c.shape
    sa, ea, sb, eb = got["span"]
    assert got["complete"] and 0 <= sa <= ea <= n and 0 <= sb <= eb <= m, got["span"]
    if sa < ea and sb < eb:
        assert le.window_global(c.params(tie), *vc.mu_tables(c.inputs(tie), vc.frozen(c.params(tie))), sa, ea, sb, eb) == score
    else:
        assert score == 0 and (sa, sb) == (ea, eb)


@pytest.mark.parametrize("c", LOCAL_ONE, ids=[c.id for c in LOCAL_ONE])
def test_local_variant_one_wave(c, local_ref, monkeypatch):
    set_env(monkeypatch, c)
    for tie in ties_of(c):
        want = local_ref[(c.inputs(tie), vc.frozen(c.params(tie)))]
        got = run_local(c, tie)
        assert got["score"] == want["score"] and (got["span"][1], got["span"][3]) == want["end"], tie
        if c.storage == "full":
            check_local_window(c, tie, got, want["score"])
            assert int(want["windows"][got["span"][0], got["span"][2], got["span"][1], got["span"][3]]) == want["score"]
            le.compare_layers(got["layers"], want["layers"], *c.shape, c.s)
        else:
            assert got["span"][0] == -1 and got["span"][2] == -1      # (the LEAN sweeps keep no starts)


def one_wave_local(c, tie):
    """The one-wave launch of a team case's inputs (the kernel test_local_variant_one_wave holds to the expectation)."""
    return run_local(c._replace(env=tuple((k, "1" if k == "BIALIGN_TEAM" else v) for k, v in c.env)), tie)


@pytest.mark.parametrize("c", LOCAL_TEAM, ids=[c.id for c in LOCAL_TEAM])
def test_local_variant_team(c, monkeypatch):
    for tie in ties_of(c):
        set_env(monkeypatch, c._replace(env=tuple((k, "1" if k == "BIALIGN_TEAM" else v) for k, v in c.env)))
        base = one_wave_local(c, tie)
        set_env(monkeypatch, c)
        got = run_local(c, tie)
        assert got["score"] == base["score"] and got["span"] == base["span"], tie
        if c.storage == "full":
            assert got["trace"] == base["trace"] and got["complete"] == base["complete"], tie
            np.testing.assert_array_equal(got["layers"], base["layers"])
            check_local_window(c, tie, got, got["score"])
