"""Every DP path at the admitted edge of the int32 safety window (tests/window_edge.py; the cases are verified from
the oracle alone by test_window_edge_host.py): all scores of a problem multiplied by the largest k the host's check
admits, so that finite values reach 2^23 .. 2^26.4 -- bits the rest of the suite never sets -- and "-infinity" cells
drift by up to 5 % of 2^28.  Every comparison is exact: score, trace, completeness flag and, wherever the path can
dump them, every in-band cell of every layer against the CPU oracle; the null reductions against Python integers.
One step further, at k + 1, the same input is refused with BIALIGN_E_RANGE: the mirror and the C formula agree on
both sides."""
import contextlib
import io

import numpy as np
import pytest

import window_edge as we

pytestmark = pytest.mark.gpu


def ids(problems):
    return [p.name for p in problems]


def check(b, index, p, k=None, layers=True, traces=True):
    """Pair ``index`` of a run batch against the oracle's solve of problem p at scale k."""
    from bialign_amd.engine import trace_codes_to_columns
    ref = p.reference(k)
    assert int(b.scores()[index]) == ref["score"]
    if traces:
        tr, ok = b.traces()
        assert trace_codes_to_columns(tr[index]) == ref["trace"]
        assert bool(ok[index]) == ref["complete"]
    if layers:
        band = we.band_index(p.n, p.m, p.s)
        got = b.dump_layers(index)
        assert got.shape == ref["layers"].shape
        for st in range(len(got)):
            np.testing.assert_array_equal(got[st][band], ref["layers"][st][band], err_msg=f"layer {st}")


def run_and_check(p, layers=True, traces=True, **kw):
    b = p.make_batch(**kw)
    try:
        b.run()
        check(b, 0, p, layers=layers, traces=traces)
        return b.timing(), b.current_info()
    finally:
        b.close()


# ---- 1. tiled full layers ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", we.TILED + we.EXTREMES, ids=ids(we.TILED + we.EXTREMES))
def test_tiled_full_layers(p):
    """max_shift 0 .. 5, one strip and several, affine / one-layer / beta > 0 sweeps, and the two constant-table inputs
    that realise most of the bound (finite values up to 0.336 * 2^28)."""
    t, info = run_and_check(p)
    assert info["storage"] == 0 and not t["packed_records"] and t["recovered_runs"] == 0


# ---- 2. teams and kernel variants ------------------------------------------------------------------------------------

#: name -> (problem, environment, waves per pair and cross-CU flag that timing() must report for the run with full records)
VARIANTS = {
    "team1": (we.TEAM_S1, dict(BIALIGN_TEAM="1"), 1, False),
    "team2": (we.TEAM_S1, dict(BIALIGN_TEAM="2"), 2, False),
    "team3": (we.TEAM_S1, dict(BIALIGN_TEAM="3"), 2, False),   # full records: the two-wave kernel, teams in powers of two
    "team4": (we.TEAM4_S1, dict(BIALIGN_TEAM="4"), 4, False),
    "x3": (we.TEAM_S1, dict(BIALIGN_TEAM="x3"), 3, True),
    "team1-slim0": (we.TEAM_S1, dict(BIALIGN_TEAM="1", BIALIGN_SLIM="0"), 1, False),
    "team2-slim0": (we.TEAM_S1, dict(BIALIGN_TEAM="2", BIALIGN_SLIM="0"), 2, False),
    "team3-slim1": (we.TEAM_S1, dict(BIALIGN_TEAM="3", BIALIGN_SLIM="1"), 2, False),
    "eight-wave-s2": (we.EIGHT_WAVE_S2, dict(BIALIGN_TEAM="8"), 8, False),
}


@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_team_and_kernel_variants(variant, pack, monkeypatch):
    """BIALIGN_PACK=1: the first sweep stores packed records (at s = 1 in teams of 2 and 3 it is fill_affine_slim_kernel
    unless BIALIGN_SLIM=0), whose 16-bit offsets cannot hold scores of this scale: the sweep must notice at any
    magnitude of the record's base, the run is repeated once with full records and the batch stays unpacked -- the
    bookkeeping of test_offsets_that_do_not_fit_fall_back.  Either way the results equal the oracle."""
    p, env, waves, xcu = VARIANTS[variant]
    monkeypatch.setenv("BIALIGN_PACK", pack)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    b = p.make_batch()
    try:
        b.run()
        t = b.timing()
        print(variant, pack, t)
        assert (t["waves_per_pair"], t["cross_cu"]) == (waves, xcu)
        assert not t["packed_records"]
        if pack == "1":
            assert t["recovered_runs"] >= 1, "scores of this scale were meant to overflow the 16-bit offsets"
        else:
            assert t["recovered_runs"] == 0
        check(b, 0, p)
        b.run()
        assert b.timing()["recovered_runs"] == t["recovered_runs"] and not b.timing()["packed_records"]   # no second repeat
        check(b, 0, p, layers=False)
    finally:
        b.close()


# ---- 3. reduced storage ------------------------------------------------------------------------------------------------

def reduced_env(p, monkeypatch, slim=None):
    """s = 1 LOOKUP with beta <= 0: the reduced-storage sweeps of fill_affine_slim_kernel in teams of three (or, with
    BIALIGN_SLIM=0, the two-wave kernel in teams of two) -> the waves per pair timing() must report, or None."""
    if not (p.s == 1 and p.costs == "affine"):
        return None
    monkeypatch.setenv("BIALIGN_TEAM", "2" if slim == "0" else "3")
    if slim is not None:
        monkeypatch.setenv("BIALIGN_SLIM", slim)
    return 2 if slim == "0" else 3


SCORE_ONLY = [(p, None) for p in we.REDUCED] + [(p, "0") for p in we.REDUCED if p.s == 1 and p.costs == "affine"]


@pytest.mark.parametrize("p,slim", SCORE_ONLY, ids=[p.name + ("-slim0" if slim else "") for p, slim in SCORE_ONLY])
def test_score_only(p, slim, monkeypatch):
    waves = reduced_env(p, monkeypatch, slim)
    t, info = run_and_check(p, layers=False, traces=False, score_only=True)
    assert info["storage"] == 1
    if waves:
        assert t["waves_per_pair"] == waves


@pytest.mark.parametrize("resw", ["1", "32"])
@pytest.mark.parametrize("p", we.REDUCED, ids=ids(we.REDUCED))
def test_lean_trace(p, resw, monkeypatch):
    monkeypatch.setenv("BIALIGN_RESW_K", resw)
    reduced_env(p, monkeypatch)
    t, info = run_and_check(p, layers=False, lean_trace=True)
    assert info["storage"] == 2


@pytest.mark.parametrize("p", we.REDUCED, ids=ids(we.REDUCED))
def test_tiny_budget_falls_back_to_lean_trace(p):
    probe = p.make_batch()
    budget = int(probe.info["hbm_layer_bytes"] * 0.6)
    assert probe.info["storage"] == 0
    probe.close()
    t, info = run_and_check(p, layers=False, hbm_budget_bytes=budget)
    assert info["storage"] == 2      # BIALIGN_BATCH_LEAN_TRACE, chosen by the engine


def test_ragged_chunked_batch_scaled_by_its_longest_pair():
    """Eight pairs of lengths 1 .. 100 at the scale the longest admits, in one launch and in chunks."""
    k = we.batch_scale(we.RAGGED)
    for budget in (0, 5 << 20):
        b = we.make_batch(we.RAGGED, hbm_budget_bytes=budget)
        try:
            assert (b.info["nchunks"] > 1) == bool(budget)
            b.run()
            for t, p in enumerate(we.RAGGED):
                check(b, t, p, k, layers=(p.n + p.m >= 100))
        finally:
            b.close()


# ---- 4. wide band ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", we.WIDE, ids=ids(we.WIDE))
def test_wide_band_full_layers(p):
    t, info = run_and_check(p)
    assert info["storage"] == 0


@pytest.mark.parametrize("p", [q for q in we.WIDE if q.costs != "linear"], ids=ids([q for q in we.WIDE if q.costs != "linear"]))
def test_wide_band_score_only(p):
    """The ring of derived values (affine recurrence, beta of either sign)."""
    t, info = run_and_check(p, layers=False, traces=False, score_only=True)
    assert info["storage"] == 1


@pytest.mark.parametrize("parts", ["1", "3"])
@pytest.mark.parametrize("p", we.WIDE, ids=ids(we.WIDE))
def test_wide_band_level_trace(p, parts, monkeypatch):
    monkeypatch.setenv("BIALIGN_WIDE_SEG", "8")
    monkeypatch.setenv("BIALIGN_WIDE_PARTS", parts)
    t, info = run_and_check(p, layers=False, level_trace=True)
    assert info["storage"] == 4 and t["cross_cu"] == (parts != "1")


# ---- 5. forms ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", we.FORMS, ids=ids(we.FORMS))
def test_forms_full_layers(p):
    """Dense mu1, dense mu2, both, the FEATURE form (the GPU builds the table: every entry against the host's) and RNA
    LOOKUP."""
    b = p.make_batch()
    try:
        b.run()
        form = b.feature_info()["form"]
        assert form == {"mu1": "lookup", "rna": "lookup", "mu2": "dense", "mu12": "dense", "feature": "feature"}[p.form]
        if p.form == "feature":
            np.testing.assert_array_equal(b.dump_mu2(0), p.tables(p.k)[1][1:, 1:])
        check(b, 0, p)
    finally:
        b.close()


def test_bialigner_and_cli_end_to_end(capsys):
    from bialign_amd import bialignment as ba, cli
    p = we.DROPIN
    ref, prm = p.reference(), p.at(p.k)
    al = ba.BiAligner(*p.pair, nameA="A", nameB="B", outmode="default", nodescription=False, **prm)
    assert int(al.optimize()) == ref["score"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        trace = al.traceback()
    assert [[int(v) for v in col] for col in trace] == ref["trace"]
    assert ("WARNING" not in buf.getvalue()) == ref["complete"]
    lines = al.decode_trace()
    capsys.readouterr()
    sa, sb, ta, tb = p.pair
    cli.main([sa, sb, "--strA", ta, "--strB", tb, "--type", "Protein"] +
             [x for key in ("sequence_match_similarity", "sequence_mismatch_similarity", "structure_weight",
                            "gap_opening_cost", "gap_cost", "shift_cost", "max_shift") for x in ("--" + key, str(prm[key]))])
    out = capsys.readouterr().out.split("\n")
    assert "SCORE: %d" % ref["score"] in out
    assert out[out.index("SCORE: %d" % ref["score"]) + 2:][:len(lines)] == list(lines)
    # one step further the CLI reports the engine's refusal
    with pytest.raises(SystemExit):
        prm = p.at(p.k + 1)
        cli.main([sa, sb, "--strA", ta, "--strB", tb, "--type", "Protein"] +
                 [x for key in ("sequence_match_similarity", "sequence_mismatch_similarity", "structure_weight",
                                "gap_opening_cost", "gap_cost", "shift_cost", "max_shift") for x in ("--" + key, str(prm[key]))])
    assert "safety window" in capsys.readouterr().out


# ---- 6. both sides of the check ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", we.BOTH_SIDES, ids=ids(we.BOTH_SIDES))
def test_admitted_at_k_refused_at_k_plus_one(p):
    """The C formula and the mirror agree on the last admitted scale of every form: k is created (and run: scores and
    traces equal the oracle), k + 1 is BIALIGN_E_RANGE."""
    from bialign_amd import _lib
    assert p.product(p.k) < we.WINDOW <= p.product(p.k + 1)
    run_and_check(p, layers=False)
    with pytest.raises(_lib.BialignError) as e:
        p.make_batch(p.k + 1).close()
    assert e.value.code == _lib.E_RANGE and "safety window" in e.value.message


# ---- 7. null batches ---------------------------------------------------------------------------------------------------------

def python_stats(scores, observed):
    rows = [[int(v) for v in row] for row in scores]
    return dict(sum=[sum(r) for r in rows], sumsq=[sum(v * v for v in r) for r in rows], min=[min(r) for r in rows],
                max=[max(r) for r in rows], n_ge=[sum(v >= o for v in r) for r, o in zip(rows, observed)])


def null_run(p, replicas, seed, k=None, observed=None):
    b = p.null_batch(replicas, seed, k)
    try:
        b.run()
        scores = b.null_scores().copy()
        obs = [int(np.sort(scores[0])[replicas // 2])] if observed is None else observed
        st = b.null_stats(np.array(obs, dtype=np.int32))
        assert st["sum"].dtype == np.int64 and st["sumsq"].dtype == np.int64
        return scores, {key: [int(v) for v in st[key]] for key in ("sum", "sumsq", "min", "max", "n_ge")}, obs
    finally:
        b.close()


@pytest.mark.parametrize("p", we.NULL, ids=ids(we.NULL))
def test_null_batch_at_the_edge(p):
    """Replica scores against the oracle on the mirror's permutations; the GPU's reductions against Python integers (a
    score here is 200 x beyond 46341: its square does not fit 32 bits, nor does a partial sum of two); and, where
    scaling is exact, sum_k == k sum_1 and sumsq_k == k^2 sumsq_1 for the same seed."""
    R, seed, k = 6, 31, p.k
    scores, st, obs = null_run(p, R, seed)
    assert scores.shape == (1, R)
    for r in range(R):
        assert int(scores[0, r]) == p.replica_score(k, seed, 0, r), r
    assert min(abs(int(v)) for v in scores[0]) > 1 << 22
    assert st == python_stats(scores, obs)
    if p.form not in ("rna", "feature"):
        scores1, st1, _ = null_run(p, R, seed, k=1, observed=[0])
        assert [int(v) for v in scores[0]] == [k * int(v) for v in scores1[0]]
        assert st["sum"] == [k * st1["sum"][0]] and st["sumsq"] == [k * k * st1["sumsq"][0]]
        assert st["min"] == [k * st1["min"][0]] and st["max"] == [k * st1["max"][0]]


@pytest.mark.parametrize("p", we.NULL[:3], ids=ids(we.NULL[:3]))
def test_sum_of_squares_check_on_both_sides(p):
    """replicas * bound^2 <= INT64_MAX with the window's bound on |score|: about 128 replicas at the edge.  The last
    admitted count runs (its reductions exact), one more is BIALIGN_E_RANGE naming the sum of squares."""
    from bialign_amd import _lib
    bound = p.product(p.k)
    rmax = we.sumsq_max_replicas(bound)
    assert 127 <= rmax <= 130 and rmax * bound * bound <= we.INT64_MAX < (rmax + 1) * bound * bound
    scores, st, obs = null_run(p, rmax, 5)
    assert scores.shape == (1, rmax) and st == python_stats(scores, obs)
    assert st["sumsq"][0] > rmax << 44          # (every score beyond 2^22)
    with pytest.raises(_lib.BialignError) as e:
        p.null_batch(rmax + 1, 5).close()
    assert e.value.code == _lib.E_RANGE and "sum of squares" in e.value.message
