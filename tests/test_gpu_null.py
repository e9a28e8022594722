"""Null batches (bialign_batch_create_null): shuffles of molecule B made on the GPU, scored by the SCORE_ONLY sweeps,
reduced per pair on the GPU.  The shuffles against the Python mirror of the header's permutation, the scores against
the CPU oracle on the mirrored shuffles (shapes up to 60 x 60), the reduction against numpy, exactly."""
import math

import numpy as np
import pytest

from bialign_amd import significance as sg
from bialign_amd import synth

pytestmark = pytest.mark.gpu

LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
SHAPES = [(3, 55), (55, 3), (17, 31), (40, 22), (28, 28)]   # 5 ragged pairs, lengths 3..55


def run_null(pairs, params, replicas, seed=0, **kw):
    b = sg.null_batch(pairs, params, replicas, seed=seed, **kw)
    b.run()
    out = b.null_scores().copy(), dict(b.current_info()), b.timing()
    b.close()
    return out


# ---- the shuffle against the mirror

@pytest.mark.parametrize("R", [1, 7])
def test_shuffle_equals_mirror(R):
    from bialign_amd.batch import encode_flat
    lens_b = [1, 2, 3, 17, 64, 65, 130]
    pairs = [synth.protein_pair(4000 + t, 9 + t, m) for t, m in enumerate(lens_b)]
    params = dict(synth.PROTEIN_PARAMS)
    _, fb = encode_flat(pairs, params)
    mols_b = fb.molecules("b")
    seed = 77
    b = sg.null_batch(pairs, params, R, seed=seed)
    assert b.info["npairs"] == len(pairs) and b.null_info()["replica_bytes"] == 2 * R * sum(lens_b)
    for when in ("before run", "after run"):
        for p in range(len(pairs)):          # (first and last pair, and every length between)
            for r in sorted({0, R - 1}):
                perm = sg.permutation(seed, p, r, lens_b[p])
                seq, cls = b.dump_null_codes(p, r)
                np.testing.assert_array_equal(seq, mols_b[p][0][perm])
                np.testing.assert_array_equal(cls, mols_b[p][1][perm])   # the class moved with its letter
        b.run()
    b.close()


def test_pairs_sharing_one_b_get_different_shuffles():
    from bialign_amd.batch import encode_flat
    from bialign_amd.engine import Batch, default_engine
    sa, sb, ta, tb = synth.protein_pair(4100, 20, 40)
    params = dict(synth.PROTEIN_PARAMS)
    model, fb = encode_flat([(sa, sb, ta, tb)] * 3, params)
    fb.off_b = np.zeros(3, dtype=np.int64)                      # all three pairs point at the first copy of B
    fb.seq_b, fb.cls_b = fb.seq_b[:40].copy(), fb.cls_b[:40].copy()
    b = Batch(default_engine(), fb, None, model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"],
              params["shift_cost"], params["max_shift"], null=(2, 5))
    got = [[b.dump_null_codes(p, r) for r in range(2)] for p in range(3)]
    b.close()
    for p in range(3):
        for r in range(2):
            perm = sg.permutation(5, p, r, 40)
            np.testing.assert_array_equal(got[p][r][0], fb.seq_b[perm])
            np.testing.assert_array_equal(got[p][r][1], fb.cls_b[perm])
    assert len({got[p][r][0].tobytes() for p in range(3) for r in range(2)}) == 6


# ---- scores against the oracle on the mirrored shuffles

def check_scores_vs_oracle(pairs, params, R, seed):
    from oracle import oracle
    scores, info, _ = run_null(pairs, params, R, seed=seed)
    assert scores.shape == (len(pairs), R) and info["npairs"] == len(pairs)
    assert info["cells"] == R * sum(synth.cells_per_pair(len(p[0]), len(p[1]), params["max_shift"]) for p in pairs)
    for p, pair in enumerate(pairs):
        for r in range(R):
            want = oracle.solve(*sg.shuffle_b(pair, seed, p, r), params, want_trace=False)["score"]
            assert int(scores[p, r]) == want, (p, r)
    return scores


@pytest.mark.parametrize("s", [0, 1, 2, 5])
@pytest.mark.parametrize("ov", [{}, LIN], ids=["affine", "linear"])
def test_scores_equal_oracle(s, ov):
    pairs = [synth.protein_pair(4200 + t, n, m) for t, (n, m) in enumerate(SHAPES)]
    check_scores_vs_oracle(pairs, dict(synth.PROTEIN_PARAMS, max_shift=s, **ov), 4, 11 + s)


def test_scores_equal_oracle_general_beta():
    pairs = [synth.protein_pair(4300 + t, n, m) for t, (n, m) in enumerate(SHAPES)]
    check_scores_vs_oracle(pairs, dict(synth.PROTEIN_PARAMS, gap_opening_cost=100), 4, 3)


def test_scores_equal_oracle_wide_band():
    pairs = [synth.protein_pair(4400 + t, n, m) for t, (n, m) in enumerate(SHAPES)]
    check_scores_vs_oracle(pairs, dict(synth.PROTEIN_PARAMS, max_shift=7), 4, 9)


def test_wide_band_rings_are_cut_into_chunks():
    """The batch of test_scores_equal_oracle_wide_band (20 virtual pairs, rings up to 3.6 MB) under a budget of two rings:
    several chunks, the same null scores, reductions and z-scores."""
    from oracle import oracle
    from wide_ring import check_chunked_null
    pairs = [synth.protein_pair(4400 + t, n, m) for t, (n, m) in enumerate(SHAPES)]
    params, R, seed = dict(synth.PROTEIN_PARAMS, max_shift=7), 4, 9
    want = [[oracle.solve(*sg.shuffle_b(pair, seed, p, r), params, want_trace=False)["score"] for r in range(R)]
            for p, pair in enumerate(pairs)]
    observed = np.array([sorted(row)[R // 2] for row in want], dtype=np.int32)
    check_chunked_null(lambda bud: sg.null_batch(pairs, params, R, seed=seed, hbm_budget_bytes=bud),
                       lambda bud: sg.zscores(pairs, params, replicas=R, seed=seed, hbm_budget_bytes=bud),
                       [n for n, _ in SHAPES], 7, want, observed)


def test_scores_equal_oracle_rna():
    """RNA: what moves with a residue is its structure class.  A shuffled class string is no dot-bracket structure the
    oracle could parse, so the oracle's own mu1 / mu2 tables of the real pair get their B columns permuted."""
    from oracle import oracle
    pairs = [synth.rna_pair(4500 + t, n, m) for t, (n, m) in enumerate([(30, 44), (12, 9), (55, 50), (41, 17), (8, 33)])]
    params = dict(synth.RNA_PARAMS, max_shift=2)
    R, seed = 4, 21
    scores, _, _ = run_null(pairs, params, R, seed=seed)
    for p, pair in enumerate(pairs):
        n, m = len(pair[0]), len(pair[1])
        mu1, mu2 = oracle.mu_tables(*pair, params)
        for r in range(R):
            cols = np.concatenate([[0], 1 + sg.permutation(seed, p, r, m)])
            want = oracle.solve_tables(n, m, params, mu1[:, cols], mu2[:, cols], want_trace=False)["score"]
            assert int(scores[p, r]) == want, (p, r)


# ---- the result does not depend on the plan

def test_independent_of_chunks_and_team(monkeypatch):
    from bialign_amd.batch import make_batch
    pairs = [synth.protein_pair(4600 + t, 300 - 7 * t, 310 + 5 * t) for t in range(3)]
    params = dict(synth.PROTEIN_PARAMS)
    R, seed = 3, 8
    base, info, timing = run_null(pairs, params, R, seed=seed)
    assert info["nchunks"] == 1
    chunked, info_c, _ = run_null(pairs, params, R, seed=seed, hbm_budget_bytes=4 << 20)
    assert info_c["nchunks"] > 1
    np.testing.assert_array_equal(chunked, base)
    monkeypatch.setenv("BIALIGN_TEAM", "1")
    solo, _, timing_1 = run_null(pairs, params, R, seed=seed)
    monkeypatch.delenv("BIALIGN_TEAM")
    assert timing_1["waves_per_pair"] == 1 and timing["waves_per_pair"] > 1
    np.testing.assert_array_equal(solo, base)
    other, _, _ = run_null(pairs, params, R, seed=seed + 1)
    assert not np.array_equal(other, base)
    # the same virtual pairs as an ordinary host-expanded score-only batch of the mirror's shuffles
    b = make_batch([sg.shuffle_b(pair, seed, p, r) for p, pair in enumerate(pairs) for r in range(R)], params, score_only=True)
    b.run()
    np.testing.assert_array_equal(b.scores().reshape(len(pairs), R), base)
    b.close()


# ---- the reduction

@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 200])
def test_stats_equal_numpy(R):
    pairs = [synth.protein_pair(4700 + t, n, m) for t, (n, m) in enumerate([(30, 21), (9, 30), (25, 25)])]
    b = sg.null_batch(pairs, dict(synth.PROTEIN_PARAMS), R, seed=R)
    b.run()
    sc = b.null_scores().astype(np.int64)
    observed = np.array([np.sort(sc[0])[R // 2], sc[1].max() + 1, sc[2].min()], dtype=np.int32)
    for obs in (observed, None):
        st = b.null_stats(obs)
        np.testing.assert_array_equal(st["sum"], sc.sum(axis=1))
        np.testing.assert_array_equal(st["sumsq"], (sc * sc).sum(axis=1))
        np.testing.assert_array_equal(st["min"], sc.min(axis=1))
        np.testing.assert_array_equal(st["max"], sc.max(axis=1))
        np.testing.assert_array_equal(st["replicas"], [R] * 3)
        want = (sc >= observed[:, None].astype(np.int64)).sum(axis=1) if obs is not None else [0, 0, 0]
        np.testing.assert_array_equal(st["n_ge"], want)
    assert st["sum"].dtype == np.int64 and st["sumsq"].dtype == np.int64
    ni = b.null_info()
    assert ni["shuffle_ms"] > 0 and ni["stats_ms"] > 0
    b.close()


def test_stats_equal_python_integers_at_large_scores():
    """test_stats_equal_numpy's scores stay below 46341, where a 32-bit square, or a 32-bit shuffle of a partial sum of
    squares, would pass it.  The same three shapes with every score multiplied by the largest factor the int32 safety
    window admits (tests/window_edge.py): replica scores of 10^6 .. 10^7, 65 replicas (more than a wave's lanes),
    reduced in Python integers."""
    import window_edge as we
    problems = [we.Problem("lookup", n, m, 1, 4700 + t) for t, (n, m) in enumerate([(30, 21), (9, 30), (25, 25)])]
    k, R = we.batch_scale(problems), 65
    assert max(p.product(k) for p in problems) < we.WINDOW <= max(p.product(k + 1) for p in problems)
    b = sg.null_batch([p.pair for p in problems], problems[0].at(k), R, seed=R)
    b.run()
    rows = [[int(v) for v in row] for row in b.null_scores()]
    assert max(abs(v) for v in rows[0]) > 1 << 22
    observed = [sorted(rows[0])[R // 2], max(rows[1]) + 1, min(rows[2])]
    st = b.null_stats(np.array(observed, dtype=np.int32))
    b.close()
    assert [int(v) for v in st["sum"]] == [sum(r) for r in rows]
    assert [int(v) for v in st["sumsq"]] == [sum(v * v for v in r) for r in rows]
    assert [int(v) for v in st["min"]] == [min(r) for r in rows] and [int(v) for v in st["max"]] == [max(r) for r in rows]
    assert [int(v) for v in st["n_ge"]] == [sum(v >= o for v in r) for r, o in zip(rows, observed)]
    assert max(int(v) for v in st["sumsq"]) > 1 << 50


# ---- refusals

def test_refusals():
    from bialign_amd import _lib
    from bialign_amd._lib import BialignError
    from bialign_amd.batch import encode_flat
    from bialign_amd.engine import Batch, default_engine
    import ctypes
    pairs = [synth.protein_pair(4800, 12, 10)]
    params = dict(synth.PROTEIN_PARAMS)
    with pytest.raises(BialignError) as e:   # the one-layer recurrence beyond the tiled band: as SCORE_ONLY there
        sg.null_batch(pairs, dict(params, max_shift=6, **LIN), 3)
    assert e.value.code == _lib.E_UNSUPPORTED
    b = sg.null_batch(pairs, params, 3)
    b.run()
    for call in (b.scores, b.traces, lambda: b.dump_layers(0)):
        with pytest.raises(BialignError) as e:
            call()
        assert e.value.code == _lib.E_INVALID
    b.close()
    # what the Python layer refuses itself, asked of the C ABI directly
    model, fb = encode_flat(pairs, params)
    eng = default_engine()
    ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    s1, s2 = np.ascontiguousarray(model.s1, np.int32), np.ascontiguousarray(model.s2, np.int32)
    sc = _lib.Scoring(s1.shape[0], ptr(s1, ctypes.c_int32), s2.shape[0], ptr(s2, ctypes.c_int32))
    tab, off = np.zeros(120, np.int32), np.zeros(1, np.int64)

    def create(flags=0, replicas=3, dense1=False, dense2=False, spec=True):
        prm = _lib.Params(-150, -50, -150, 1, 0, flags)
        pr = _lib.Pairs(1, ptr(fb.len_a, ctypes.c_int32), ptr(fb.len_b, ctypes.c_int32), ptr(fb.off_a, ctypes.c_int64),
                        ptr(fb.off_b, ctypes.c_int64), ptr(fb.seq_a, ctypes.c_uint8), ptr(fb.cls_a, ctypes.c_uint8),
                        ptr(fb.seq_b, ctypes.c_uint8), ptr(fb.cls_b, ctypes.c_uint8),
                        ptr(tab, ctypes.c_int32) if dense2 else None, ptr(off, ctypes.c_int64) if dense2 else None,
                        ptr(tab, ctypes.c_int32) if dense1 else None, ptr(off, ctypes.c_int64) if dense1 else None)
        h = ctypes.c_void_p()
        rc = _lib.lib.bialign_batch_create_null(eng._h, ctypes.byref(prm), ctypes.byref(sc), ctypes.byref(pr),
                                                ctypes.byref(_lib.NullSpec(replicas, 0)) if spec else None, 0, ctypes.byref(h))
        msg = _lib.lib.bialign_last_error().decode()
        if h:
            _lib.lib.bialign_batch_destroy(h)
        return rc, msg
    assert create()[0] == 0
    assert create(flags=_lib.BATCH_SCORE_ONLY)[0] == 0
    assert create(dense1=True)[0] == _lib.E_UNSUPPORTED and create(dense2=True)[0] == _lib.E_UNSUPPORTED
    assert create(flags=_lib.BATCH_LEAN_TRACE)[0] == _lib.E_INVALID
    assert create(flags=_lib.BATCH_LEVEL_TRACE)[0] == _lib.E_INVALID
    for bad in (0, 65536):
        rc, msg = create(replicas=bad)
        assert rc == _lib.E_INVALID and "replicas" in msg
    rc, msg = create(spec=False)
    assert rc == _lib.E_INVALID and "spec" in msg


# ---- z-scores end to end

def test_zscores_readme_protein(golden_known):
    from oracle import oracle
    rec = next(r for r in golden_known if r["name"] == "readme_protein")
    pair = (rec["seqA"], rec["seqB"], rec["strA"], rec["strB"])
    params = {k: v for k, v in rec["params"].items() if k not in ("nameA", "nameB")}
    R, seed = 50, 2
    z = sg.zscores([pair], params, replicas=R, seed=seed)
    assert int(z["score"][0]) == 48500
    null = [oracle.solve(*sg.shuffle_b(pair, seed, 0, r), params, want_trace=False)["score"] for r in range(R)]
    s1, s2 = sum(null), sum(x * x for x in null)
    mean, std = s1 / R, math.sqrt((R * s2 - s1 * s1) / (R * (R - 1)))
    assert z["mean"][0] == mean and z["std"][0] == std and z["z"][0] == (48500 - mean) / std
    n_ge = sum(x >= 48500 for x in null)
    assert int(z["n_ge"][0]) == n_ge and z["p_emp"][0] == (n_ge + 1) / (R + 1) and int(z["replicas"][0]) == R
    assert z["z"][0] > 5   # two near-identical 42-mers against shuffles


def test_batch_cli_zscore(tmp_path, capsys):
    from bialign_amd import batch_cli
    rows = []
    for t in range(2):
        sa, sb, ta, tb = synth.protein_pair(4900 + t, 20 + 3 * t, 25 - t)
        rows.append(("a%d" % t, sa, ta, "b%d" % t, sb, tb))
    f = tmp_path / "pairs.tsv"
    f.write_text("".join("\t".join(r) + "\n" for r in rows))
    opts = ["--type", "Protein", "--simmatrix", "BLOSUM62", "--gap_opening_cost", "-150", "--gap_cost", "-50",
            "--shift_cost", "-150", "--structure_weight", "800", "--max_shift", "1", "--outmode", "sorted"]
    batch_cli.main([str(f)] + opts)
    plain = capsys.readouterr().out
    batch_cli.main([str(f)] + opts + ["--zscore", "8", "--zscore_seed", "4"])
    with_z = capsys.readouterr().out
    zlines = [ln for ln in with_z.split("\n") if ln.startswith("ZSCORE: ")]
    assert len(zlines) == 2
    assert "\n".join(ln for ln in with_z.split("\n") if not ln.startswith("ZSCORE: ")) == plain
    blocks = with_z.split(">pair ")[1:]
    params = dict(synth.PROTEIN_PARAMS)
    z = sg.zscores([(r[1], r[4], r[2], r[5]) for r in rows], params, replicas=8, seed=4)
    for t in range(2):
        assert blocks[t].rstrip("\n").split("\n")[-1] == zlines[t] == batch_cli.zscore_line(z, t)
        assert zlines[t].endswith("/8 shuffles >= score)")
