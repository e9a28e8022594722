"""The dinucleotide null model on the GPU (bialign_batch_set_null_model, BIALIGN_NULL_DINUCLEOTIDE): the replicas of all
three forms of null batch against the Python mirror of the header's DINUCLEOTIDE PERMUTATION, their scores against the CPU
oracle and against host-expanded batches of the mirror's shuffles, the reduction against numpy, the way back to the mono
model, and the refusals.  All comparisons exact."""
import math
import os
import random

import numpy as np
import pytest

from bialign_amd import significance as sg
from bialign_amd import synth

pytestmark = pytest.mark.gpu

LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
DI = "dinucleotide"
LENS_B = [1, 2, 3, 4, 64, 65, 66, 129, 200]   # edges: none .. 3, 63, 64, 65 (the 64-lane blocks), two blocks, three and a bit


def few_letter_pair(seed, n, m, letters="ARND"):
    """A protein pair over few letters: pairs of neighbours repeat, so the dinucleotide shuffle has room to move."""
    rng = random.Random(seed)
    draw = lambda alpha, k: "".join(rng.choice(alpha) for _ in range(k))
    return draw(letters, n), draw(letters, m), draw("HECT", n), draw("HECT", m)


def codes_b(pairs, params):
    from bialign_amd.batch import encode_flat
    return encode_flat(pairs, params)[1].molecules("b")


def check_codes(b, pairs, params, seed, replicas, tree_cap=sg.TREE_CAP, msg=""):
    mols_b = codes_b(pairs, params)
    for p, pair in enumerate(pairs):
        for r in replicas:
            perm = sg.dinucleotide_permutation(seed, p, r, pair[1], tree_cap=tree_cap)
            seq, cls = b.dump_null_codes(p, r)
            np.testing.assert_array_equal(seq, mols_b[p][0][perm], err_msg=f"{msg} p={p} r={r}")
            np.testing.assert_array_equal(cls, mols_b[p][1][perm], err_msg=f"{msg} p={p} r={r}")   # the class moved with its position


# ---- 1. the replicas against the mirror

def test_codes_equal_mirror_rna():
    pairs = [synth.rna_pair(9000 + t, 9 + t, m) for t, m in enumerate(LENS_B)]
    params, R, seed = dict(synth.RNA_PARAMS), 7, 77
    b = sg.null_batch(pairs, params, R, seed=seed, shuffle=DI)
    assert b.null_model == DI and b.null_info()["replica_bytes"] == 2 * R * sum(LENS_B)
    for when in ("before run", "after run"):
        check_codes(b, pairs, params, seed, range(R), msg=when)
        b.run()
    b.close()


def test_codes_equal_mirror_special_molecules():
    one_letter = ("ARND", "G" * 70, "HECT", "H" * 30 + "E" * 40)
    last_once = few_letter_pair(9100, 5, 90, "AR")
    last_once = (last_once[0], last_once[1][:-1] + "W", last_once[2], last_once[3])   # z has no exit
    protein = synth.protein_pair(9101, 12, 50)                                        # 20 letters
    skewed = ("ARND", "A" * 40 + "C" + "A" * 40, "HECT", "HE" * 40 + "C")
    pairs = [one_letter, last_once, protein, skewed]
    params, R, seed = dict(synth.PROTEIN_PARAMS), 7, 5
    b = sg.null_batch(pairs, params, R, seed=seed, shuffle=DI)
    check_codes(b, pairs, params, seed, range(R))
    b.close()
    assert sg.dinucleotide_permutation(seed, 0, 3, one_letter[1]).tolist() != list(range(70))   # a one-letter B still moves its classes


def test_pairs_sharing_one_b_get_different_replicas():
    from bialign_amd.batch import encode_flat
    from bialign_amd.engine import Batch, default_engine
    pair = few_letter_pair(9200, 20, 40)
    params = dict(synth.PROTEIN_PARAMS)
    model, fb = encode_flat([pair] * 3, params)
    fb.off_b = np.zeros(3, dtype=np.int64)                      # all three pairs point at the first copy of B
    fb.seq_b, fb.cls_b = fb.seq_b[:40].copy(), fb.cls_b[:40].copy()
    b = Batch(default_engine(), fb, None, model.s1, model.s2, params["gap_opening_cost"], params["gap_cost"],
              params["shift_cost"], params["max_shift"], null=(2, 5))
    b.set_null_model(DI)
    got = [[b.dump_null_codes(p, r) for r in range(2)] for p in range(3)]
    b.close()
    for p in range(3):
        for r in range(2):
            perm = sg.dinucleotide_permutation(5, p, r, pair[1])
            np.testing.assert_array_equal(got[p][r][0], fb.seq_b[perm])
            np.testing.assert_array_equal(got[p][r][1], fb.cls_b[perm])
    assert len({got[p][r][1].tobytes() + got[p][r][0].tobytes() for p in range(3) for r in range(2)}) == 6


def test_tree_cap_zero_takes_the_fallback(monkeypatch):
    pairs = [synth.rna_pair(9300 + t, 8, m) for t, m in enumerate([3, 40, 65, 130])]
    params, R, seed = dict(synth.RNA_PARAMS), 7, 9
    b = sg.null_batch(pairs, params, R, seed=seed, shuffle=DI)
    monkeypatch.setenv("BIALIGN_NULL_TREE_CAP", "0")
    check_codes(b, pairs, params, seed, range(R), tree_cap=0)
    monkeypatch.delenv("BIALIGN_NULL_TREE_CAP")
    check_codes(b, pairs, params, seed, range(R))
    b.close()
    assert any(sg._dinucleotide(seed, p, 0, pair[1], 0)[2] for p, pair in enumerate(pairs))   # ... and it was the fallback


def test_feature_form_equals_mirror():
    rng = np.random.default_rng(9400)
    mols, lens_b = [], [2, 3, 65, 130]
    for t, m in enumerate(lens_b):
        for k in (7 + t, m):
            mols.append(("".join(rng.choice(list("ACGU"), size=k)), tuple(rng.random(k) for _ in range(3))))
    index = [(2 * t, 2 * t + 1) for t in range(len(lens_b))]
    params, R, seed = dict(synth.RNA_PARAMS), 7, 31
    from bialign_amd.scoring import ScoreModel
    model = ScoreModel(params, sequences=[s for s, _ in mols], structures=["."])
    b = sg.null_feature_batch(mols, index, params, R, seed=seed, shuffle=DI)
    for when in ("before run", "after run"):
        for p, (_, ib) in enumerate(index):
            for r in range(R):
                perm = sg.dinucleotide_permutation(seed, p, r, mols[ib][0])
                seq, cls = b.dump_null_codes(p, r)
                np.testing.assert_array_equal(seq, model.encode_sequence(mols[ib][0])[perm], err_msg=f"{when} p={p} r={r}")
                assert not cls.any()
                want_seq, want = sg.shuffle_features(mols[ib][0], mols[ib][1], seed, p, r, shuffle=DI)
                assert want_seq == "".join(mols[ib][0][x] for x in perm)
                for g, w, src in zip(b.dump_null_features(p, r), want, mols[ib][1]):
                    np.testing.assert_array_equal(g.view(np.uint64), w.view(np.uint64), err_msg=f"{when} p={p} r={r}")
                    np.testing.assert_array_equal(g.view(np.uint64), src[perm].view(np.uint64))   # bit for bit the gather
        b.run()
    b.close()


def test_dense_form_equals_mirror():
    shapes = [(5, 3), (16, 64), (17, 65), (33, 130)]
    pairs = [few_letter_pair(9500 + t, n, m) for t, (n, m) in enumerate(shapes)]
    params, R, seed = dict(synth.PROTEIN_PARAMS), 7, 13
    mu2 = [-(np.arange(n, dtype=np.int32)[:, None] * 1000 + np.arange(m, dtype=np.int32)[None, :]) for n, m in shapes]
    mols_b = codes_b(pairs, params)
    b = sg.null_dense_batch(pairs, params, R, seed=seed, mu2_dense=mu2, shuffle=DI)   # mu2 dense, mu1 LOOKUP: B has letters
    for when in ("before run", "after run"):
        for p, pair in enumerate(pairs):
            for r in range(R):
                perm = sg.dinucleotide_permutation(seed, p, r, pair[1])
                got1, got2 = b.null_tables(p, r)
                assert got1 is None
                np.testing.assert_array_equal(got2, mu2[p][:, perm], err_msg=f"{when} p={p} r={r}")
                np.testing.assert_array_equal(got2, sg.shuffle_tables(mu2[p], seed, p, r, shuffle=DI, letters=pair[1]))
                seq, cls = b.dump_null_codes(p, r)
                np.testing.assert_array_equal(seq, mols_b[p][0][perm])
                assert not cls.any()
        b.run()
    b.close()


# ---- 2. the scores

SCORED = [(22, 50), (25, 47), (19, 53)]


def run_null(pairs, params, R, seed, **kw):
    b = sg.null_batch(pairs, params, R, seed=seed, shuffle=DI, **kw)
    b.run()
    out = b.null_scores().copy(), dict(b.current_info()), b.timing()
    b.close()
    return out


@pytest.mark.parametrize("s", [0, 1, 2])
@pytest.mark.parametrize("ov", [{}, LIN], ids=["affine", "linear"])
def test_scores_equal_oracle(s, ov):
    """RNA: a shuffled class string is no dot-bracket structure the oracle could parse, so the oracle's own mu1 / mu2
    tables of the real pair get their B columns permuted by the mirror."""
    from oracle import oracle
    pairs = [synth.rna_pair(9600 + t, n, m) for t, (n, m) in enumerate(SCORED)]
    params = dict(synth.RNA_PARAMS, max_shift=s, **ov)
    R, seed = 3, 40 + s
    scores, info, _ = run_null(pairs, params, R, seed)
    assert scores.shape == (len(pairs), R) and info["npairs"] == len(pairs)
    for p, pair in enumerate(pairs):
        n, m = len(pair[0]), len(pair[1])
        mu1, mu2 = oracle.mu_tables(*pair, params)
        for r in range(R):
            cols = np.concatenate([[0], 1 + sg.dinucleotide_permutation(seed, p, r, pair[1])])
            want = oracle.solve_tables(n, m, params, mu1[:, cols], mu2[:, cols], want_trace=False)["score"]
            assert int(scores[p, r]) == want, (p, r)


def test_wide_band_rings_are_cut_into_chunks():
    """The pairs of test_gpu_null.test_scores_equal_oracle_wide_band (max_shift 7) under the dinucleotide model and a budget
    of two rings: several chunks, the same null scores as unbudgeted and as the oracle on the mirror's shuffles, the same
    reductions and z-scores."""
    from oracle import oracle
    from wide_ring import check_chunked_null
    shapes = [(3, 55), (55, 3), (17, 31), (40, 22), (28, 28)]
    pairs = [synth.protein_pair(4400 + t, n, m) for t, (n, m) in enumerate(shapes)]
    params, R, seed = dict(synth.PROTEIN_PARAMS, max_shift=7), 4, 9
    want = [[oracle.solve(*sg.shuffle_b(pair, seed, p, r, shuffle=DI), params, want_trace=False)["score"] for r in range(R)]
            for p, pair in enumerate(pairs)]
    observed = np.array([sorted(row)[R // 2] for row in want], dtype=np.int32)
    check_chunked_null(lambda bud: sg.null_batch(pairs, params, R, seed=seed, shuffle=DI, hbm_budget_bytes=bud),
                       lambda bud: sg.zscores(pairs, params, replicas=R, seed=seed, shuffle=DI, hbm_budget_bytes=bud),
                       [n for n, _ in shapes], 7, want, observed)


@pytest.mark.parametrize("mode", ["fit", "local"])
def test_free_end_modes_equal_host_expanded_batch(mode):
    from bialign_amd.batch import make_batch
    pairs = [few_letter_pair(9700 + t, n, m) for t, (n, m) in enumerate(SCORED)]
    params, R, seed = dict(synth.PROTEIN_PARAMS), 3, 6
    scores, _, _ = run_null(pairs, params, R, seed, **{mode: True})
    b = make_batch([sg.shuffle_b(pair, seed, p, r, shuffle=DI) for p, pair in enumerate(pairs) for r in range(R)], params,
                   score_only=True, **{mode: True})
    b.run()
    np.testing.assert_array_equal(b.scores().reshape(len(pairs), R), scores)
    b.close()


def test_independent_of_chunks_and_team(monkeypatch):
    pairs = [few_letter_pair(9800 + t, 300 - 7 * t, 310 + 5 * t) for t in range(3)]
    params, R, seed = dict(synth.PROTEIN_PARAMS), 3, 8
    base, info, timing = run_null(pairs, params, R, seed)
    assert info["nchunks"] == 1
    chunked, info_c, _ = run_null(pairs, params, R, seed, hbm_budget_bytes=4 << 20)
    assert info_c["nchunks"] > 1
    np.testing.assert_array_equal(chunked, base)
    monkeypatch.setenv("BIALIGN_TEAM", "1")
    solo, _, timing_1 = run_null(pairs, params, R, seed)
    monkeypatch.delenv("BIALIGN_TEAM")
    assert timing_1["waves_per_pair"] == 1 and timing["waves_per_pair"] > 1
    np.testing.assert_array_equal(solo, base)
    mono = sg.null_batch(pairs, params, R, seed=seed)
    mono.run()
    assert not np.array_equal(mono.null_scores(), base)
    mono.close()


def test_stats_and_zscores_equal_numpy():
    pairs = [synth.rna_pair(9900 + t, n, m) for t, (n, m) in enumerate(SCORED)]
    params, R, seed = dict(synth.RNA_PARAMS), 65, 3
    b = sg.null_batch(pairs, params, R, seed=seed, shuffle=DI)
    b.run()
    sc = b.null_scores().astype(np.int64)
    observed = np.array([np.sort(sc[0])[R // 2], sc[1].max() + 1, sc[2].min()], dtype=np.int32)
    st = b.null_stats(observed)
    assert b.null_info()["shuffle_ms"] > 0
    b.close()
    np.testing.assert_array_equal(st["sum"], sc.sum(axis=1))
    np.testing.assert_array_equal(st["sumsq"], (sc * sc).sum(axis=1))
    np.testing.assert_array_equal(st["min"], sc.min(axis=1))
    np.testing.assert_array_equal(st["max"], sc.max(axis=1))
    np.testing.assert_array_equal(st["n_ge"], (sc >= observed[:, None].astype(np.int64)).sum(axis=1))
    z = sg.zscores(pairs, params, replicas=R, seed=seed, shuffle=DI)
    plain = sg.zscores(pairs, params, replicas=R, seed=seed)
    np.testing.assert_array_equal(z["score"], plain["score"])          # the observed batch does not depend on the model
    assert not np.array_equal(z["mean"], plain["mean"])
    for p in range(len(pairs)):
        null = [int(v) for v in sc[p]]
        s1, s2 = sum(null), sum(x * x for x in null)
        mean, std = s1 / R, math.sqrt((R * s2 - s1 * s1) / (R * (R - 1)))
        assert z["mean"][p] == mean and z["std"][p] == std and z["z"][p] == (int(z["score"][p]) - mean) / std
        assert int(z["n_ge"][p]) == sum(x >= int(z["score"][p]) for x in null) and int(z["replicas"][p]) == R


# ---- 3. the model of a batch: there and back, and the refusals

def test_back_to_mono_reproduces_todays_replicas():
    pairs = [synth.rna_pair(10000 + t, 15, m) for t, m in enumerate([40, 66])]
    params, R, seed = dict(synth.RNA_PARAMS), 4, 12
    mols_b = codes_b(pairs, params)
    plain = sg.null_batch(pairs, params, R, seed=seed)
    assert plain.null_model == "mono"
    plain.run()
    want = plain.null_scores().copy()
    plain.close()
    b = sg.null_batch(pairs, params, R, seed=seed, shuffle=DI)
    b.run()
    assert not np.array_equal(b.null_scores(), want)
    b.set_null_model("mono")
    assert b.null_model == "mono"
    for p in range(len(pairs)):
        for r in range(R):
            perm = sg.permutation(seed, p, r, len(pairs[p][1]))
            seq, cls = b.dump_null_codes(p, r)
            np.testing.assert_array_equal(seq, mols_b[p][0][perm])
            np.testing.assert_array_equal(cls, mols_b[p][1][perm])
    b.run()
    np.testing.assert_array_equal(b.null_scores(), want)
    b.set_null_model(1)
    check_codes(b, pairs, params, seed, range(R))
    b.close()


def test_refusals():
    import ctypes
    from bialign_amd import _lib
    from bialign_amd._lib import BialignError
    from bialign_amd.batch import make_batch
    params = dict(synth.PROTEIN_PARAMS)
    pair = few_letter_pair(10100, 12, 30)
    # not a null batch
    plain = make_batch([pair], params, score_only=True)
    assert _lib.lib.bialign_batch_set_null_model(plain._h, 1) == _lib.E_INVALID
    model = ctypes.c_int32(-7)
    assert _lib.lib.bialign_batch_get_null_model(plain._h, ctypes.byref(model)) == _lib.E_INVALID
    plain.run()          # (still usable)
    plain.close()
    # an unknown model: the batch keeps its model and runs
    b = sg.null_batch([pair], params, 3, seed=2, shuffle=DI)
    for bad in (2, -1):
        with pytest.raises(BialignError) as e:
            b.set_null_model(bad)
        assert e.value.code == _lib.E_INVALID
    assert b.null_model == DI
    check_codes(b, [pair], params, 2, range(3))
    b.close()
    # a dense mu1: B has no letters
    tab = [np.arange(12 * 30, dtype=np.int32).reshape(12, 30)]
    d = sg.null_dense_batch([pair], params, 3, seed=2, mu1_dense=tab)
    with pytest.raises(BialignError) as e:
        d.set_null_model(DI)
    assert e.value.code == _lib.E_UNSUPPORTED and "letters" in e.value.message
    assert d.null_model == "mono"
    np.testing.assert_array_equal(d.null_tables(0, 1)[0], sg.shuffle_tables(tab[0], 2, 0, 1))
    d.run()
    d.close()
    with pytest.raises(BialignError) as e:      # ... and through the keyword, which closes the batch it made
        sg.null_dense_batch([pair], params, 3, seed=2, mu1_dense=tab, shuffle=DI)
    assert e.value.code == _lib.E_UNSUPPORTED
    # a B molecule beyond the kernel's LDS layout: n = 1, R = 1, refused before any launch, mono still runs
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bialign.h")) as fh:
        bound = int(fh.read().split("#define BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN ")[1].split()[0])
    assert bound >= 30000
    long_b = few_letter_pair(10101, 1, bound + 1)
    lb = sg.null_batch([long_b], params, 1, seed=2)
    with pytest.raises(BialignError) as e:
        lb.set_null_model(DI)
    assert e.value.code == _lib.E_UNSUPPORTED and str(bound) in e.value.message
    assert lb.null_model == "mono"
    seq, _ = lb.dump_null_codes(0, 0)
    np.testing.assert_array_equal(seq, codes_b([long_b], params)[0][0][sg.permutation(2, 0, 0, bound + 1)])
    lb.close()
    promised = [few_letter_pair(10102, 1, 30000)]          # the length the header promises: taken, and shuffled right
    ok = sg.null_batch(promised, params, 1, seed=2, shuffle=DI)
    check_codes(ok, promised, params, 2, [0])
    ok.close()


def test_batch_cli_zscore_shuffle(tmp_path, capsys):
    from bialign_amd import batch_cli
    rows = []
    for t in range(2):
        sa, sb, ta, tb = few_letter_pair(10200 + t, 20 + 3 * t, 25 - t)
        rows.append(("a%d" % t, sa, ta, "b%d" % t, sb, tb))
    f = tmp_path / "pairs.tsv"
    f.write_text("".join("\t".join(r) + "\n" for r in rows))
    opts = ["--type", "Protein", "--simmatrix", "BLOSUM62", "--gap_opening_cost", "-150", "--gap_cost", "-50",
            "--shift_cost", "-150", "--structure_weight", "800", "--max_shift", "1", "--outmode", "sorted"]
    batch_cli.main([str(f)] + opts)
    plain = capsys.readouterr().out
    batch_cli.main([str(f)] + opts + ["--zscore", "5", "--zscore_shuffle", "dinucleotide"])
    out = capsys.readouterr().out
    assert out.split("\n")[0] == "#zscore_shuffle\tdinucleotide"            # the header line names the model
    zlines = [ln for ln in out.split("\n") if ln.startswith("ZSCORE: ")]
    assert "\n".join(ln for ln in out.split("\n")[1:] if not ln.startswith("ZSCORE: ")) == plain
    z = sg.zscores([(r[1], r[4], r[2], r[5]) for r in rows], dict(synth.PROTEIN_PARAMS), replicas=5, shuffle=DI)
    assert zlines == [batch_cli.zscore_line(z, t) for t in range(2)]
