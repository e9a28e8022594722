"""GPU tests of the FEATURE form of mu2 (include/bialign.h, bialign_features; bialign_mu2_build.hpp): the GPU builds
the RNA structure-score tables from three doubles per residue.  Every comparison is exact (integers, ==): against
the golden vectors of the compiled reference, against the DENSE form fed with the host's table of the same
features (scoring.dense_mu2_from_features, itself pinned to the reference in test_mu2_features_host.py), and
against the oracle."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from bialign_amd import synth

pytestmark = pytest.mark.gpu

FEATURES = load_golden("fractional_features.json")
LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
KEYS = ("up", "down", "unp")


def fractional(seed, n):
    """(up, down, unp), 0-based float64 arrays, in the distribution of tests/golden/make_golden_features.py's
    fractional_features: a probability split per residue, some entries exactly 0 or 1."""
    rng = np.random.default_rng(seed)
    raw = rng.dirichlet([0.6, 0.6, 0.9], size=n)
    kind = rng.integers(0, 6, size=n)
    up, down = raw[:, 0].copy(), raw[:, 1].copy()
    up[kind == 0] = 0.0
    down[kind == 1] = 0.0
    up[kind == 2], down[kind == 2] = 0.0, 0.0
    return up, down, 1.0 - up - down


def host_table(fa, fb, sw):
    from bialign_amd.scoring import dense_mu2_from_features
    one_based = lambda f: {k: np.concatenate([[0.0], np.asarray(v, dtype=np.float64)]) for k, v in zip(KEYS, f)}  # noqa: E731
    return dense_mu2_from_features(one_based(fa), one_based(fb), sw)


def rna_seq(seed, n):
    return "".join(np.random.default_rng(seed).choice(list("ACGU"), size=n))


def collect(b, traces=True, layers_of=None, mu2_of=()):
    from bialign_amd.engine import trace_codes_to_columns
    out = dict(scores=[int(v) for v in b.scores()], timing=b.timing(), info=b.current_info(), finfo=b.feature_info())
    if traces:
        tr, ok = b.traces()
        out["traces"], out["complete"] = [trace_codes_to_columns(t) for t in tr], [bool(v) for v in ok]
    if layers_of is not None:
        out["layers"] = b.dump_layers(layers_of)
    out["mu2"] = {p: b.dump_mu2(p) for p in mu2_of}
    b.close()
    return out


def run_feature(mols, index, params, traces=True, layers_of=None, mu2_of=(), wait=True, **kw):
    from bialign_amd.batch import make_feature_batch
    b = make_feature_batch(mols, index, params, **kw)
    b.run(wait=wait)
    if not wait:
        b.wait()
    return collect(b, traces, layers_of, mu2_of)


def run_dense(mols, index, params, traces=True, layers_of=None, mu2_of=(), **kw):
    from bialign_amd.batch import make_batch
    sw = params["structure_weight"]
    pairs = [(mols[a][0], mols[b][0], "." * len(mols[a][0]), "." * len(mols[b][0])) for a, b in index]
    tabs = [host_table(mols[a][1], mols[b][1], sw) for a, b in index]
    b = make_batch(pairs, params, mu2_dense=tabs, **kw)
    b.run()
    return collect(b, traces, layers_of, mu2_of), tabs


def same_results(f, d, traces=True):
    assert f["scores"] == d["scores"]
    if traces:
        assert f["traces"] == d["traces"] and f["complete"] == d["complete"]
    assert f["finfo"]["form"] == "feature" and d["finfo"]["form"] == "dense"
    assert f["finfo"]["build_launches"] == f["info"]["nchunks"] and d["finfo"]["build_launches"] == 0


# ---------------------------------------------------------------- goldens of the compiled reference
@pytest.mark.parametrize("rec", FEATURES, ids=[r["name"] for r in FEATURES])
def test_golden_through_the_c_abi(rec):
    from oracle import oracle
    n, m, p = len(rec["seqA"]), len(rec["seqB"]), rec["params"]
    mols = [(rec["seqA"], tuple(rec["featuresA"][k][1:] for k in KEYS)),
            (rec["seqB"], tuple(rec["featuresB"][k][1:] for k in KEYS))]
    got = run_feature(mols, [(0, 1)], p, layers_of=0, mu2_of=(0,))
    assert got["mu2"][0].tolist() == rec["mu2"]
    assert got["scores"][0] == rec["score"]
    assert got["traces"][0] == rec["trace"]
    assert got["complete"][0] == rec["complete"]
    if "layers" in rec:
        for g, e in zip(oracle.band_values(got["layers"], n, m, p["max_shift"]), rec["layers"]):
            np.testing.assert_array_equal(g, np.array(e, dtype=np.int64))


@pytest.mark.parametrize("rec", FEATURES, ids=[r["name"] for r in FEATURES])
def test_golden_through_bialigner(rec):
    """The drop-in class sends fractional features in FEATURE form (no host table)."""
    import contextlib
    import io
    from bialign_amd import bialignment as ba, scoring
    feats = {rec["seqA"]: rec["featuresA"], rec["seqB"]: rec["featuresB"]}

    class FeatureAligner(ba.BiAligner):
        def _preprocess_seq(self, sequence, structure):
            mol = super()._preprocess_seq(sequence, structure)
            f = feats[str(sequence)]
            mol["up"], mol["down"], mol["unp"] = f["up"], f["down"], f["unp"]
            return mol

    def no_host_table(*a, **k):
        raise AssertionError("BiAligner built the mu2 table on the host")
    b = FeatureAligner(rec["seqA"], rec["seqB"], rec["strA"], rec["strB"], **rec["params"])
    orig, scoring.dense_mu2_from_features = scoring.dense_mu2_from_features, no_host_table
    try:
        assert int(b.optimize()) == rec["score"]
    finally:
        scoring.dense_mu2_from_features = orig
    assert b._batch.feature_info()["form"] == "feature"
    assert b._batch.dump_mu2(0).tolist() == rec["mu2"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        trace = b.traceback()
    assert [[int(v) for v in col] for col in trace] == rec["trace"]
    assert ("WARNING" not in buf.getvalue()) == rec["complete"]


# ---------------------------------------------------------------- FEATURE form against DENSE form
def two_molecules(seed, n, m):
    return [(rna_seq(seed, n), fractional(seed * 2, n)), (rna_seq(seed + 500, m), fractional(seed * 2 + 1, m))]


@pytest.mark.parametrize("n,m,s,ov,kw", [
    (70, 63, 0, {}, {}), (130, 64, 1, {}, {}), (75, 65, 2, {}, {}), (61, 200, 3, {}, {}), (40, 50, 4, {}, {}),
    (33, 45, 5, {}, {}), (45, 1, 1, {}, {}), (1, 1, 1, {}, {}), (1, 63, 2, {}, {}),
    (70, 63, 0, LIN, {}), (130, 64, 1, LIN, {}), (75, 65, 2, LIN, {}), (61, 200, 3, LIN, {}), (40, 50, 4, LIN, {}),
    (33, 45, 5, LIN, {}), (64, 1, 1, LIN, {}),
    (129, 200, 1, dict(gap_opening_cost=100), {}),
    (30, 33, 6, {}, {}), (28, 65, 8, {}, {}), (30, 33, 6, LIN, {}),
    (200, 130, 1, {}, dict(score_only=True)), (130, 200, 2, LIN, dict(score_only=True)), (40, 64, 6, {}, dict(score_only=True)),
    (200, 130, 1, {}, dict(lean_trace=True)), (90, 200, 2, {}, dict(lean_trace=True)), (130, 200, 1, LIN, dict(lean_trace=True)),
], ids=lambda v: None if not isinstance(v, dict) else ("+".join(f"{k}" for k in v) or "-"))
def test_feature_equals_dense(n, m, s, ov, kw):
    """Scores, traces, completeness, layers and the table itself equal the DENSE form's: tiled sweeps s = 0..5 in
    both recurrences, beta > 0, the wide path, score-only and lean-trace storage."""
    sw = 777 if (n + m) % 2 else 400
    params = dict(synth.RNA_PARAMS, max_shift=s, structure_weight=sw, **ov)
    mols = two_molecules(1000 + n * 7 + m + s, n, m)
    traces = not kw.get("score_only")
    layers = 0 if not kw else None
    f = run_feature(mols, [(0, 1)], params, traces=traces, layers_of=layers, mu2_of=(0,), **kw)
    d, tabs = run_dense(mols, [(0, 1)], params, traces=traces, layers_of=layers, mu2_of=(0,), **kw)
    np.testing.assert_array_equal(f["mu2"][0], tabs[0])
    np.testing.assert_array_equal(d["mu2"][0], tabs[0])   # dump_mu2 of a DENSE batch: the uploaded table
    same_results(f, d, traces)
    if layers is not None:
        np.testing.assert_array_equal(f["layers"], d["layers"])
    assert f["finfo"]["table_bytes"] == 4 * n * m


@pytest.mark.parametrize("n,m,s,ov,team,lean", [
    (300, 310, 1, {}, "2", False), (150, 400, 2, {}, "2", False), (300, 320, 1, LIN, "2", False),
    (330, 650, 1, LIN, "x6", False), (200, 500, 2, LIN, "x5", False), (170, 400, 1, {}, "4", False),
    (330, 650, 1, {}, "x6", False), (100, 300, 2, {}, "4", False), (200, 400, 2, {}, "x5", False),
    (90, 400, 3, {}, "x3", False), (170, 400, 1, {}, "4", True), (330, 650, 1, {}, "x6", True)])
def test_feature_equals_dense_in_forced_team_shapes(n, m, s, ov, team, lean, monkeypatch):
    """Teams in a workgroup and across CUs, forced as tests/test_gpu_dense_mu2.py forces them."""
    monkeypatch.setenv("BIALIGN_TEAM", team)
    params = dict(synth.RNA_PARAMS, max_shift=s, **ov)
    mols = two_molecules(3000 + n + m + s, n, m)
    kw = dict(score_only=True) if lean else {}
    f = run_feature(mols, [(0, 1)], params, traces=not lean, layers_of=None if lean else 0, **kw)
    d, _ = run_dense(mols, [(0, 1)], params, traces=not lean, layers_of=None if lean else 0, **kw)
    same_results(f, d, not lean)
    if not lean:
        np.testing.assert_array_equal(f["layers"], d["layers"])
    for t in (f["timing"], d["timing"]):
        assert t["waves_per_pair"] == int(team.lstrip("x")) and t["cross_cu"] == team.startswith("x")


RAGGED = [(40, 33), (5, 90), (90, 5), (64, 64), (1, 1), (17, 18), (100, 100), (2, 50), (1, 70), (70, 1), (63, 65), (200, 63)]


def ragged_molecules(seed):
    mols, index = [], []
    for t, (n, m) in enumerate(RAGGED):
        mols += two_molecules(seed + 10 * t, n, m)
        index.append((2 * t, 2 * t + 1))
    return mols, index


@pytest.mark.parametrize("ov", [{}, dict(max_shift=2, **LIN)], ids=["affine_s1", "linear_s2"])
@pytest.mark.parametrize("dense1", [False, True], ids=["lookup_mu1", "dense_mu1"])
def test_ragged_batch_with_both_mu1_forms_and_chunking(ov, dense1):
    """A ragged batch, with LOOKUP mu1 and with a dense mu1 riding along, unbudgeted and cut into chunks."""
    params = dict(synth.RNA_PARAMS, **ov)
    mols, index = ragged_molecules(4000)
    rng = np.random.default_rng(4001)
    mu1 = [rng.integers(-300, 901, size=nm).astype(np.int32) for nm in RAGGED] if dense1 else None
    d, tabs = run_dense(mols, index, params, mu2_of=range(len(index)), mu1_dense=mu1)
    for budget in (0, 5 << 20):
        f = run_feature(mols, index, params, mu2_of=range(len(index)), mu1_dense=mu1, hbm_budget_bytes=budget)
        same_results(f, d)
        for p in range(len(index)):
            np.testing.assert_array_equal(f["mu2"][p], tabs[p])
        if budget and params["gap_opening_cost"]:
            assert f["info"]["nchunks"] > 1
            assert f["finfo"]["table_bytes"] + f["info"]["hbm_layer_bytes"] <= budget


def test_dense_mu1_with_features_single_pairs():
    """Dense mu1 next to feature mu2 in the modes dense mu1 exists in: layers equal the two-dense-tables form's."""
    rng = np.random.default_rng(4100)
    for n, m, s, ov, kw in [(130, 75, 1, {}, {}), (75, 130, 2, LIN, {}), (30, 33, 6, {}, {}),
                            (200, 130, 1, {}, dict(lean_trace=True)), (130, 200, 1, {}, dict(score_only=True))]:
        params = dict(synth.RNA_PARAMS, max_shift=s, **ov)
        mols = two_molecules(4100 + n + s, n, m)
        mu1 = [rng.integers(-300, 901, size=(n, m)).astype(np.int32)]
        traces, layers = not kw.get("score_only"), (0 if not kw else None)
        f = run_feature(mols, [(0, 1)], params, traces=traces, layers_of=layers, mu1_dense=mu1, **kw)
        d, _ = run_dense(mols, [(0, 1)], params, traces=traces, layers_of=layers, mu1_dense=mu1, **kw)
        same_results(f, d, traces)
        if layers is not None:
            np.testing.assert_array_equal(f["layers"], d["layers"])


# ---------------------------------------------------------------- rounding adversaries: dump_mu2 against the host table
def table_mismatches(mols, index, sw):
    """Entries in which the GPU's tables differ from the host's, over all pairs; and the entries compared."""
    from bialign_amd.batch import make_feature_batch
    b = make_feature_batch(mols, index, dict(synth.RNA_PARAMS, structure_weight=sw), score_only=True)
    bad = total = 0
    for p, (ia, ib) in enumerate(index):
        want = host_table(mols[ia][1], mols[ib][1], sw)
        got = b.dump_mu2(p)
        assert got.shape == want.shape
        bad += int((got != want).sum())
        total += want.size
    b.close()
    return bad, total


@pytest.mark.parametrize("sw", [400, 333, 777, 1000])
def test_rounding_on_and_beside_integers(sw):
    """Both molecules carry p = q / sw (q = 0..sw) in one feature and 0 in the others, so that sw * sqrt(p * p) sits
    on an integer or a hair beside it: a square root one ulp off changes most of the diagonal entries.  The whole
    (sw+1) x (sw+1) table of every feature is compared, diagonal included; 0 mismatches."""
    p = np.arange(sw + 1, dtype=np.float64) / sw
    zero = np.zeros(sw + 1)
    seq = rna_seq(sw, sw + 1)
    mols = [(seq, tuple(p if f == g else zero for g in range(3))) for f in range(3)]
    diag = np.diagonal(host_table(mols[0][1], mols[0][1], sw))
    q = np.arange(sw + 1)
    assert ((diag == q) | (diag == q - 1)).all()  # the family sits on the integers or a hair below (q - 1 in 82 of 2510)
    bad, total = table_mismatches(mols, [(0, 0), (1, 1), (2, 2)], sw)
    print(f"sw={sw}: {bad} mismatches in {total} entries")
    assert bad == 0


def test_rounding_on_a_million_random_feature_pairs():
    mols = [(rna_seq(71, 1000), fractional(71, 1000)), (rna_seq(72, 1000), fractional(72, 1000))]
    bad, total = table_mismatches(mols, [(0, 1)], 777)
    print(f"{bad} mismatches in {total} entries")
    assert total == 10 ** 6 and bad == 0


def test_rounding_special_values():
    """Zeros, ones, products that underflow to 0 (1e-300 * 1e-300), subnormal products (1e-160 * 1e-160), powers of
    four down to the smallest subnormal; and subnormal INPUTS against huge ones, whose products are ordinary numbers
    (a flushed input would give 0 where the reference gives thousands)."""
    vals = np.array([0.0, 1.0, 1e-300, 1e-160, 0.5, 0.25, 1.0 / 3, 2.0 / 3] + [4.0 ** -k for k in range(1, 538)])
    assert vals[-1] == 5e-324
    n = len(vals)
    mols = [(rna_seq(81, n), (vals, np.roll(vals, 1), np.roll(vals, 7))),
            (rna_seq(82, n), (np.roll(vals, 3), vals[::-1].copy(), vals))]
    bad, total = table_mismatches(mols, [(0, 1), (0, 0), (1, 1)], 1000)
    print(f"specials: {bad} mismatches in {total} entries")
    assert bad == 0
    tiny = np.array([1, 3, 12345, 2 ** 30 + 1, 2 ** 44 - 1, 2 ** 44], dtype=np.float64) * 5e-324   # subnormals up to 2^-1030
    huge = np.array([2.0 ** 1000, 2.0 ** 1010, 1.5 * 2.0 ** 1020, 2.0 ** 1021, 3.0 * 2.0 ** 1015, 1e300])
    mols = [(rna_seq(83, 6), (tiny, tiny[::-1].copy(), np.roll(tiny, 2))),
            (rna_seq(84, 6), (huge, np.roll(huge, 1), huge[::-1].copy()))]
    want = host_table(mols[0][1], mols[1][1], 1000000)
    assert want.max() > 10000  # the case is visible in the integers
    bad, total = table_mismatches(mols, [(0, 1)], 1000000)
    print(f"subnormal inputs: {bad} mismatches in {total} entries")
    assert bad == 0


# ---------------------------------------------------------------- shared molecules
def test_all_against_all_by_pair_index():
    """24 molecules, 276 pairs pointing into one upload; equals the pairs sent one by one in DENSE form, and the
    oracle on the host tables for a seeded tenth."""
    from oracle import oracle
    rng = np.random.default_rng(90)
    lens = rng.integers(20, 91, size=24)
    mols = [(rna_seq(900 + t, int(n)), fractional(950 + t, int(n))) for t, n in enumerate(lens)]
    index = [(a, b) for a in range(24) for b in range(a + 1, 24)]
    assert len(index) == 276
    params = dict(synth.RNA_PARAMS)
    f = run_feature(mols, index, params, traces=False, score_only=True)
    assert f["finfo"]["form"] == "feature" and f["finfo"]["build_launches"] == f["info"]["nchunks"] == 1
    one_by_one = []
    for pair in index:
        d, _ = run_dense(mols, [pair], params, traces=False, score_only=True)
        one_by_one.append(d["scores"][0])
    assert f["scores"] == one_by_one
    for p in rng.choice(276, size=28, replace=False):
        a, b = index[p]
        sa, sb = mols[a][0], mols[b][0]
        n, m = len(sa), len(sb)
        mu1, _ = oracle.mu_tables(sa, sb, "." * n, "." * m, params)
        mu2 = np.zeros((n + 1, m + 1), dtype=np.int32)
        mu2[1:, 1:] = host_table(mols[a][1], mols[b][1], params["structure_weight"])
        assert f["scores"][p] == oracle.solve_tables(n, m, params, mu1, mu2)["score"]


# ---------------------------------------------------------------- budget
def test_tables_are_part_of_the_chunk_plan():
    """16 pairs of 200 x 200, one-layer score-only storage: the tables alone (2.56 MB) exceed a 1 MB budget."""
    params = dict(synth.RNA_PARAMS, **LIN)
    mols, index = [], []
    for t in range(16):
        mols += two_molecules(5000 + t, 200, 200)
        index.append((2 * t, 2 * t + 1))
    budget = 1 << 20
    assert sum(4 * 200 * 200 for _ in index) > budget
    free = run_feature(mols, index, params, traces=False, score_only=True)
    tight = run_feature(mols, index, params, traces=False, score_only=True, hbm_budget_bytes=budget)
    assert free["info"]["nchunks"] == 1 and free["finfo"]["table_bytes"] == 16 * 4 * 200 * 200
    assert tight["info"]["nchunks"] > 1
    assert tight["finfo"]["table_bytes"] + tight["info"]["hbm_layer_bytes"] <= budget
    assert tight["finfo"]["build_launches"] == tight["info"]["nchunks"]
    assert tight["scores"] == free["scores"]
    d, _ = run_dense(mols, index, params, traces=False, score_only=True)
    assert free["scores"] == d["scores"]


def test_budgeted_traces_equal_unbudgeted():
    params = dict(synth.RNA_PARAMS, max_shift=1)
    mols, index = [], []
    for t in range(10):
        mols += two_molecules(5100 + t, 120 + 5 * t, 110)
        index.append((2 * t, 2 * t + 1))
    free = run_feature(mols, index, params)
    tight = run_feature(mols, index, params, hbm_budget_bytes=12 << 20)
    assert tight["info"]["nchunks"] > 1
    assert tight["finfo"]["table_bytes"] + tight["info"]["hbm_layer_bytes"] <= 12 << 20
    assert (tight["scores"], tight["traces"], tight["complete"]) == (free["scores"], free["traces"], free["complete"])


def test_a_pair_that_cannot_fit_is_nomem():
    from bialign_amd import _lib
    from bialign_amd.batch import make_feature_batch
    mols = two_molecules(5200, 600, 600)   # the table alone is 1.44 MB
    for kw in (dict(score_only=True), dict(lean_trace=True), {}):
        with pytest.raises(_lib.BialignError) as e:
            make_feature_batch(mols, [(0, 1)], dict(synth.RNA_PARAMS, **LIN), hbm_budget_bytes=1 << 20, **kw)
        assert e.value.code == _lib.E_NOMEM, e.value


# ---------------------------------------------------------------- async, errors
def test_async_run_and_wait():
    params = dict(synth.RNA_PARAMS)
    mols, index = ragged_molecules(6000)
    sync = run_feature(mols, index, params)
    for budget in (0, 5 << 20):
        got = run_feature(mols, index, params, wait=False, hbm_budget_bytes=budget)
        assert (got["scores"], got["traces"], got["complete"]) == (sync["scores"], sync["traces"], sync["complete"])
        assert got["finfo"]["build_launches"] == got["info"]["nchunks"] and got["finfo"]["build_ms"] > 0


def test_dump_layers_after_a_chunked_run():
    """dump_layers re-runs one pair: its table is rebuilt even when the buffer holds another chunk's by then."""
    from bialign_amd.batch import make_feature_batch
    params = dict(synth.RNA_PARAMS)
    mols, index = ragged_molecules(6100)
    b = make_feature_batch(mols, index, params, hbm_budget_bytes=5 << 20)
    assert b.info["nchunks"] > 1
    b.run()
    scores = [int(v) for v in b.scores()]
    layers = {p: b.dump_layers(p) for p in (0, 6, 11)}
    assert [int(v) for v in b.scores()] == scores
    b.close()
    for p, got in layers.items():
        d, _ = run_dense(mols, [index[p]], params, layers_of=0)
        np.testing.assert_array_equal(got, d["layers"])
        assert d["scores"][0] == scores[p]


def test_pack_overflow_replans_a_chunked_feature_batch(monkeypatch):
    """Packed records whose offsets overflow (as tests/test_gpu_packed_records.py makes them): the batch is cut into
    chunks again, the tables move with it and are built anew in the repeated run."""
    from bialign_amd.batch import make_feature_batch
    monkeypatch.setenv("BIALIGN_PACK", "1")
    params = dict(synth.RNA_PARAMS, sequence_match_similarity=5000, sequence_mismatch_similarity=-5000,
                  structure_weight=100, gap_opening_cost=-5000, gap_cost=-5000, shift_cost=-5000)
    mols, index = [], []
    for t in range(8):
        mols += two_molecules(6200 + t, 120 + 9 * t, 170 - 3 * t)
        index.append((2 * t, 2 * t + 1))
    probe = make_feature_batch(mols, index, params)
    one_chunk = probe.info["hbm_layer_bytes"] + probe.feature_info()["table_bytes"]
    probe.close()
    d, tabs = run_dense(mols, index, params)
    b = make_feature_batch(mols, index, params, hbm_budget_bytes=int(one_chunk * 0.4))
    assert b.info["nchunks"] >= 3
    b.run()
    t = b.timing()
    assert t["recovered_runs"] == 1 and not t["packed_records"]
    np.testing.assert_array_equal(b.dump_mu2(5), tabs[5])
    f = collect(b)
    assert f["finfo"]["build_launches"] == f["info"]["nchunks"]
    same_results(f, d)


def test_lost_co_residency_repeat_builds_again(monkeypatch):
    """A spin limit of zero makes a cross-CU team give up (tests/test_gpu_xcu_residency.py); the repeat with
    in-workgroup teams gets its tables like the first run."""
    from bialign_amd.batch import make_feature_batch
    monkeypatch.setenv("BIALIGN_TEAM", "x6")
    params = dict(synth.RNA_PARAMS)
    mols, index = [], []
    for t in range(3):
        mols += two_molecules(6300 + t, 250 + 11 * t, 560)
        index.append((2 * t, 2 * t + 1))
    d, _ = run_dense(mols, index, params, layers_of=1)
    monkeypatch.setenv("BIALIGN_XCU_SPIN_LIMIT", "0")
    b = make_feature_batch(mols, index, params)
    b.run()
    t = b.timing()
    assert t["recovered_runs"] == 1 and not t["cross_cu"]
    f = collect(b, layers_of=1)
    same_results(f, d)
    np.testing.assert_array_equal(f["layers"], d["layers"])


def raw_create(feat, n=8, m=9):
    """bialign_batch_create_features through ctypes alone (the Python layer would refuse these arguments first)."""
    from bialign_amd import _lib
    from bialign_amd.engine import default_engine, _ptr
    eng = default_engine()
    keep = dict(len_a=np.array([n], dtype=np.int32), len_b=np.array([m], dtype=np.int32),
                off=np.zeros(1, dtype=np.int64), seq=np.zeros(max(n, m), dtype=np.uint8), s=np.zeros(1, dtype=np.int32))
    prm = _lib.Params(-150, -50, -200, 1, 0, 0)
    sc = _lib.Scoring(1, _ptr(keep["s"], ctypes.c_int32), 1, _ptr(keep["s"], ctypes.c_int32))
    pr = _lib.Pairs(1, _ptr(keep["len_a"], ctypes.c_int32), _ptr(keep["len_b"], ctypes.c_int32),
                    _ptr(keep["off"], ctypes.c_int64), _ptr(keep["off"], ctypes.c_int64),
                    _ptr(keep["seq"], ctypes.c_uint8), None, _ptr(keep["seq"], ctypes.c_uint8), None, None, None, None, None)
    h = ctypes.c_void_p()
    rc = _lib.lib.bialign_batch_create_features(eng._h, ctypes.byref(prm), ctypes.byref(sc), ctypes.byref(pr),
                                                None if feat is None else ctypes.byref(feat), 0, ctypes.byref(h))
    msg = _lib.lib.bialign_last_error().decode()
    if rc == 0:
        _lib.lib.bialign_batch_destroy(h)
    return rc, msg


def test_c_abi_error_paths():
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch, make_feature_batch
    from bialign_amd.engine import _ptr
    a = [np.full(8, 0.25) for _ in range(3)]
    b = [np.full(9, 0.25) for _ in range(3)]
    mk = lambda sw, xs, ys: _lib.Features(sw, *(None if v is None else _ptr(v, ctypes.c_double) for v in xs + ys))  # noqa: E731
    assert raw_create(mk(400, a, b))[0] == 0            # cls_a / cls_b / mu2_dense NULL: fine
    assert raw_create(None)[0] == _lib.E_INVALID
    for hole in range(6):
        xs = list(a + b)
        xs[hole] = None
        assert raw_create(mk(400, xs[:3], xs[3:]))[0] == _lib.E_INVALID
    for bad in (float("nan"), float("inf"), -0.125):
        y = [v.copy() for v in b]
        y[1][4] = bad
        rc, msg = raw_create(mk(400, a, y))
        assert rc == _lib.E_INVALID and "pair 0" in msg and "position 5" in msg and "down_b" in msg, msg
    rc, msg = raw_create(mk(1 << 27, a, b))
    assert rc == _lib.E_RANGE and "safety window" in msg
    big = [np.full(8, 1e12) for _ in range(3)]
    assert raw_create(mk(400, big, b))[0] == _lib.E_RANGE   # features need not be probabilities; the bound decides
    mols = two_molecules(7000, 8, 9)
    with pytest.raises(_lib.BialignError) as e:
        make_feature_batch(mols, [(0, 1)], dict(synth.RNA_PARAMS, structure_weight=1 << 27))
    assert e.value.code == _lib.E_RANGE
    lookup = make_batch([synth.rna_pair(7, 20, 22)], dict(synth.RNA_PARAMS))
    assert lookup.feature_info() == dict(form="lookup", table_bytes=0, build_ms=0.0, build_launches=0)
    with pytest.raises(_lib.BialignError) as e:
        lookup.dump_mu2(0)
    assert e.value.code == _lib.E_INVALID
    lookup.close()
    fb = make_feature_batch(mols, [(0, 1)], dict(synth.RNA_PARAMS))
    out = np.zeros(72, dtype=np.int32)
    assert _lib.lib.bialign_batch_dump_mu2(fb._h, 1, _ptr(out, ctypes.c_int32)) == _lib.E_INVALID   # pair out of range
    np.testing.assert_array_equal(fb.dump_mu2(0), host_table(mols[0][1], mols[1][1], synth.RNA_PARAMS["structure_weight"]))
    fb.close()
