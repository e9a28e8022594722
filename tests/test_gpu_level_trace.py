"""Level-checkpointed traceback of the wide-band path (BIALIGN_BATCH_LEVEL_TRACE, bialign_wide.hpp): scores, traces
and completeness flags from checkpoints of five anti-diagonal levels and one segment of re-swept levels at a time.
Everything is compared exactly (integers, ==) with the CPU oracle and with the full-storage wide path of the same
build; the shapes are the smallest at which segments, parts and chunks still come in numbers greater than one."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from bialign_amd import synth

pytestmark = pytest.mark.gpu

WIDE = load_golden("wide_band.json")
LIN = dict(gap_opening_cost=0, gap_cost=-200, shift_cost=-250)
SHAPES = [(23, 31), (40, 17)]
RAGGED = [(5, 45), (45, 5), (12, 30), (33, 34), (20, 9), (41, 38)]


def run(pairs, params, **kw):
    """-> dict(scores, traces, complete, info, timing) of one run of a batch."""
    from bialign_amd.batch import make_batch
    return collect(make_batch(pairs, params, **kw))


def collect(b):
    from bialign_amd.engine import trace_codes_to_columns
    b.run()
    tr, ok = b.traces()
    out = dict(scores=[int(v) for v in b.scores()], traces=[trace_codes_to_columns(t) for t in tr],
               complete=[bool(v) for v in ok], info=b.current_info(), timing=b.timing())
    b.close()
    return out


def frozen(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def oracle_ref(pair, params):
    """(score, trace, complete) of the oracle, computed once per (pair, parameters)."""
    from oracle import oracle
    ref = oracle.solve(*pair, dict(params))
    return ref["score"], oracle.trace_to_lists(ref["trace"]), bool(ref["complete"])


def assert_oracle(got, pairs, params):
    for t, pair in enumerate(pairs):
        score, trace, complete = oracle_ref(tuple(pair), frozen(params))
        assert got["scores"][t] == score, t
        assert got["traces"][t] == trace, t
        assert got["complete"][t] == complete, t


def assert_same(got, full):
    from bialign_amd import _lib
    assert got["info"]["storage"] == _lib.BATCH_LEVEL_TRACE and full["info"]["storage"] == 0
    assert got["scores"] == full["scores"] and got["traces"] == full["traces"] and got["complete"] == full["complete"]


@functools.lru_cache(maxsize=None)
def full_ref(pairs, params):
    return run(list(pairs), dict(params))


@pytest.mark.parametrize("parts", ["1", "3"])
@pytest.mark.parametrize("seg", ["8", "13", "64"])
@pytest.mark.parametrize("rec", ["affine", "linear"])
@pytest.mark.parametrize("s", [6, 7, 10])
def test_segments_and_parts(s, rec, seg, parts, monkeypatch):
    """Many segments, segments that do not divide the levels, a single segment; one and several workgroups per pair."""
    monkeypatch.setenv("BIALIGN_WIDE_SEG", seg)
    monkeypatch.setenv("BIALIGN_WIDE_PARTS", parts)
    pairs = tuple(synth.protein_pair(5000 + n, n, m) for n, m in SHAPES)
    params = dict(synth.PROTEIN_PARAMS, max_shift=s, **(LIN if rec == "linear" else {}))
    got = run(list(pairs), params, level_trace=True)
    assert got["timing"]["cross_cu"] == (parts != "1")
    assert_oracle(got, pairs, params)
    assert_same(got, full_ref(pairs, frozen(params)))


@pytest.mark.parametrize("name,shape,s,ov", [("band_wider_than_molecules", (9, 11), 12, {}),
                                              ("band_wider_linear", (9, 11), 12, LIN),
                                              ("length_one_a", (1, 14), 6, {}), ("length_one_b", (14, 1), 6, LIN),
                                              ("one_by_one", (1, 1), 6, {}),
                                              ("beta_positive", (21, 19), 6, dict(gap_opening_cost=60)),
                                              ("beta_positive_s7", (16, 24), 7, dict(gap_opening_cost=80))])
@pytest.mark.parametrize("seg", ["8", None])
def test_edge_shapes(name, shape, s, ov, seg, monkeypatch):
    if seg:
        monkeypatch.setenv("BIALIGN_WIDE_SEG", seg)
    pairs = (synth.protein_pair(5100 + shape[0] + s, *shape),)
    params = dict(synth.PROTEIN_PARAMS, max_shift=s, **ov)
    got = run(list(pairs), params, level_trace=True)
    assert_oracle(got, pairs, params)
    assert_same(got, full_ref(pairs, frozen(params)))


@pytest.mark.parametrize("rec", WIDE, ids=[r["name"] for r in WIDE])
def test_golden_wide_band_through_level_trace(rec, monkeypatch):
    """The compiled reference's vectors: score, trace and the incomplete-traceback flag equal the fixture."""
    monkeypatch.setenv("BIALIGN_WIDE_SEG", "8")
    got = run([(rec["seqA"], rec["seqB"], rec["strA"], rec["strB"])], rec["params"], level_trace=True)
    assert got["scores"][0] == rec["score"]
    assert got["traces"][0] == rec["trace"]
    assert got["complete"][0] == rec["complete"]
    assert got["info"]["storage"] == 4


def ragged_pairs():
    return tuple(synth.protein_pair(5200 + t, n, m) for t, (n, m) in enumerate(RAGGED))


@pytest.mark.parametrize("rec", ["affine", "linear"])
def test_ragged_batch_and_chunks(rec, monkeypatch):
    """Six pairs of lengths 5..45 at different segments in one launch; the same under a budget that forces chunks."""
    monkeypatch.setenv("BIALIGN_WIDE_SEG", "16")
    pairs = ragged_pairs()
    params = dict(synth.PROTEIN_PARAMS, max_shift=6, **(LIN if rec == "linear" else {}))
    one = run(list(pairs), params, level_trace=True)
    assert one["info"]["nchunks"] == 1
    assert_oracle(one, pairs, params)
    assert_same(one, full_ref(pairs, frozen(params)))
    # half of what the six regions take together: more than the largest pair's (about a third), so at least two chunks
    budget = one["info"]["hbm_layer_bytes"] // 2
    many = run(list(pairs), params, level_trace=True, hbm_budget_bytes=budget)
    assert many["info"]["nchunks"] > 1
    assert many["info"]["hbm_layer_bytes"] <= budget
    assert many["info"]["storage"] == 4
    assert many["scores"] == one["scores"] and many["traces"] == one["traces"] and many["complete"] == one["complete"]


def test_dense_mu2_and_dense_mu1(monkeypatch):
    from oracle import oracle
    monkeypatch.setenv("BIALIGN_WIDE_SEG", "11")
    rng = np.random.default_rng(52)
    shapes = [(23, 31), (40, 17), (7, 9)]
    pairs = [synth.protein_pair(5300 + t, n, m) for t, (n, m) in enumerate(shapes)]
    tab2 = [rng.integers(-500, 1500, size=s).astype(np.int32) for s in shapes]
    tab1 = [rng.integers(-400, 1100, size=s).astype(np.int32) for s in shapes]
    for ov in ({}, LIN):
        params = dict(synth.PROTEIN_PARAMS, max_shift=6, **ov)
        for kw in (dict(mu2_dense=tab2), dict(mu1_dense=tab1), dict(mu2_dense=tab2, mu1_dense=tab1)):
            got = run(pairs, params, level_trace=True, **kw)
            assert_same(got, run(pairs, params, **kw))
            for t, (pair, (n, m)) in enumerate(zip(pairs, shapes)):
                mu1, mu2 = oracle.mu_tables(*pair, params)
                if "mu2_dense" in kw:
                    mu2 = np.zeros((n + 1, m + 1), dtype=np.int32)
                    mu2[1:, 1:] = tab2[t]
                if "mu1_dense" in kw:
                    mu1 = np.zeros((n + 1, m + 1), dtype=np.int32)
                    mu1[1:, 1:] = tab1[t]
                ref = oracle.solve_tables(n, m, params, mu1, mu2)
                assert got["scores"][t] == ref["score"]
                assert got["traces"][t] == oracle.trace_to_lists(ref["trace"])
                assert got["complete"][t] == bool(ref["complete"])


def test_feature_form_mu2(monkeypatch):
    """FEATURE-form mu2 (the GPU builds each chunk's tables): equal to the full-storage run and, through the tables
    the batch dumps, to the oracle."""
    from oracle import oracle
    from bialign_amd.batch import make_feature_batch
    from test_gpu_mu2_features import fractional, rna_seq
    monkeypatch.setenv("BIALIGN_WIDE_SEG", "9")
    lens = [22, 31, 12]
    mols = [(rna_seq(5400 + t, n), fractional(5410 + t, n)) for t, n in enumerate(lens)]
    index = [(0, 1), (1, 2), (2, 0)]
    params = dict(synth.RNA_PARAMS, max_shift=6)
    full = collect(make_feature_batch(mols, index, params))
    b = make_feature_batch(mols, index, params, level_trace=True)
    tabs = [b.dump_mu2(p) for p in range(len(index))]
    got = collect(b)
    assert_same(got, full)
    for p, (ia, ib) in enumerate(index):
        n, m = lens[ia], lens[ib]
        mu1, _ = oracle.mu_tables(mols[ia][0], mols[ib][0], "." * n, "." * m, params)
        mu2 = np.zeros((n + 1, m + 1), dtype=np.int32)
        mu2[1:, 1:] = tabs[p]
        ref = oracle.solve_tables(n, m, params, mu1, mu2)
        assert got["scores"][p] == ref["score"]
        assert got["traces"][p] == oracle.trace_to_lists(ref["trace"])
        assert got["complete"][p] == bool(ref["complete"])


def test_memory_and_automatic_choice():
    """One 300 x 300 pair at max_shift 6, affine: 735 MB of layers in the default mode.  Asked for, the mode takes at
    most 0.4 of that (0.27 by the formula at the best C with 12-dword cells; the rest is whole-segment rounding, the
    ring and the sixth level of segment 0); not asked for, the engine takes it when the budget is 400 MiB."""
    from bialign_amd import _lib
    pairs = [synth.protein_pair(5500, 300, 300)]
    params = dict(synth.PROTEIN_PARAMS, max_shift=6)
    full = run(pairs, params)
    assert full["info"]["storage"] == 0
    asked = run(pairs, params, level_trace=True)
    print(f"full {full['info']['hbm_layer_bytes']} B fill {full['timing']['fill_ms']:.1f} tb {full['timing']['traceback_ms']:.1f} ms | "
          f"level {asked['info']['hbm_layer_bytes']} B fill {asked['timing']['fill_ms']:.1f} tb {asked['timing']['traceback_ms']:.1f} ms")
    assert asked["info"]["hbm_layer_bytes"] <= 0.4 * full["info"]["hbm_layer_bytes"]
    assert_same(asked, full)
    auto = run(pairs, params, hbm_budget_bytes=400 << 20)
    assert auto["info"]["storage"] == _lib.BATCH_LEVEL_TRACE == 4
    assert auto["info"]["hbm_layer_bytes"] <= 400 << 20
    assert_same(auto, full)


def test_refusals_and_errors():
    from bialign_amd import _lib
    from bialign_amd.batch import make_batch
    pair = synth.protein_pair(5600, 20, 22)
    with pytest.raises(_lib.BialignError) as e:   # the tiled bands have the memory-lean traceback
        make_batch([pair], dict(synth.PROTEIN_PARAMS, max_shift=2), level_trace=True)
    assert e.value.code == _lib.E_UNSUPPORTED and "LEAN_TRACE" in e.value.message
    b = make_batch([pair], dict(synth.PROTEIN_PARAMS, max_shift=6), level_trace=True)
    b.run()
    with pytest.raises(_lib.BialignError) as e:   # no full layers to dump
        b.dump_layers(0)
    assert e.value.code == _lib.E_INVALID
    b.close()
    with pytest.raises(_lib.BialignError) as e:   # 60 x 60 at max_shift 8: not even this mode fits 1 MiB
        make_batch([synth.protein_pair(5601, 60, 60)], dict(synth.PROTEIN_PARAMS, max_shift=8), hbm_budget_bytes=1 << 20)
    assert e.value.code == _lib.E_NOMEM


def test_raw_flag_combinations_are_invalid():
    """Through the C ABI itself (the Python front end refuses earlier): LEVEL_TRACE with SCORE_ONLY or LEAN_TRACE."""
    import ctypes
    from bialign_amd import _lib
    from bialign_amd.engine import default_engine, _ptr
    eng = default_engine()
    one = np.ones(1, dtype=np.int32)
    zero64 = np.zeros(1, dtype=np.int64)
    code = np.zeros(1, dtype=np.uint8)
    tab = np.zeros(1, dtype=np.int32)
    sc = _lib.Scoring(1, _ptr(tab, ctypes.c_int32), 1, _ptr(tab, ctypes.c_int32))
    pr = _lib.Pairs(1, _ptr(one, ctypes.c_int32), _ptr(one, ctypes.c_int32), _ptr(zero64, ctypes.c_int64),
                    _ptr(zero64, ctypes.c_int64), _ptr(code, ctypes.c_uint8), _ptr(code, ctypes.c_uint8),
                    _ptr(code, ctypes.c_uint8), _ptr(code, ctypes.c_uint8), None, None, None, None)
    for other in (_lib.BATCH_SCORE_ONLY, _lib.BATCH_LEAN_TRACE):
        prm = _lib.Params(-150, -50, -150, 6, 0, _lib.BATCH_LEVEL_TRACE | other)
        h = ctypes.c_void_p()
        rc = _lib.lib.bialign_batch_create(eng._h, ctypes.byref(prm), ctypes.byref(sc), ctypes.byref(pr), 0, ctypes.byref(h))
        assert rc == _lib.E_INVALID and not h.value


def test_lost_co_residency_is_recovered(monkeypatch):
    """Spin limit zero (the engine's recovery switch): every level barrier of a multi-part sweep gives up at once and
    the host repeats the run with one workgroup per pair."""
    monkeypatch.setenv("BIALIGN_XCU_SPIN_LIMIT", "0")
    monkeypatch.setenv("BIALIGN_WIDE_SEG", "24")
    pairs = tuple(synth.protein_pair(5700 + t, 50 + t, 60) for t in range(3))
    for ov in (LIN, {}):
        params = dict(synth.PROTEIN_PARAMS, max_shift=6, **ov)
        got = run(list(pairs), params, level_trace=True)
        assert got["timing"]["recovered_runs"] == 1 and not got["timing"]["cross_cu"]
        assert got["info"]["storage"] == 4
        assert_oracle(got, pairs, params)
