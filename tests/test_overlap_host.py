"""Overlap alignments (BIALIGN_BATCH_OVERLAP), what can be checked without a GPU:

  * the expectation the GPU tests rely on (tests/overlap_expected.py: one oracle fill per free start) against plain
    ``oracle.solve`` on explicitly cut windows, and the planted inputs' geometry;
  * the planner's decisions about the flag, as ``batch`` requests to tests/plan_check.hip: for the same request they are
    FIT's in everything but the mode -- storage, chunks, sizes, packed records, slim sweep, team -- then the refusals and
    their order, and the bits that stay unknown;
  * ``batch_cli --overlap`` with the engine stubbed, the Python layers' arguments, and the binding's new entry point."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_expected as oe
import plan_host as ph
from bialign_amd import _lib, synth
from free_ends_expected import LOW
from oracle import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE, FIT, LOCAL, OVERLAP = 1, 2, 4, 8, 64, 128
E_INVALID, E_UNSUPPORTED, E_NOMEM = -1, -2, -4
MODE_OVERLAP = 3   # AlignMode::Overlap as plan_check prints it


# ---- the helper against plain global alignments of cut windows -----------------------------------------------------

@pytest.mark.parametrize("seed,n,m,beta,s", [(11, 5, 7, -150, 1), (12, 7, 5, 0, 2), (13, 1, 6, -150, 1), (14, 6, 1, 100, 1)],
                         ids=["affine", "one-layer", "n=1", "m=1,beta>0"])
def test_expectation_equals_global_scores_of_cut_windows(seed, n, m, beta, s):
    params = dict(synth.PROTEIN_PARAMS, gap_opening_cost=beta, max_shift=s)
    sa, sb, ta, tb = pair = synth.protein_pair(seed, n, m)
    mu1, mu2 = oe.tables_of(pair, params)
    want = oe.overlap_expected(n, m, params, mu1, mu2)
    assert sorted(want["windows"]) == sorted(oe.sources(n, m)) and len(want["windows"]) == n + m + 1
    best, best_end = None, None
    for i0, j0 in oe.sources(n, m):
        for i1 in range(i0, n + 1):
            for j1 in range(j0, m + 1):
                got = oe.window_score(want, n, m, (i0, i1, j0, j1))
                if i1 < n and j1 < m:
                    assert got is None   # not an end cell
                    continue
                if i0 < i1 and j0 < j1:
                    assert got == oracle.solve(sa[i0:i1], sb[j0:j1], ta[i0:i1], tb[j0:j1], params, want_trace=False)["score"], (i0, i1, j0, j1)
                elif i0 == i1 and j0 == j1:
                    assert got == 0
                if best is None or got > best or (got == best and (i1, j1) < best_end):
                    best, best_end = got, (i1, j1)
    assert oe.window_score(want, n, m, (1, n, 1, m)) is None   # starts inside both molecules: not admissible
    assert want["score"] == best and want["end"] == best_end and best >= 0
    # the OVERLAP layers: on the end cells the windows' maxima; floored where a path may start, and the origin
    lay = want["layers"]
    ei, ej = oe.end_cells(n, m)
    for i1, j1 in zip(ei, ej):
        assert lay[:, i1, j1, s, s].max() == want["ends"][i1, j1]
    assert (lay[-1, :, 0, s, s] >= 0).all() and (lay[-1, 0, :, s, s] >= 0).all() and lay[-1, 0, 0, s, s] == 0
    # ... and without a free start that is admissible, the plain layers: the run of the source (0, 0) is one of the maxima
    plain = oracle.solve_tables(n, m, params, mu1, mu2, want_trace=False)["layers"]
    ok = oe.run_mask(n, m, s)[None] & (plain > LOW)
    assert (lay[ok] >= plain[ok]).all()


@pytest.mark.parametrize("kind,n,m", [("a_suffix_b_prefix", 12, 14), ("b_suffix_a_prefix", 14, 12), ("a_in_b", 8, 15), ("b_in_a", 15, 8)])
def test_planted_pairs_have_their_geometry(kind, n, m):
    params = dict(synth.PROTEIN_PARAMS, max_shift=1)
    pair = oe.make_pair("protein", 3, n, m, kind)
    assert (len(pair[0]), len(pair[1])) == (n, m)
    want = oe.overlap_expected(n, m, params, *oe.tables_of(pair, params), want_layers=False)
    assert want["score"] > 0 and want["starts"] and oe.geometry(kind, want, n, m), (want["end"], want["starts"])


# ---- the planner ---------------------------------------------------------------------------------------------------

SHARED = {   # name -> a request both modes answer alike but for the mode: ph.case without its flags
    "full-affine": dict(),
    "full-linear": dict(s=2, beta=0),
    "full-s0": dict(s=0),
    "full-s5": dict(s=5),
    "full-beta-positive": dict(beta=100),
    "full-dense": dict(dense=1),
    "score-only": dict(storage=SCORE_ONLY),
    "score-only-linear": dict(storage=SCORE_ONLY, beta=0),
    "tight": dict(budget=ph.TIGHT),
    "tight-score-only": dict(storage=SCORE_ONLY, budget=ph.TIGHT),
    "lean-trace": dict(storage=LEAN_TRACE),
    "level-trace": dict(storage=LEVEL_TRACE),
    "level-trace-wide": dict(storage=LEVEL_TRACE, s=7),
    "wide": dict(s=6),
    "wide-score-only": dict(storage=SCORE_ONLY, s=6),
    "null": dict(null=1),
    "null-dense": dict(null=1, dense=1),
    "forced-pack-x4": dict(team="x4", pack="1"),
    "forced-3": dict(team="3", pack="1"),
    "forced-3-no-pack": dict(team="3", pack="0"),
    "forced-h2": dict(s=2, team="h2", pack="1"),
    "score-only-forced-3": dict(storage=SCORE_ONLY, team="3"),
    "score-only-forced-x3": dict(storage=SCORE_ONLY, team="x3"),
}
OWN = {
    "plain-full": ph.case(0),
    "overlap-fit": ph.case(OVERLAP | FIT),
    "overlap-local": ph.case(OVERLAP | LOCAL),
    "overlap-fit-local": ph.case(OVERLAP | FIT | LOCAL),
    "overlap-fit-lean-trace": ph.case(OVERLAP | FIT | LEAN_TRACE),
    "overlap-local-wide": ph.case(OVERLAP | LOCAL, s=6),
    "unknown-bit-0x100": ph.case(OVERLAP | 0x100),
    "unknown-bit-16": ph.case(OVERLAP | 16),
    "unknown-bit-32": ph.case(OVERLAP | 32),
    "null-unknown-bit": ph.case(OVERLAP | 32, null=1),
}


def _case(mode, c):
    c = dict(c)
    return ph.case(mode | c.pop("storage", 0), **c)


def _requests(cases):
    lines = []
    for c in cases.values():
        words = dict(ph.SMALL, flags=c["flags"], s=c["s"], beta=c["beta"], budget=c["budget"])
        if c.get("dense"):
            words.update(form="mu12", mu1=100, mu2=100)
        if c.get("null"):
            words.update(replicas=4, seed=7)
        lines += [f"env BIALIGN_TEAM={c.get('team', '')}", f"env BIALIGN_PACK={c.get('pack', '')}", ph.request(pairs=[(300, 400, 2)], **words)]
    return lines


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ph.build(tmp_path_factory.mktemp("overlapplan"))


@pytest.fixture(scope="module")
def both(exe):
    """name -> (FIT's Plan, OVERLAP's Plan) of the shared requests."""
    fit = ph.plans(exe, _requests({k: _case(FIT, c) for k, c in SHARED.items()}))
    ovl = ph.plans(exe, _requests({k: _case(OVERLAP, c) for k, c in SHARED.items()}))
    return dict(zip(SHARED, zip(fit, ovl)))


@pytest.fixture(scope="module")
def own(exe):
    return ph.mode_answers(exe, OWN)


@pytest.mark.parametrize("name", list(SHARED))
def test_planner_answers_overlap_as_fit_but_for_the_mode(both, name):
    fit, ovl = both[name]
    assert ovl.rc == fit.rc and ovl.msg == fit.msg.replace("FIT", "OVERLAP"), (fit.msg, ovl.msg)
    assert fit.mode == 1 and ovl.mode == MODE_OVERLAP and ovl.flags == fit.flags - FIT + OVERLAP
    strip = lambda p: {k: v for k, v in p.fields.items() if k not in ("mode", "flags")}
    assert strip(ovl) == strip(fit)
    assert (ovl.chunks, ovl.order, ovl.sizes, ovl.pairs, ovl.teams) == (fit.chunks, fit.order, fit.sizes, fit.pairs, fit.teams)


def test_planner_accepts_overlap_on_the_fast_kernels(both):
    for name in ("full-affine", "full-linear", "full-s0", "full-s5", "full-beta-positive", "full-dense", "score-only",
                 "score-only-linear", "tight-score-only", "null", "null-dense"):
        assert both[name][1].rc == 0 and both[name][1].msg == "", name
    assert both["forced-pack-x4"][1].fields["pack"] == 1 and both["forced-pack-x4"][1].teams[0]["gw"] == 4   # packed records, a cross-CU team
    assert both["forced-3"][1].teams[0]["slim"] == 1 and both["forced-3"][1].teams[0]["tw"] == 3           # the slim sweep
    assert both["score-only-forced-3"][1].teams[0]["slim"] == 1                                           # ... and its LEAN form
    assert both["score-only-forced-x3"][1].teams[0]["gw"] == 3
    assert both["null"][1].flags == SCORE_ONLY | OVERLAP


def test_planner_refusals_and_their_order(both, own):
    for name in ("lean-trace", "level-trace", "level-trace-wide", "wide", "wide-score-only"):
        got = both[name][1]
        assert got.rc == E_UNSUPPORTED and "OVERLAP" in got.msg, (name, got.msg)
    got = both["tight"][1]   # no silent fallback to LEAN_TRACE
    assert got.rc == E_NOMEM and "OVERLAP" in got.msg and "LEAN_TRACE" in got.msg, got.msg
    assert own["plain-full"]["rc"] == 0 and own["plain-full"]["mode"] == 0
    for name, other in (("overlap-fit", "FIT"), ("overlap-local", "LOCAL")):
        assert own[name]["rc"] == E_INVALID and "OVERLAP" in own[name]["msg"] and other in own[name]["msg"], own[name]
    assert own["overlap-fit-local"]["rc"] == E_INVALID and "exclude" in own["overlap-fit-local"]["msg"]
    # the free-ends refusals come first, as between FIT and LOCAL
    assert own["overlap-fit-lean-trace"]["rc"] == E_UNSUPPORTED and "LEAN_TRACE" in own["overlap-fit-lean-trace"]["msg"]
    assert own["overlap-local-wide"]["rc"] == E_UNSUPPORTED and "max_shift" in own["overlap-local-wide"]["msg"]


@pytest.mark.parametrize("name", ["unknown-bit-0x100", "unknown-bit-16", "unknown-bit-32", "null-unknown-bit"])
def test_unknown_flag_bits_stay_invalid(own, name):
    assert own[name]["rc"] == E_INVALID and "unknown bits" in own[name]["msg"], own[name]


def test_long_pairs_are_refused_for_the_key(exe):
    """n + m < 60000: the end's position in the pair's key is 32 bits wide (score-only and full storage alike)."""
    words = dict(ph.SMALL, s=1, beta=-10, budget=ph.ROOMY)
    words.update(amax=50, bmax=50, gamma=-10, delta=-10)   # (small scores: pairs this long stay inside the int32 window)
    fit, ovl, ok = ph.plans(exe, [ph.request(pairs=[(100, 59900, 1)], flags=FIT | SCORE_ONLY, **words),
                                  ph.request(pairs=[(100, 59900, 1)], flags=OVERLAP | SCORE_ONLY, **words),
                                  ph.request(pairs=[(100, 59899, 1)], flags=OVERLAP | SCORE_ONLY, **words)])
    assert fit.rc == 0 and ok.rc == 0
    assert ovl.rc == E_UNSUPPORTED and "OVERLAP" in ovl.msg and "60000" in ovl.msg, ovl.msg


# ---- the binding and the Python layers -----------------------------------------------------------------------------

def test_binding_declares_overlap():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert "bialign_batch_get_overlap_spans" in names and _lib.BATCH_OVERLAP == OVERLAP
    with open(os.path.join(REPO, "include", "bialign.h")) as fh:
        header = fh.read()
    assert re.search(r"^#define\s+BIALIGN_BATCH_OVERLAP\s+128u\s*$", header, re.M)
    assert re.search(r"^int bialign_batch_get_overlap_spans\(const bialign_batch\* b, int32_t\* start_a, int32_t\* end_a, "
                     r"int32_t\* start_b, int32_t\* end_b\);", header, re.M)
    assert hasattr(_lib.lib, "bialign_batch_get_overlap_spans")
    assert _lib.lib.bialign_abi_version() == 10


def test_python_layers_take_overlap():
    import inspect
    from bialign_amd import batch, distributed, engine, significance
    for fn in (significance.null_batch, significance.null_feature_batch, significance.null_dense_batch, significance.zscores,
               significance.zscores_features, significance.zscores_dense, batch.make_batch, batch.make_feature_batch,
               engine.Batch.__init__, distributed.align_sharded):
        assert inspect.signature(fn).parameters["overlap"].default is False, fn
    assert callable(engine.Batch.overlap_spans)
    pairs = [synth.protein_pair(1, 5, 6)]
    for fn in (significance.null_batch, significance.zscores):   # refused ahead of any device work
        for other in ("fit", "local"):
            with pytest.raises(ValueError, match="exclude"):
                fn(pairs, dict(synth.PROTEIN_PARAMS), replicas=2, overlap=True, **{other: True})
    mols = [("ACGU", tuple(np.full(4, 1 / 3) for _ in range(3)))] * 2
    with pytest.raises(ValueError, match="exclude"):
        significance.zscores_features(mols, [(0, 1)], dict(synth.RNA_PARAMS), replicas=2, overlap=True, local=True)
    with pytest.raises(ValueError, match="exclude"):
        significance.null_dense_batch(pairs, dict(synth.PROTEIN_PARAMS), 2, mu1_dense=[np.zeros((5, 6), dtype=np.int32)], overlap=True, fit=True)


def test_significance_passes_the_mode_through(monkeypatch):
    """zscores(overlap=True): the observed scores and the null batch are made in the mode."""
    from bialign_amd import batch, significance
    seen = []

    class Stub:
        npairs = 1

        def __init__(self, kw):
            seen.append(kw)

        def run(self):
            pass

        def scores(self):
            return np.array([500], dtype=np.int32)

        def null_stats(self, observed):
            return dict(sum=np.array([400]), sumsq=np.array([100000]), min=np.array([100]), max=np.array([300]),
                        n_ge=np.array([0]), replicas=np.array([2]))

        def close(self):
            pass
    monkeypatch.setattr(batch, "make_batch", lambda pairs, params, **kw: Stub(dict(kw, what="observed")))
    monkeypatch.setattr(significance, "null_batch", lambda pairs, params, replicas, **kw: Stub(dict(kw, what="null")))
    z = significance.zscores([synth.protein_pair(1, 5, 6)], dict(synth.PROTEIN_PARAMS), replicas=2, overlap=True)
    assert len(seen) == 2 and all(kw["overlap"] is True and kw["fit"] is False and kw["local"] is False for kw in seen), seen
    assert {kw["what"] for kw in seen} == {"observed", "null"} and len(z["z"]) == 1


# ---- batch_cli --overlap, the engine stubbed -----------------------------------------------------------------------

class FakeBatch:
    """What batch_cli asks of engine.Batch: pair t's walk is the ungapped alignment of A[sa:ea] with B[sb:eb]."""
    affine = True

    def __init__(self, pairs, spans):
        self.pairs, self.spans = pairs, spans

    def run(self):
        pass

    def scores(self):
        return np.array([1000 + t for t in range(len(self.pairs))], dtype=np.int32)

    def overlap_spans(self):
        return tuple(np.array([sp[x] for sp in self.spans], dtype=np.int32) for x in range(4))

    def traces(self):
        return [np.full(ea - sa, 15, dtype=np.uint8) for sa, ea, _, _ in self.spans], np.ones(len(self.spans), dtype=bool)

    def close(self):
        pass


SPANS = [(0, 3, 4, 7), (2, 5, 0, 3)]   # A inside B's tail; A's suffix on B's prefix
ROWS = [("a0", "CDE", "HHE", "b0", "AAAACDE", "CCCCHHE"), ("a1", "KACDE", "CHHEE", "b1", "CDEWKK", "HEECCC")]
OPTS = ["--type", "Protein", "--simmatrix", "BLOSUM62", "--gap_opening_cost", "-150", "--gap_cost", "-50",
        "--shift_cost", "-150", "--structure_weight", "800", "--max_shift", "1", "--outmode", "sorted"]


@pytest.fixture
def stub_engine(monkeypatch):
    from bialign_amd import batch, distributed, engine, significance
    calls = dict(make_batch=[], zscores=[])

    def make_batch(pairs, params, **kw):
        calls["make_batch"].append(kw)
        return FakeBatch(pairs, SPANS[:len(pairs)])

    def zscores(pairs, params, **kw):
        calls["zscores"].append(kw)
        n = len(pairs)
        return dict(z=np.full(n, 2.5), mean=np.full(n, 10.0), std=np.full(n, 4.0), n_ge=np.zeros(n, dtype=np.int64),
                    replicas=np.full(n, kw["replicas"], dtype=np.int64))
    monkeypatch.setattr(batch, "make_batch", make_batch)
    monkeypatch.setattr(significance, "zscores", zscores)
    monkeypatch.setattr(engine, "default_engine", lambda device=0: None)
    monkeypatch.setattr(distributed, "init_from_env", lambda backend=None: (0, 0, 1))
    return calls


def write_rows(tmp_path):
    f = tmp_path / "pairs.tsv"
    f.write_text("".join("\t".join(r) + "\n" for r in ROWS))
    return str(f)


def test_batch_cli_overlap_blocks(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    assert batch_cli.build_parser().parse_args(["x.tsv"]).overlap is False
    assert batch_cli.local_span_lines(2, 5, 0, 3) == ["A span\t 3..5", "B span\t 1..3"]   # the span formatting the mode shares
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--overlap"])
    out = capsys.readouterr().out
    kw = stub_engine["make_batch"][0]
    assert kw["overlap"] is True and kw["fit"] is False and kw["local"] is False and kw["score_only"] is False
    blocks = out.split(">pair ")[1:]
    assert len(blocks) == 2
    for t, (blk, (sa, ea, sb, eb)) in enumerate(zip(blocks, SPANS)):
        lines = blk.split("\n")
        at = lines.index(f"SCORE: {1000 + t}")
        assert lines[at + 1] == f"A span\t {sa + 1}..{ea}" and lines[at + 2] == f"B span\t {sb + 1}..{eb}" and lines[at + 3] == ""
        assert "seqA\t " + ROWS[t][1] in lines and "seqB\t " + ROWS[t][4] in lines   # the input echo shows the whole molecules
        rows_a = [ln for ln in lines[at + 4:] if ln.startswith(ROWS[t][0] + " ") and "shifts" not in ln]
        rows_b = [ln for ln in lines[at + 4:] if ln.startswith(ROWS[t][3] + " ") and "shifts" not in ln]
        assert rows_a and all(ln.split()[-1] in (ROWS[t][1][sa:ea], ROWS[t][2][sa:ea]) for ln in rows_a), rows_a
        assert rows_b and all(ln.split()[-1] in (ROWS[t][4][sb:eb], ROWS[t][5][sb:eb]) for ln in rows_b), rows_b


def test_batch_cli_overlap_score_only_and_zscore(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--overlap", "--score_only", "--zscore", "8"])
    out = capsys.readouterr().out.split("\n")
    assert stub_engine["make_batch"][0]["overlap"] is True and stub_engine["make_batch"][0]["score_only"] is True
    z = stub_engine["zscores"][0]
    assert z["overlap"] is True and z["fit"] is False and z["local"] is False and z["replicas"] == 8
    assert out[0] == "pair 0\ta0\tb0\t1000\t3\t7" and out[2] == "pair 1\ta1\tb1\t1001\t5\t3"   # the 1-based ends of A and B
    assert out[1].startswith("ZSCORE: 2.50 ") and out[3].startswith("ZSCORE: 2.50 ")


@pytest.mark.parametrize("other", ["--fit", "--local"])
def test_batch_cli_refuses_overlap_with_another_mode(tmp_path, capsys, stub_engine, other):
    from bialign_amd import batch_cli
    with pytest.raises(SystemExit) as err:
        batch_cli.main([write_rows(tmp_path)] + OPTS + ["--overlap", other])
    assert err.value.code == 2 and "exclude" in capsys.readouterr().err and not stub_engine["make_batch"]
