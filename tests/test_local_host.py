"""Local alignments (BIALIGN_BATCH_LOCAL), what can be checked without a GPU:

  * the expectation the GPU tests rely on (tests/local_expected.py: one oracle fill per start (i0, j0)) against plain
    ``oracle.solve`` on explicitly cut windows;
  * the planner's decisions about the flag -- where it is accepted, every refusal, no silent fallback to LEAN_TRACE, null
    batches pass it through, bits 16 and 32 stay unknown, no pack, no slim sweep and no cross-CU team -- as ``batch``
    requests to tests/plan_check.hip, the stand-alone host program around bialign_plan.hpp;
  * ``batch_cli --local``: argument handling, the span lines and the windows, with the engine stubbed;
  * the binding declares the new entry point."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_expected as le
import plan_host as ph
from bialign_amd import _lib, synth
from oracle import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE, FIT, LOCAL = 1, 2, 4, 8, 64
E_INVALID, E_UNSUPPORTED, E_NOMEM = -1, -2, -4


# ---- the helper against plain global alignments of cut windows -----------------------------------------------------

@pytest.mark.parametrize("seed,n,m,beta,s", [(11, 5, 7, -150, 1), (12, 6, 7, 0, 2)], ids=["affine", "one-layer"])
def test_expectation_equals_global_scores_of_cut_windows(seed, n, m, beta, s):
    params = dict(synth.PROTEIN_PARAMS, gap_opening_cost=beta, max_shift=s)
    sa, sb, ta, tb = pair = synth.protein_pair(seed, n, m)
    mu1, mu2 = le.tables_of(pair, params)
    want = le.local_expected(n, m, params, mu1, mu2)
    win = want["windows"]
    best, best_end = 0, (0, 0)   # the window that is empty in both molecules
    for i0 in range(n + 1):
        for j0 in range(m + 1):
            assert win[i0, j0, i0, j0] == 0
            assert (win[i0, j0, :i0] == le.NONE32).all() and (win[i0, j0, :, :j0] == le.NONE32).all()
    for i0 in range(n):
        for i1 in range(i0 + 1, n + 1):
            for j0 in range(m):
                for j1 in range(j0 + 1, m + 1):
                    cut = oracle.solve(sa[i0:i1], sb[j0:j1], ta[i0:i1], tb[j0:j1], params, want_trace=False)["score"]
                    assert win[i0, j0, i1, j1] == cut, (i0, i1, j0, j1)
                    assert le.window_global(params, mu1, mu2, i0, i1, j0, j1) == cut
                    if cut > best or (cut == best and (i1, j1) < best_end):
                        best, best_end = cut, (i1, j1)
    # a window that is empty in one molecule is all gaps: the same for every start of the other, never above 0
    for j0 in range(m):
        for j1 in range(j0 + 1, m + 1):
            assert len({int(win[i0, j0, i0, j1]) for i0 in range(n + 1)}) == 1 and win[0, j0, 0, j1] < 0
    assert want["score"] == best and want["end"] == best_end
    assert (want["ends"] == win.max(axis=(0, 1))).all()
    assert (want["edge"] == np.maximum(win[0].max(axis=0), win[:, 0].max(axis=0))).all()
    # the LOCAL layers on the diagonal points are the windows' maxima by end, and never below the floor
    lay = want["layers"]
    for i1 in range(n + 1):
        for j1 in range(m + 1):
            assert lay[:, i1, j1, s, s].max() == want["ends"][i1, j1]
            assert lay[-1, i1, j1, s, s] >= 0
    assert lay[-1, 0, 0, s, s] == 0


def test_planted_pair_has_an_inner_window():
    params = dict(synth.PROTEIN_PARAMS, max_shift=1)
    pair = le.make_pair("protein", 3, 12, 14, True)
    want = le.local_expected(12, 14, params, *le.tables_of(pair, params), want_layers=False)
    assert want["inner"] and want["score"] > 0
    starts = np.argwhere(want["windows"][:, :, want["end"][0], want["end"][1]] == want["score"])
    assert len(starts) and (starts > 0).all()


# ---- the planner ---------------------------------------------------------------------------------------------------

CASES = {   # two pairs of 300 x 400: full layers at max_shift 1 ~42 MB a pair, the LEAN form ~2 MB
    "plain-full": ph.case(0),
    "local-full-affine": ph.case(LOCAL),
    "local-full-linear": ph.case(LOCAL, s=2, beta=0),
    "local-full-s0": ph.case(LOCAL, s=0),
    "local-full-s5": ph.case(LOCAL, s=5),
    "local-full-dense": ph.case(LOCAL, dense=1),
    "local-score-only": ph.case(LOCAL | SCORE_ONLY),
    "local-fit": ph.case(LOCAL | FIT),
    "local-lean-trace": ph.case(LOCAL | LEAN_TRACE),
    "local-level-trace": ph.case(LOCAL | LEVEL_TRACE),
    "local-level-trace-wide": ph.case(LOCAL | LEVEL_TRACE, s=7),
    "local-wide": ph.case(LOCAL, s=6),
    "local-wide-score-only": ph.case(LOCAL | SCORE_ONLY, s=6),
    "local-beta-positive": ph.case(LOCAL, beta=100),
    "plain-tight": ph.case(0, budget=ph.TIGHT),
    "local-tight": ph.case(LOCAL, budget=ph.TIGHT),
    "local-tight-score-only": ph.case(LOCAL | SCORE_ONLY, budget=ph.TIGHT),
    "null-plain": ph.case(0, null=1),
    "null-local": ph.case(LOCAL, null=1),
    "null-local-dense": ph.case(LOCAL, null=1, dense=1),
    "unknown-bit-16": ph.case(16),
    "unknown-bit-32": ph.case(32),
    "unknown-bit-local": ph.case(LOCAL | 0x100),
    "null-unknown-bit": ph.case(32, null=1),
    # what a test can force: without the flag it takes, with the flag it does not
    "plain-forced-pack-x4": ph.case(0, team="x4", pack="1"),
    "local-forced-pack-x4": ph.case(LOCAL, team="x4", pack="1"),
    "plain-forced-3": ph.case(0, team="3", pack="1"),
    "local-forced-3": ph.case(LOCAL, team="3", pack="1"),
    "local-forced-h2": ph.case(LOCAL, s=2, team="h2", pack="1"),
    "local-score-only-forced-3": ph.case(LOCAL | SCORE_ONLY, team="3"),
}


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    got = ph.mode_answers(ph.build(tmp_path_factory.mktemp("localplan")), CASES)
    return {name: dict(g, local=int(g["mode"] == 2)) for name, g in got.items()}


def accepted(got, storage, flags):
    return got["rc"] == 0 and got["local"] == 1 and got["storage"] == storage and got["flags"] == flags and got["msg"] == ""


def test_planner_accepts_local_in_full_storage_and_score_only(plan_lines):
    assert plan_lines["plain-full"]["rc"] == 0 and plan_lines["plain-full"]["local"] == 0
    for name in ("local-full-affine", "local-full-linear", "local-full-s0", "local-full-s5", "local-full-dense"):
        assert accepted(plan_lines[name], 0, LOCAL), name
    assert accepted(plan_lines["local-score-only"], SCORE_ONLY, LOCAL | SCORE_ONLY)
    assert accepted(plan_lines["local-tight-score-only"], SCORE_ONLY, LOCAL | SCORE_ONLY)   # (LEAN records fit the budget)


def test_planner_refuses_local_with_fit(plan_lines):
    got = plan_lines["local-fit"]
    assert got["rc"] == E_INVALID and "LOCAL" in got["msg"] and "FIT" in got["msg"], got


@pytest.mark.parametrize("name", ["local-lean-trace", "local-level-trace", "local-level-trace-wide", "local-wide",
                                  "local-wide-score-only", "local-beta-positive"])
def test_planner_refuses_local_outside_its_modes(plan_lines, name):
    got = plan_lines[name]
    assert got["rc"] == E_UNSUPPORTED and "LOCAL" in got["msg"], got


def test_no_silent_fallback_to_lean_trace(plan_lines):
    """The same pair under the same budget: a plain batch takes LEAN_TRACE by itself, a LOCAL batch is refused."""
    assert plan_lines["plain-tight"]["rc"] == 0 and plan_lines["plain-tight"]["storage"] == LEAN_TRACE
    got = plan_lines["local-tight"]
    assert got["rc"] == E_NOMEM and "LOCAL" in got["msg"] and "LEAN_TRACE" in got["msg"], got


def test_null_batches_pass_local_through(plan_lines):
    assert plan_lines["null-plain"]["rc"] == 0 and plan_lines["null-plain"]["flags"] == SCORE_ONLY
    for name in ("null-local", "null-local-dense"):
        assert accepted(plan_lines[name], SCORE_ONLY, SCORE_ONLY | LOCAL), name


@pytest.mark.parametrize("name", ["unknown-bit-16", "unknown-bit-32", "unknown-bit-local", "null-unknown-bit"])
def test_unknown_flag_bits_stay_invalid(plan_lines, name):
    got = plan_lines[name]
    assert got["rc"] == E_INVALID and "unknown bits" in got["msg"], got


def test_local_plans_no_pack_no_slim_no_cross_cu_team(plan_lines):
    """Every accepted LOCAL case, also where a test forces packed records, a cross-CU team, the slim kernel's team of
    three or eight-wave workgroups -- which the same pairs without the flag do take."""
    for name, got in plan_lines.items():
        if got["local"] and got["rc"] == 0:
            assert got["pack"] == 0 and got["slim"] == 0 and got["gw"] == 1 and got["tw"] in (1, 2, 4, 8), (name, got)
    assert plan_lines["plain-forced-pack-x4"]["pack"] == 1 and plan_lines["plain-forced-pack-x4"]["gw"] == 4
    assert plan_lines["plain-forced-3"]["slim"] == 1 and plan_lines["plain-forced-3"]["tw"] == 3
    for name in ("local-forced-pack-x4", "local-forced-3", "local-forced-h2", "local-score-only-forced-3"):
        assert plan_lines[name]["rc"] == 0 and plan_lines[name]["local"] == 1, name


# ---- the binding ---------------------------------------------------------------------------------------------------

def test_binding_declares_local():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert "bialign_batch_get_local_spans" in names and _lib.BATCH_LOCAL == LOCAL
    with open(os.path.join(REPO, "include", "bialign.h")) as fh:
        header = fh.read()
    assert re.search(r"^#define\s+BIALIGN_BATCH_LOCAL\s+64u\s*$", header, re.M)
    assert re.search(r"^int bialign_batch_get_local_spans\(const bialign_batch\* b, int32_t\* start_a, int32_t\* end_a, "
                     r"int32_t\* start_b, int32_t\* end_b\);", header, re.M)
    assert hasattr(_lib.lib, "bialign_batch_get_local_spans")
    assert _lib.lib.bialign_abi_version() == 10


def test_python_layers_take_local():
    import inspect
    from bialign_amd import batch, engine, significance
    for fn in (significance.null_batch, significance.null_feature_batch, significance.null_dense_batch, significance.zscores,
               significance.zscores_features, significance.zscores_dense, batch.make_batch, batch.make_feature_batch, engine.Batch.__init__):
        assert inspect.signature(fn).parameters["local"].default is False, fn
    assert callable(engine.Batch.local_spans)
    pairs = [synth.protein_pair(1, 5, 6)]
    for fn in (significance.null_batch, significance.zscores):   # refused ahead of any device work
        with pytest.raises(ValueError, match="exclude"):
            fn(pairs, dict(synth.PROTEIN_PARAMS), replicas=2, fit=True, local=True)


# ---- batch_cli --local, the engine stubbed -------------------------------------------------------------------------

class FakeBatch:
    """What batch_cli asks of engine.Batch: pair t's walk is the ungapped alignment of A[sa:ea] with B[sb:eb]."""
    affine = True

    def __init__(self, pairs, spans):
        self.pairs, self.spans, self.closed = pairs, spans, False

    def run(self):
        pass

    def scores(self):
        return np.array([1000 + t for t in range(len(self.pairs))], dtype=np.int32)

    def local_spans(self):
        return tuple(np.array([sp[x] for sp in self.spans], dtype=np.int32) for x in range(4))

    def traces(self):
        return [np.full(ea - sa, 15, dtype=np.uint8) for sa, ea, _, _ in self.spans], np.ones(len(self.spans), dtype=bool)

    def close(self):
        self.closed = True


SPANS = [(0, 3, 2, 5), (1, 4, 1, 4)]


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


ROWS = [("a0", "CDE", "HHE", "b0", "AACDEAA", "CCHHECC"), ("a1", "KACDE", "CHHEE", "b1", "WACDKK", "EHHECC")]
OPTS = ["--type", "Protein", "--simmatrix", "BLOSUM62", "--gap_opening_cost", "-150", "--gap_cost", "-50",
        "--shift_cost", "-150", "--structure_weight", "800", "--max_shift", "1", "--outmode", "sorted"]


def write_rows(tmp_path):
    f = tmp_path / "pairs.tsv"
    f.write_text("".join("\t".join(r) + "\n" for r in ROWS))
    return str(f)


def test_batch_cli_local_blocks(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    assert batch_cli.build_parser().parse_args(["x.tsv"]).local is False
    assert batch_cli.local_span_lines(0, 3, 2, 5) == ["A span\t 1..3", "B span\t 3..5"]
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--local"])
    out = capsys.readouterr().out
    kw = stub_engine["make_batch"][0]
    assert kw["local"] is True and kw["fit"] is False and kw["score_only"] is False
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


def test_batch_cli_local_is_off_by_default(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--score_only"])
    out = capsys.readouterr().out
    assert stub_engine["make_batch"][0]["local"] is False
    assert out.split("\n")[:2] == ["pair 0\ta0\tb0\t1000", "pair 1\ta1\tb1\t1001"] and "span" not in out


def test_batch_cli_local_score_only_and_zscore(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--local", "--score_only", "--zscore", "8"])
    out = capsys.readouterr().out.split("\n")
    assert stub_engine["make_batch"][0]["local"] is True and stub_engine["make_batch"][0]["score_only"] is True
    z = stub_engine["zscores"][0]
    assert z["local"] is True and z["fit"] is False and z["replicas"] == 8
    assert out[0] == "pair 0\ta0\tb0\t1000\t3\t5" and out[2] == "pair 1\ta1\tb1\t1001\t4\t4"   # the 1-based ends of A and B
    assert out[1].startswith("ZSCORE: 2.50 ") and out[3].startswith("ZSCORE: 2.50 ")


def test_batch_cli_refuses_local_with_fit(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    with pytest.raises(SystemExit) as err:
        batch_cli.main([write_rows(tmp_path)] + OPTS + ["--local", "--fit"])
    assert err.value.code == 2 and "exclude" in capsys.readouterr().err and not stub_engine["make_batch"]
