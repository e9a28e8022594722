"""Fit alignments (BIALIGN_BATCH_FIT), what can be checked without a GPU:

  * the expectation the GPU tests rely on (tests/fit_expected.py: one oracle fill per start of the substring) against
    plain ``oracle.solve`` on explicitly cut substrings;
  * the planner's decisions about the flag -- where it is accepted, its refusals, no silent fallback to LEAN_TRACE,
    null batches pass it through, unknown flag bits are refused -- as ``batch`` requests to tests/plan_check.hip, the
    stand-alone host program around bialign_plan.hpp;
  * ``batch_cli --fit``: argument handling and the span line, with the engine stubbed;
  * the binding declares the new entry point."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_expected as fe
import plan_host as ph
from bialign_amd import _lib, synth
from oracle import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE, FIT = 1, 2, 4, 8
E_INVALID, E_UNSUPPORTED, E_NOMEM = -1, -2, -4


# ---- the helper against plain global alignments of cut substrings --------------------------------------------------

@pytest.mark.parametrize("seed,n,m,beta,s", [(11, 5, 9, -150, 1), (12, 6, 8, 0, 2)], ids=["affine", "one-layer"])
def test_expectation_equals_global_scores_of_cut_substrings(seed, n, m, beta, s):
    params = dict(synth.PROTEIN_PARAMS, gap_opening_cost=beta, max_shift=s)
    sa, sb, ta, tb = pair = synth.protein_pair(seed, n, m)
    want = fe.fit_expected(n, m, params, *fe.tables_of(pair, params))
    best = want["glob"][0, 0]   # the empty substring: all of A against nothing
    assert (np.diag(want["glob"]) == best).all()
    for j0 in range(m):
        for j1 in range(j0 + 1, m + 1):
            cut = oracle.solve(sa, sb[j0:j1], ta, tb[j0:j1], params, want_trace=False)["score"]
            assert want["glob"][j0, j1] == cut, (j0, j1)
            best = max(best, cut)
    assert want["score"] == best
    ends = [max(want["glob"][:j1 + 1, j1]) for j1 in range(m + 1)]
    assert want["end_b"] == ends.index(best)
    # the FIT layers at the end cells are the substrings' maxima, and row 0's diagonal starts at 0
    lay = want["layers"]
    for j1 in range(m + 1):
        assert lay[:, n, j1, s, s].max() == ends[j1]
        assert lay[-1, 0, j1, s, s] >= 0
    assert lay[-1, 0, 0, s, s] == 0


# ---- the planner ---------------------------------------------------------------------------------------------------

CASES = {   # two pairs of 300 x 400: full layers at max_shift 1 ~42 MB a pair (packed: about half), the LEAN form ~2 MB
    "plain-full": ph.case(0),
    "fit-full-affine": ph.case(FIT),
    "fit-full-linear": ph.case(FIT, s=2, beta=0),
    "fit-full-s5": ph.case(FIT, s=5),
    "fit-full-dense": ph.case(FIT, dense=1),
    "fit-score-only": ph.case(FIT | SCORE_ONLY),
    "fit-lean-trace": ph.case(FIT | LEAN_TRACE),
    "fit-level-trace": ph.case(FIT | LEVEL_TRACE),
    "fit-level-trace-wide": ph.case(FIT | LEVEL_TRACE, s=7),
    "fit-wide": ph.case(FIT, s=6),
    "fit-wide-score-only": ph.case(FIT | SCORE_ONLY, s=6),
    "plain-tight": ph.case(0, budget=ph.TIGHT),
    "fit-tight": ph.case(FIT, budget=ph.TIGHT),
    "fit-tight-score-only": ph.case(FIT | SCORE_ONLY, budget=ph.TIGHT),
    "null-plain": ph.case(0, null=1),
    "null-fit": ph.case(FIT, null=1),
    "null-fit-dense": ph.case(FIT, null=1, dense=1),
    "unknown-bit": ph.case(16),
    "unknown-bit-fit": ph.case(FIT | 0x100),
    "null-unknown-bit": ph.case(32, null=1),
}


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    got = ph.mode_answers(ph.build(tmp_path_factory.mktemp("fitplan")), CASES)
    return {name: dict(rc=g["rc"], fit=int(g["mode"] == 1), storage=g["storage"], flags=g["flags"], msg=g["msg"]) for name, g in got.items()}


def test_planner_accepts_fit_in_full_storage_and_score_only(plan_lines):
    assert plan_lines["plain-full"] == dict(rc=0, fit=0, storage=0, flags=0, msg="")
    for name in ("fit-full-affine", "fit-full-linear", "fit-full-s5", "fit-full-dense"):
        assert plan_lines[name] == dict(rc=0, fit=1, storage=0, flags=FIT, msg=""), name
    assert plan_lines["fit-score-only"] == dict(rc=0, fit=1, storage=SCORE_ONLY, flags=FIT | SCORE_ONLY, msg="")
    assert plan_lines["fit-tight-score-only"]["rc"] == 0   # (LEAN records fit the budget the full layers exceed)


@pytest.mark.parametrize("name", ["fit-lean-trace", "fit-level-trace", "fit-level-trace-wide", "fit-wide", "fit-wide-score-only"])
def test_planner_refuses_fit_outside_its_modes(plan_lines, name):
    got = plan_lines[name]
    assert got["rc"] == E_UNSUPPORTED and "FIT" in got["msg"], got


def test_no_silent_fallback_to_lean_trace(plan_lines):
    """The same pair under the same budget: a plain batch takes LEAN_TRACE by itself, a FIT batch is refused."""
    assert plan_lines["plain-tight"]["rc"] == 0 and plan_lines["plain-tight"]["storage"] == LEAN_TRACE
    got = plan_lines["fit-tight"]
    assert got["rc"] == E_NOMEM and "FIT" in got["msg"] and "LEAN_TRACE" in got["msg"], got


def test_null_batches_pass_fit_through(plan_lines):
    assert plan_lines["null-plain"] == dict(rc=0, fit=0, storage=SCORE_ONLY, flags=SCORE_ONLY, msg="")
    for name in ("null-fit", "null-fit-dense"):
        assert plan_lines[name] == dict(rc=0, fit=1, storage=SCORE_ONLY, flags=SCORE_ONLY | FIT, msg=""), name


@pytest.mark.parametrize("name", ["unknown-bit", "unknown-bit-fit", "null-unknown-bit"])
def test_unknown_flag_bits_are_invalid(plan_lines, name):
    got = plan_lines[name]
    assert got["rc"] == E_INVALID and "unknown bits" in got["msg"], got


# ---- the binding ---------------------------------------------------------------------------------------------------

def test_binding_declares_fit():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert "bialign_batch_get_fit_spans" in names and _lib.BATCH_FIT == FIT
    with open(os.path.join(REPO, "include", "bialign.h")) as fh:
        header = fh.read()
    assert re.search(r"^#define\s+BIALIGN_BATCH_FIT\s+8u\s*$", header, re.M)
    assert re.search(r"^int bialign_batch_get_fit_spans\(const bialign_batch\* b, int32_t\* start_b, int32_t\* end_b\);", header, re.M)
    assert hasattr(_lib.lib, "bialign_batch_get_fit_spans")


# ---- batch_cli --fit, the engine stubbed ---------------------------------------------------------------------------

class FakeBatch:
    """What batch_cli asks of engine.Batch: pair t's walk is the ungapped alignment of A with B[start:end]."""
    affine = True

    def __init__(self, pairs, spans):
        self.pairs, self.spans, self.closed = pairs, spans, False

    def run(self):
        pass

    def scores(self):
        return np.array([1000 + t for t in range(len(self.pairs))], dtype=np.int32)

    def fit_spans(self):
        return (np.array([s for s, _ in self.spans], dtype=np.int32), np.array([e for _, e in self.spans], dtype=np.int32))

    def traces(self):
        return [np.full(e - s, 15, dtype=np.uint8) for s, e in self.spans], np.ones(len(self.spans), dtype=bool)

    def close(self):
        self.closed = True


@pytest.fixture
def stub_engine(monkeypatch):
    from bialign_amd import batch, distributed, engine, significance
    calls = dict(make_batch=[], zscores=[])
    spans = [(2, 5), (0, 4)]

    def make_batch(pairs, params, **kw):
        calls["make_batch"].append(kw)
        return FakeBatch(pairs, spans[:len(pairs)])

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


ROWS = [("a0", "CDE", "HHE", "b0", "AACDEAA", "CCHHECC"), ("a1", "ACDE", "HHEE", "b1", "ACDEKK", "HHEECC")]
OPTS = ["--type", "Protein", "--simmatrix", "BLOSUM62", "--gap_opening_cost", "-150", "--gap_cost", "-50",
        "--shift_cost", "-150", "--structure_weight", "800", "--max_shift", "1", "--outmode", "sorted"]


def write_rows(tmp_path):
    f = tmp_path / "pairs.tsv"
    f.write_text("".join("\t".join(r) + "\n" for r in ROWS))
    return str(f)


def test_batch_cli_fit_blocks(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    assert batch_cli.build_parser().parse_args(["x.tsv"]).fit is False
    assert batch_cli.span_line(2, 5) == "B span\t 3..5"
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--fit"])
    out = capsys.readouterr().out
    assert stub_engine["make_batch"][0]["fit"] is True and stub_engine["make_batch"][0]["score_only"] is False
    blocks = out.split(">pair ")[1:]
    assert len(blocks) == 2
    for t, (blk, (start, end)) in enumerate(zip(blocks, [(2, 5), (0, 4)])):
        lines = blk.split("\n")
        at = lines.index(f"SCORE: {1000 + t}")
        assert lines[at + 1] == f"B span\t {start + 1}..{end}" and lines[at + 2] == ""
        assert "seqB\t " + ROWS[t][4] in lines             # the input echo shows all of B
        rows = [ln for ln in lines[at + 3:] if ln.startswith(ROWS[t][3] + " ") and "shifts" not in ln]
        assert rows and all(ln.split()[-1] in (ROWS[t][4][start:end], ROWS[t][5][start:end]) for ln in rows), rows


def test_batch_cli_fit_is_off_by_default(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--score_only"])
    out = capsys.readouterr().out
    assert stub_engine["make_batch"][0]["fit"] is False
    assert out.split("\n")[:2] == ["pair 0\ta0\tb0\t1000", "pair 1\ta1\tb1\t1001"] and "B span" not in out


def test_batch_cli_fit_score_only_and_zscore(tmp_path, capsys, stub_engine):
    from bialign_amd import batch_cli
    batch_cli.main([write_rows(tmp_path)] + OPTS + ["--fit", "--score_only", "--zscore", "8"])
    out = capsys.readouterr().out.split("\n")
    assert stub_engine["make_batch"][0]["fit"] is True and stub_engine["make_batch"][0]["score_only"] is True
    assert stub_engine["zscores"][0]["fit"] is True and stub_engine["zscores"][0]["replicas"] == 8
    assert out[0] == "pair 0\ta0\tb0\t1000\t5" and out[2] == "pair 1\ta1\tb1\t1001\t4"   # the 1-based end = end_b
    assert out[1].startswith("ZSCORE: 2.50 ") and out[3].startswith("ZSCORE: 2.50 ")


def test_fit_window_keeps_rna_structures_balanced():
    from bialign_amd import batch_cli
    seq, struct = "ACGUACGUAC", "((..)).(.)"
    assert batch_cli.fit_window(seq, struct, 1, 6, True) == ("CGUAC", "(..).")
    assert batch_cli.fit_window(seq, struct, 0, 10, True) == (seq, struct)
    assert batch_cli.fit_window(seq, struct, 4, 9, True) == ("ACGUA", ".....")
    assert batch_cli.fit_window(seq, struct, 6, 10, True) == ("GUAC", ".(.)")
    assert batch_cli.fit_window("ACDEF", "HHEEC", 1, 4, False) == ("CDE", "HEE")


def test_significance_takes_fit():
    import inspect
    from bialign_amd import batch, engine, significance
    for fn in (significance.null_batch, significance.null_feature_batch, significance.null_dense_batch, significance.zscores,
               significance.zscores_features, significance.zscores_dense, batch.make_batch, batch.make_feature_batch, engine.Batch.__init__):
        assert inspect.signature(fn).parameters["fit"].default is False, fn
