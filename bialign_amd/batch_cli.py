"""Batch front end: align many pairs in one GPU launch.

    python -m bialign_amd.batch_cli pairs.tsv --type Protein --simmatrix BLOSUM62 \\
        --gap_opening_cost -150 --gap_cost -50 --shift_cost -150 --structure_weight 800 --max_shift 1

``pairs.tsv``: one pair per line, tab separated ``nameA seqA strA nameB seqB strB`` (lines
starting with ``#`` are skipped).  All scoring / output options of ``bialign.py`` apply to every
pair.  For each pair the output is the reference CLI's block (``Input:`` echo, ``SCORE:``, the
decoded alignment in the chosen ``--outmode``) behind a ``>pair`` header line.  Under
``torchrun`` (one process per GPU) the pairs are sharded over the ranks; every rank prints its
own pairs, rank 0 additionally a ``#scores`` line with all gathered scores.

``--zscore R`` adds one line behind each pair's block: where the score lies among the scores of A against R shuffles
of B (``bialign_amd.significance``; the shuffles are made and scored on the GPU),
``ZSCORE: <z> (mean <mean>, sd <sd>, <n_ge>/<R> shuffles >= score)``.  Without the option the output is unchanged.
``--zscore_shuffle {mono,dinucleotide}`` names the null model of those shuffles (``mono``, the default, keeps B's letter
composition; ``dinucleotide`` keeps the count of every ordered pair of neighbouring letters, the accepted null for nucleic
acids); given the option, the output opens with a header line ``#zscore_shuffle\t<model>``.  Not without ``--zscore``.

``--fit`` aligns every pair's molecule A with the best-scoring substring of its molecule B (fit alignments, free end
gaps in B: include/bialign.h, BIALIGN_BATCH_FIT).  The alignment is decoded on that substring, one extra line
``B span\t <start_b+1>..<end_b>`` (1-based, inclusive) follows ``SCORE:``, ``--score_only`` lines gain the 1-based end
as a fourth column, and ``--zscore`` scores the shuffles in the same mode.

``--local`` aligns the best-scoring part of every pair's molecule A with the best-scoring part of its molecule B (local
alignments, the ends of both molecules free: include/bialign.h, BIALIGN_BATCH_LOCAL; not with ``--fit``).  Two extra
lines ``A span\t <start_a+1>..<end_a>`` and ``B span\t <start_b+1>..<end_b>`` (1-based, inclusive) follow ``SCORE:``,
the alignment is decoded on the two windows, ``--score_only`` lines gain the 1-based ends of A and B as a fourth and
fifth column, and ``--zscore`` scores the shuffles in the same mode.

``--overlap`` aligns every pair end to end on the stretch its molecules share, with the end gaps of both molecules free
(overlap alignments: include/bialign.h, BIALIGN_BATCH_OVERLAP; not with ``--fit`` or ``--local``).  The output has the
form of ``--local``: the ``A span`` and ``B span`` lines, the alignment decoded on the two windows, the 1-based ends as
fourth and fifth column under ``--score_only``, ``--zscore`` in the same mode.

``--fit --hits K --hit_min_score X`` also searches every pair for up to K disjoint placements of A in B that score at
least X (include/bialign.h, "Hit search").  Behind each pair's block follow ``HITS: <n> (<status>)`` and one line per hit
in the form of ``--fit``'s span line behind a hit index, ``hit <h>\tB span\t <start_b+1>..<end_b>\t<score>``; hit 0 is the
pair's own alignment.  Not without ``--fit``, not with ``--score_only`` or ``--zscore``.  ``--hit_peaks`` takes only the
peaks of a pair's end-score profile as candidates, which finds the farther copies of A within the default walk budget;
``--hit_min_permille N`` also asks of a placement N thousandths of the pair's own fit score.  Both need ``--hits``.
"""
import argparse
import sys

from . import bialignment
from .cli import _OPTIONS

_PER_PAIR = {"seqA", "seqB", "--strA", "--strB", "--nameA", "--nameB", "--fileinput", "--version"}


def read_pairs(path):
    pairs = []
    with open(path) as fh:
        for ln, line in enumerate(fh, start=1):
            line = line.rstrip("\n")
            if not line.strip() or line.startswith("#"):
                continue
            cols = line.split("\t")
            if len(cols) != 6:
                raise ValueError(f"{path}:{ln}: expected 6 tab-separated fields, got {len(cols)}")
            pairs.append(tuple(cols))
    if not pairs:
        raise ValueError(f"{path}: no pairs")
    return pairs


def build_parser():
    p = argparse.ArgumentParser(description="Batch bialignment on the GPU.")
    p.add_argument("pairs", help="TSV file: nameA seqA strA nameB seqB strB")
    for flags, kwargs in _OPTIONS:
        if flags[0] not in _PER_PAIR:
            p.add_argument(*flags, **kwargs)
    p.add_argument("--score_only", action="store_true",
                   help="Print one 'pair nameA nameB score' line per pair and skip the alignments "
                        "(the GPU then keeps a fraction of the DP layers: faster, far less memory).")
    p.add_argument("--zscore", type=int, default=0, metavar="R",
                   help="Also print each pair's z-score against R shuffles of molecule B (1..65535), as a "
                        "'ZSCORE:' line behind the pair's block.")
    p.add_argument("--zscore_shuffle", choices=("mono", "dinucleotide"), default=None,
                   help="With --zscore: the null model of the shuffles. mono (the default) keeps molecule B's letter "
                        "composition, dinucleotide the count of every ordered pair of neighbouring letters. "
                        "Names the model in a '#zscore_shuffle' header line.")
    p.add_argument("--fit", action="store_true",
                   help="Fit alignments: molecule A against the best substring of molecule B (B's end gaps are free); "
                        "prints the substring as a 'B span' line behind 'SCORE:'.")
    p.add_argument("--local", action="store_true",
                   help="Local alignments: the best-scoring part of molecule A against the best-scoring part of molecule "
                        "B (the ends of both are free); prints the parts as 'A span' and 'B span' lines behind 'SCORE:'. "
                        "Not with --fit.")
    p.add_argument("--overlap", action="store_true",
                   help="Overlap alignments: the global alignment whose end gaps are free in both molecules (dovetails, "
                        "containment in either direction); prints the aligned stretch as 'A span' and 'B span' lines "
                        "behind 'SCORE:'. Not with --fit or --local.")
    p.add_argument("--hits", type=int, default=0, metavar="K",
                   help="With --fit: also search every pair for up to K (1..256) disjoint placements of molecule A in "
                        "molecule B and print one 'hit' line each behind the pair's block. Not with --score_only or --zscore.")
    p.add_argument("--hit_min_score", type=int, default=None, metavar="X",
                   help="The least score (>= 1) of a placement that --hits reports; required with --hits.")
    p.add_argument("--hit_peaks", action="store_true",
                   help="With --hits: only the peaks of a pair's end-score profile are candidate ends (the ends just "
                        "behind a reported placement are not tried one by one).")
    p.add_argument("--hit_min_permille", type=int, default=None, metavar="N",
                   help="With --hits: a placement must also score at least N thousandths (0..1000) of the pair's fit score.")
    p.add_argument("--zscore_seed", type=int, default=0, metavar="N",
                   help="Seed of the shuffles (default 0); shuffle r of a pair is a function of the seed, r and the "
                        "pair's position among the pairs its process aligns.")
    return p


def zscore_line(z, t):
    """The ZSCORE line of pair t from ``significance.zscores`` results."""
    return (f"ZSCORE: {z['z'][t]:.2f} (mean {z['mean'][t]:.1f}, sd {z['std'][t]:.1f}, "
            f"{int(z['n_ge'][t])}/{int(z['replicas'][t])} shuffles >= score)")


def span_line(start_b, end_b):
    """The line behind ``SCORE:`` of a ``--fit`` pair: the aligned part of B, 1-based and inclusive (an empty part, where
    all of A is gapped, reads start_b+1..start_b)."""
    return f"B span\t {int(start_b) + 1}..{int(end_b)}"


def hit_line(h, start_b, end_b, score):
    """The line of hit ``h`` of a ``--hits`` pair: ``--fit``'s span line behind the hit index, then the hit's score."""
    return f"hit {h}\t{span_line(start_b, end_b)}\t{int(score)}"


def check_hit_options(parser, args):
    """``--hits`` / ``--hit_min_score`` and the two options that refine them -> ``hits=`` of ``make_batch`` (today's tuple, or a dict once one of
    ``--hit_peaks`` / ``--hit_min_permille`` is given) or None; a parser error where they do not apply."""
    if not args.hits and (args.hit_peaks or args.hit_min_permille is not None):
        parser.error("--hit_peaks and --hit_min_permille need --hits")
    if not args.hits and args.hit_min_score is None:
        return None
    if not args.hits or args.hit_min_score is None:
        parser.error("--hits and --hit_min_score go together")
    if not args.fit:
        parser.error("--hits needs --fit")
    if args.score_only or args.zscore:
        parser.error("--hits excludes --score_only and --zscore")
    from .batch import check_hit_rules, check_hit_spec
    try:
        spec = check_hit_spec(args.hits, args.hit_min_score)
        if not args.hit_peaks and args.hit_min_permille is None:
            return spec
        peaks, _, permille = check_hit_rules(args.hit_peaks, None, args.hit_min_permille or 0)
        return dict(max_hits=spec[0], min_score=spec[1], max_walks=spec[2], peaks=peaks, min_permille=permille)
    except ValueError as e:
        parser.error(str(e))


def local_span_lines(start_a, end_a, start_b, end_b):
    """The lines behind ``SCORE:`` of a ``--local`` or ``--overlap`` pair: the aligned parts of A and B, 1-based and inclusive (an empty
    part reads start+1..start)."""
    return [f"A span\t {int(start_a) + 1}..{int(end_a)}", span_line(start_b, end_b)]


def fit_window(seq_b, str_b, start_b, end_b, rna):
    """``B[start_b:end_b]`` as the decoder takes it.  RNA: a bracket whose partner lies outside the window becomes
    ``.``, so that the window's structure is a balanced dot-bracket string again."""
    seq, struct = seq_b[start_b:end_b], list(str_b[start_b:end_b])
    if rna:
        stack = []
        for x, ch in enumerate(struct):
            if ch == "(":
                stack.append(x)
            elif ch == ")":
                if stack:
                    stack.pop()
                else:
                    struct[x] = "."
        for x in stack:
            struct[x] = "."
    return seq, "".join(struct)


def pair_block(idx, rec, params, score, trace, complete, verbose, span=None, local_span=None):
    """Output lines of one pair, framed like the reference CLI (bialign.py:109-124).  ``span``: ``(start_b, end_b)`` of
    a ``--fit`` pair, whose alignment is decoded on that part of B.  ``local_span``: ``(start_a, end_a, start_b, end_b)``
    of a ``--local`` or ``--overlap`` pair, whose alignment is decoded on those parts of A and B."""
    name_a, seq_a, str_a, name_b, seq_b, str_b = rec
    yield f">pair {idx}\t{name_a}\t{name_b}"
    yield "Input:"
    yield "seqA\t " + seq_a
    yield "seqB\t " + seq_b
    yield "strA\t " + str_a
    yield "strB\t " + str_b
    yield "SCORE: " + str(score)
    if span is not None:
        yield span_line(*span)
        seq_b, str_b = fit_window(seq_b, str_b, int(span[0]), int(span[1]), params.get("type") == "RNA")
    if local_span is not None:
        yield from local_span_lines(*local_span)
        rna = params.get("type") == "RNA"
        seq_a, str_a = fit_window(seq_a, str_a, int(local_span[0]), int(local_span[1]), rna)
        seq_b, str_b = fit_window(seq_b, str_b, int(local_span[2]), int(local_span[3]), rna)
    yield ""
    aligner = bialignment.BiAligner(seq_a, seq_b, str_a, str_b, **dict(params, nameA=name_a, nameB=name_b))
    if not complete:
        yield "WARNING: incomplete traceback. Alignment could be garbage."
    yield from aligner.decode_trace(trace)
    if verbose and aligner._affine:
        yield from aligner.eval_trace(trace)


def main(argv=None):
    """Engine refusals (e.g. --score_only with --max_shift above 5, scores outside the int32 window) end like the
    reference's own input errors (pyx:207-210): ``ERROR: <text>`` and exit status 255, not a Python traceback."""
    from ._lib import BialignError
    try:
        return _main(argv)
    except BialignError as e:
        print("ERROR: " + e.message)
        sys.exit(-1)


def _main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.fit and args.local:
        parser.error("--fit and --local exclude each other")
    if args.overlap and (args.fit or args.local):
        parser.error("--overlap excludes --fit and --local")
    hits = check_hit_options(parser, args)
    if args.zscore_shuffle and not args.zscore:
        parser.error("--zscore_shuffle needs --zscore")
    params = {k: v for k, v in vars(args).items()
              if k not in ("pairs", "verbose", "score_only", "zscore", "zscore_seed", "zscore_shuffle", "fit", "local", "overlap", "hits", "hit_min_score", "hit_peaks", "hit_min_permille")}
    if args.zscore:
        from .significance import check_null
        check_null((args.zscore, args.zscore_seed))
    records = read_pairs(args.pairs)
    from .batch import make_batch, pair_cost, shard
    from .distributed import gather_scores, init_from_env
    from .engine import default_engine, trace_codes_to_columns
    rank, local_rank, world = init_from_env()
    costs = [pair_cost((r[1], r[4]), params["max_shift"]) for r in records]  # shards balanced by lattice cells
    mine = shard(len(records), rank, world, costs)
    if args.zscore_shuffle and rank == 0:
        print(f"#zscore_shuffle\t{args.zscore_shuffle}")
    scores = []
    if len(mine):
        batch = make_batch([(r[1], r[4], r[2], r[5]) for r in (records[p] for p in mine)], params,
                           engine=default_engine(local_rank), score_only=args.score_only, fit=args.fit,
                           local=args.local, overlap=args.overlap, hits=hits)
        batch.run()
        scores = batch.scores()
        start_b, end_b = batch.fit_spans() if args.fit else (None, None)
        lspans = batch.local_spans() if args.local else batch.overlap_spans() if args.overlap else None
        z = None
        if args.zscore:
            from .significance import zscores
            z = zscores([(r[1], r[4], r[2], r[5]) for r in (records[p] for p in mine)], params, replicas=args.zscore,
                        seed=args.zscore_seed, observed=scores, engine=default_engine(local_rank), fit=args.fit, local=args.local,
                        overlap=args.overlap, shuffle=args.zscore_shuffle or "mono")
        if args.score_only:
            for t, p in enumerate(mine):
                print(f"pair {p}\t{records[p][0]}\t{records[p][3]}\t{int(scores[t])}" + (f"\t{int(end_b[t])}" if args.fit else "") +
                      (f"\t{int(lspans[1][t])}\t{int(lspans[3][t])}" if lspans else ""))
                if z:
                    print(zscore_line(z, t))
        else:
            traces, complete = batch.traces()
            found, status = batch.fit_hits() if hits else (None, None)
            for t, p in enumerate(mine):
                trace = trace_codes_to_columns(traces[t], as_tuples=not batch.affine)
                span = (int(start_b[t]), int(end_b[t])) if args.fit and complete[t] else None
                lspan = tuple(int(x[t]) for x in lspans) if lspans and complete[t] else None
                for line in pair_block(p, records[p], params, int(scores[t]), trace, bool(complete[t]), args.verbose, span, lspan):
                    print(line)
                if hits:
                    print(f"HITS: {len(found[t])} ({status[t]})")
                    for h, (hs, he, hscore, _) in enumerate(found[t]):
                        print(hit_line(h, hs, he, hscore))
                if z:
                    print(zscore_line(z, t))
        batch.close()
    if world > 1:
        allscores = gather_scores(scores, len(records), costs)
        if rank == 0:
            print("#scores\t" + "\t".join(str(int(s)) for s in allscores))
    return 0


if __name__ == "__main__":
    sys.exit(main())
