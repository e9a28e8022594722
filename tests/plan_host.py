"""The batch planner on the CPU: build tests/plan_check.hip (host code only), feed it requests, read its plans.
Shared by test_plan_host.py, test_fit_host.py, test_local_host.py (no GPU) and test_gpu_plan_agrees.py (the library reports
the same plans); ``build`` also compiles the other stand-alone host checks around the kernels' headers."""
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "plan_check.hip")
EXPECTED = os.path.join(REPO, "tests", "plan_expected.txt")
MODE_EXPECTED = os.path.join(REPO, "tests", "mode_expected.txt")
SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE, FIT, LOCAL = 1, 2, 4, 8, 64   # bialign_params.flags
E_INVALID, E_UNSUPPORTED, E_NOMEM, E_RANGE = -1, -2, -4, -5   # include/bialign.h


def build(tmp, src=SRC, extra=(), name=None):
    """Compile a stand-alone host program around the headers of bialign_amd/csrc -> the path of the executable."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to compile the host check"
    exe = os.path.join(str(tmp), name or os.path.splitext(os.path.basename(src))[0])
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", *extra,
                    "-I" + os.path.join(REPO, "bialign_amd", "csrc"), "-o", exe, src], check=True)
    return exe


def run(exe, text, env=None):
    """-> the program's whole output for the requests in ``text``."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("BIALIGN_")}
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=dict(clean, **(env or {})))
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout


def request(kind="batch", pairs=(), **kw):
    words = [kind] + [f"{k}={v}" for k, v in kw.items()]
    words.append("pairs=" + ",".join(f"{p[0]}x{p[1]}" + (f"*{p[2]}" if len(p) > 2 else "") for p in pairs))
    return " ".join(words)


def scoring_words(params, pairs):
    """The words of a ``batch`` request that describe a LOOKUP-form batch of these (seqA, seqB, strA, strB) pairs as
    ``batch.make_batch`` hands it to the library: table sizes and maxima, costs, max_shift."""
    import numpy as np
    from bialign_amd.batch import encode_flat
    model, _ = encode_flat(pairs, params)
    s1, s2 = np.asarray(model.s1), np.asarray(model.s2)
    return dict(s=params["max_shift"], k1=s1.shape[0], k2=s2.shape[0], amax=int(np.abs(s1).max()), bmax=int(np.abs(s2).max()),
                beta=params["gap_opening_cost"], gamma=params["gap_cost"], delta=params["shift_cost"])


def ring_dwords(n, s):
    """The ring of the wide-band affine sweep outside the LEVEL forms, per pair: 5 levels x 27 derived values x
    (n + 1) W ceil(W / 2) points, W = 2 s + 1 (bialign_wide.hpp: WIDE_RING, WIDE_SLOT, wide_ring_level_dwords)."""
    w = 2 * s + 1
    return 5 * 27 * (n + 1) * w * ((w + 1) // 2)


class Plan:
    """One answer: rc, msg, and on success the fields of the plan (after a re-plan: ``replanned`` is the second Plan)."""

    def __init__(self, lines):
        first = re.match(r"rc=(-?\d+) msg=(.*)", lines[0])
        self.rc, self.msg = int(first.group(1)), first.group(2)
        self.fields, self.pairs, self.sizes, self.teams, self.chunks, self.order, self.replanned = {}, [], [], [], [], [], None
        self.rings = []   # per pair, plans with a ring term only: ring_dwords, ring_off
        for at, ln in enumerate(lines[1:], 1):
            head, _, rest = ln.partition(" ")
            if head == "replan":
                self.replan = dict(w.split("=", 1) for w in rest.split(" msg=")[0].split())
                self.replanned = Plan([f"rc={self.replan['rc']} msg="] + lines[at + 1:])
                break
            if head == "chunks":
                self.chunks = [int(x) for x in rest.split()]
            elif head == "order":
                self.order = [int(x) for x in rest.split()]
            elif head == "size":
                self.sizes.append({k: int(v) for k, v in (w.split("=") for w in rest.split()[1:])})
            elif head == "ring":
                self.rings.append({k: int(v) for k, v in (w.split("=") for w in rest.split()[1:])})
            elif head == "pair":
                self.pairs.append({k: int(v) for k, v in (w.split("=") for w in rest.split()[1:])})
            elif head == "team":
                self.teams.append({k: int(v) for k, v in (w.split("=") for w in rest.split())})
            else:
                words = ln.split() if "=" in head else rest.split()
                self.fields.update((k, int(v)) for k, v in (w.split("=") for w in words if "=" in w))

    def __getattr__(self, name):
        try:
            return self.fields[name]
        except KeyError:
            raise AttributeError(name)

    @property
    def nchunks(self):
        return len(self.chunks) - 1


def plans(exe, requests, env=None):
    """One Plan per request line (``env`` lines of the input are answered by their echo and skipped)."""
    out = run(exe, "\n".join(requests) + "\n", env)
    blocks = re.split(r"^case \d+: .*\n", out, flags=re.M)[1:]
    assert len(blocks) == len([r for r in requests if not r.startswith("env ")])
    return [Plan([ln for ln in blk.splitlines() if not ln.startswith("env ")]) for blk in blocks]


# ---- the requests behind tests/plan_expected.txt: only `raw` and `env`, which the planner's functions answered under the
# ---- same names before they moved into bialign_plan.hpp -- the file holds that earlier code's answers

def moved_requests():
    s1 = dict(affine=1, s=1, pack=1, num_cu=256, quiet=1)
    out = []
    # the cases team_shape()'s comments quote: pairs x len at max_shift 1, affine, packed records
    headline = [request("raw", [(ln, ln, np)], resid=resid, **s1)
                for ln in (512, 1024) for np in (117, 256, 300, 1280, 2048, 3072, 4096) for resid in (0, 2048)]
    out += headline
    out.append(request("raw", [(928, 933)], resid=2048, **s1))
    out.append(request("raw", [(110, 280, 86), (170, 400, 40)], resid=2048, budget=40 << 20, **s1))
    # max_shift 2: the eight-wave DIET layout (LOOKUP, LDS fits), and without it (dense, or B too long for its LDS)
    s2 = dict(affine=1, s=2, num_cu=256, quiet=1)
    for pairs in ([(2000, 2000, 64)], [(180, 440, 64)], [(512, 512, 300)], [(400, 60000, 8)]):
        for resid, resid8 in ((0, 0), (2048, 0), (2048, 256)):
            out.append(request("raw", pairs, resid=resid, resid8=resid8, **s2))
            out.append(request("raw", pairs, resid=resid, resid8=resid8, pack=1, **s2))
    out.append(request("raw", [(2000, 2000, 64)], resid=2048, resid8=256, dense=1, **s2))
    # max_shift 3 .. 5, packed and not
    for s, pairs in ((3, [(512, 512, 512)]), (3, [(1024, 1024, 21)]), (3, [(700, 700, 86)]), (4, [(300, 300, 100)]), (4, [(2048, 2048, 8)]),
                     (5, [(33, 45, 700)]), (0, [(200, 200, 900)]), (0, [(3000, 3000, 4)])):
        for resid in (0, 2048):
            out.append(request("raw", pairs, affine=1, s=s, pack=int(s == 3), num_cu=256, resid=resid, quiet=1))
    # the one-layer recurrence
    for s in (0, 1, 2, 3, 5):
        for pairs in ([(512, 512, 300)], [(1500, 1500, 16)]):
            for resid in (0, 2048):
                out.append(request("raw", pairs, affine=0, s=s, beta=0, num_cu=256, resid=resid, quiet=1))
    # dense forms, LEAN records, FEATURE tables inside the chunk plan
    for s in (1, 2, 4):
        for form in (dict(dense=1), dict(dense1=1), dict(dense=1, dense1=1)):
            for affine in (1, 0):
                out.append(request("raw", [(600, 600, 40)], affine=affine, s=s, num_cu=256, resid=2048, quiet=1, **form))
    for s in (1, 2, 3):
        for np in (64, 1280):
            out.append(request("raw", [(512, 512, np)], affine=1, s=s, lean=1, num_cu=256, resid=2048, resid8=256, quiet=1))
    ragged = [(41, 46), (64, 300), (300, 64), (17, 18), (1, 1), (100, 100), (5, 90), (90, 5), (64, 64), (250, 260)]
    for budget in (1 << 40, 24 << 20, 6 << 20):
        out.append(request("raw", ragged, affine=1, s=1, pack=1, num_cu=256, resid=2048, budget=budget))
        out.append(request("raw", ragged, affine=1, s=2, feat=1, num_cu=256, resid=2048, budget=budget))
        out.append(request("raw", ragged, affine=0, s=3, beta=0, num_cu=256, resid=0, budget=budget))
    out.append(request("raw", ragged, affine=1, s=1, num_cu=256, budget=1 << 20))   # one pair exceeds the budget
    out.append(request("raw", ragged, affine=1, s=1, feat=1, num_cu=256, budget=1 << 20))
    out.append(request("raw", [(512, 512, 300)], affine=1, s=1, pack=1, num_cu=304, resid=2432, quiet=1))  # another device size
    # forced teams and the two-wave kernels only
    forced = [request("raw", [(1024, 1024, np)], resid=2048, **s1) for np in (117, 300)] + \
             [request("raw", [(512, 512, 2048)], resid=2048, **s1), request("raw", [(110, 280, 6)], resid=2048, **s1),
              request("raw", [(2000, 2000, 64)], resid=2048, resid8=256, **s2), request("raw", [(512, 512, 300)], resid=2048, **s2),
              request("raw", [(512, 512, 300)], affine=0, s=1, beta=0, num_cu=256, resid=2048, quiet=1)]
    for team in ("2", "3", "x4", "h2"):
        out += [f"env BIALIGN_TEAM={team}"] + forced
    out += ["env BIALIGN_TEAM=", "env BIALIGN_SLIM=0"] + headline + ["env BIALIGN_SLIM="]
    return out


# ---- one alignment mode per batch: two pairs of 300 x 400 (full layers at max_shift 1: ~42 MB a pair, LEAN: ~2 MB), on a
# ---- device that would hold cross-CU teams

SMALL = dict(amax=1100, bmax=800, gamma=-50, delta=-150, num_cu=256, resid=4096, resid8=512, quiet=1)
ROOMY, TIGHT = 1 << 36, 16 << 20


def case(flags, s=1, beta=-150, budget=ROOMY, **kw):
    """dense=1: mu1 and mu2 as tables; null=1: a null batch; team, pack: the BIALIGN_TEAM / BIALIGN_PACK a test would force"""
    return dict(flags=flags, s=s, beta=beta, budget=budget, **kw)


def mode_answers(exe, cases):
    """cases: name -> case(...).  -> name -> dict(rc, mode, storage, flags, pack, tw, gw, slim, msg), the team shape being
    the first chunk's."""
    lines = []
    for c in cases.values():
        words = dict(SMALL, flags=c["flags"], s=c["s"], beta=c["beta"], budget=c["budget"])
        if c.get("dense"):
            words.update(form="mu12", mu1=100, mu2=100)
        if c.get("null"):
            words.update(replicas=4, seed=7)
        lines += [f"env BIALIGN_TEAM={c.get('team', '')}", f"env BIALIGN_PACK={c.get('pack', '')}", request(pairs=[(300, 400, 2)], **words)]
    got = {}
    for name, p in zip(cases, plans(exe, lines)):
        team = p.teams[0] if p.teams else dict(tw=1, gw=1, slim=0)
        got[name] = dict(rc=p.rc, mode=p.mode, storage=p.fields.get("storage", 0), flags=p.flags, pack=p.fields.get("pack", 0),
                         tw=team["tw"], gw=team["gw"], slim=team["slim"], msg=p.msg)
    return got


# ---- the requests behind tests/mode_expected.txt: every mode against every storage flag, band, gap opening cost and
# ---- budget, and a few null batches and unknown bits -- the file holds the answers of the planner that kept FIT and LOCAL
# ---- as two booleans (its `batch` answers had no `mode=` line: drop_mode_lines)

def mode_requests():
    modes = (0, FIT, LOCAL, FIT | LOCAL)
    out = [request(pairs=[(300, 400, 2)], flags=mode | storage, s=s, beta=beta, budget=budget, **SMALL)
           for mode in modes for storage in (0, SCORE_ONLY, LEAN_TRACE, LEVEL_TRACE) for s in (1, 6) for beta in (-150, 0, 100)
           for budget in (ROOMY, TIGHT)]
    out += [request(pairs=[(300, 400, 2)], flags=mode, s=1, beta=beta, budget=ROOMY, replicas=4, seed=7, **SMALL)
            for mode in modes for beta in (-150, 100)]
    out += [request(pairs=[(300, 400, 2)], flags=mode | bit, s=1, beta=-150, budget=ROOMY, **SMALL) for mode in modes for bit in (16, 0x100)]
    out.append(request(pairs=[(300, 400, 2)], flags=LOCAL | 32, s=1, beta=-150, budget=ROOMY, replicas=4, seed=7, **SMALL))
    return out


def drop_mode_lines(text):
    return re.sub(r"^mode=\d flags=\d+\n", "", text, flags=re.M)
