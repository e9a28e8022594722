"""The batch planner on the CPU: build tests/plan_check.hip (host code only), feed it requests, read its plans.
Shared by test_plan_host.py (no GPU) and test_gpu_plan_agrees.py (the library reports the same plans)."""
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "plan_check.hip")
EXPECTED = os.path.join(REPO, "tests", "plan_expected.txt")
E_INVALID, E_UNSUPPORTED, E_NOMEM, E_RANGE = -1, -2, -4, -5   # include/bialign.h


def build(tmp, name="plan_check", extra=()):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to compile the host check"
    exe = os.path.join(str(tmp), name)
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", *extra,
                    "-I" + os.path.join(REPO, "bialign_amd", "csrc"), "-o", exe, SRC], check=True)
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


class Plan:
    """One answer: rc, msg, and on success the fields of the plan (after a re-plan: ``replanned`` is the second Plan)."""

    def __init__(self, lines):
        first = re.match(r"rc=(-?\d+) msg=(.*)", lines[0])
        self.rc, self.msg = int(first.group(1)), first.group(2)
        self.fields, self.pairs, self.sizes, self.teams, self.chunks, self.order, self.replanned = {}, [], [], [], [], [], None
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
