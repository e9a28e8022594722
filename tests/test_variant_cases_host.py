"""The closure of tests/variant_cases.py, on the CPU: every sweep and walk that bialign_host.hpp instantiates has a case
(or a planner-proven entry in the unreachable list), every case plans as it claims, and the tie-dense inputs are tie-dense.

What exists comes from tests/variant_check.hip, which calls the predicates themselves; what a case plans comes from
tests/plan_check.hip, the planner the library runs.  A wrong shape fails here, before any GPU time."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_host as ph
import variant_cases as vc

VARIANT_SRC = os.path.join(ph.REPO, "tests", "variant_check.hip")
SWITCHES = vc.SWITCHES
#: the device plan_check is told of: room for every cross-CU team of the table
DEVICE = dict(num_cu=256, resid=4096, resid8=512, quiet=1)
#: what the issue counted from the predicates
FAMILY_COUNTS = dict(fill_affine=359, fill_linear=252, fill_slim=8)
MIN_TIE_DENSITY = 0.9


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """{key: instantiated by a ladder}, from the predicates."""
    import subprocess
    exe = ph.build(tmp_path_factory.mktemp("variants"), src=VARIANT_SRC)
    return vc.parse_variants(subprocess.run([exe], capture_output=True, text=True, check=True, timeout=600).stdout)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return ph.build(tmp_path_factory.mktemp("plan"))


def plan_lines(c):
    """The requests that make plan_check plan a case: its switches, then its batch."""
    words = ph.scoring_words(c.params(), [vc.pair_of(c.shape, c.kind)])
    if c.form != "lookup":      # (the tables' largest entries, as variant_cases.tables_of draws them)
        words.update(form=c.form, mu1=1100, mu2=900)
    env = c.environ
    assert set(env) <= set(SWITCHES)
    return [f"env {name}={env.get(name, '')}" for name in SWITCHES] + \
           [ph.request(pairs=[c.shape], flags=vc.STORAGE_FLAG[c.storage] | (vc.LOCAL if c.local else 0), **DEVICE, **words)]


def planned(p, c):
    """The decisions of a plan that a case claims (the wide path has no team shape)."""
    assert p.rc == 0, (c.id, p.msg)
    out = dict(pack=p.pack, storage=p.storage)
    if not c.wide:
        out.update(tw=p.teams[0]["tw"], gw=p.teams[0]["gw"], slim=p.teams[0]["slim"])
    return out


def test_family_counts(variants):
    """The program sees the plan the issue counted, and every sweep the predicates admit is instantiated by a ladder."""
    count = collections.Counter(k[0] for k, ladder in variants.items() if ladder)
    print(dict(count))
    for family, want in FAMILY_COUNTS.items():
        assert count[family] == want
        assert all(ladder for k, ladder in variants.items() if k[0] == family)
    assert count["trace_affine"] >= 24 and count["trace_linear"] >= 18 and count["trace_fast"] >= 3


def test_case_ids_are_unique():
    ids = [c.id for c in vc.CASES]
    assert len(ids) == len(set(ids))


def test_cases_cover_exactly_the_instantiated_variants(variants):
    instantiated = {k for k, ladder in variants.items() if ladder}
    covered = set().union(*(vc.keys(c) for c in vc.CASES))
    missing = instantiated - covered - set(vc.UNREACHABLE)
    extra = covered - instantiated
    assert not missing, f"{len(missing)} instantiated variants without a case, e.g. {sorted(map(str, missing))[:8]}"
    assert not extra, f"cases claim variants that are not built: {sorted(map(str, extra))[:8]}"
    assert not set(vc.UNREACHABLE) - instantiated and not set(vc.UNREACHABLE) & covered


def test_every_case_plans_as_claimed(plan_exe):
    lines = [ln for c in vc.CASES for ln in plan_lines(c)]
    wrong = []
    for c, p in zip(vc.CASES, ph.plans(plan_exe, lines)):
        got, want = planned(p, c), c.plan()
        if got != {k: want[k] for k in got}:
            wrong.append((c.id, c.shape, got, want))
    assert not wrong, wrong[:10]


def test_the_planner_refuses_the_unreachable_variants(plan_exe):
    """An entry is a kernel that is compiled and never launched: the case that would force it plans something else."""
    for key, (reason, c) in vc.UNREACHABLE.items():
        assert key in vc.keys(c) and reason
        p, = ph.plans(plan_exe, plan_lines(c))
        got = planned(p, c)
        assert got != {k: c.plan()[k] for k in got}, (key, got)


def tie_inputs():
    """The distinct (inputs, parameters) of the tie-dense runs (global alignments: a local walk is not the oracle's trace)."""
    return sorted({(c.inputs(tie=True), vc.frozen(c.params(tie=True))) for c in vc.CASES if c.tie_dense() and not c.local})


def density_job(job):
    return job, vc.tie_density(*job)


def test_tie_dense_inputs_are_tie_dense():
    """shift_cost 0 at max_shift >= 1: at least 90 % of the columns of every tie-dense case's oracle trace have two or more
    candidates (the default protein costs give about 15 %)."""
    from free_ends_expected import pool_map
    done = pool_map(density_job, tie_inputs())
    for (inputs, params), d in done:
        print(f"tie density {inputs} s={dict(params)['max_shift']} beta={dict(params)['gap_opening_cost']}: {d:.3f}")
    low = [(job, d) for job, d in done if d < MIN_TIE_DENSITY]
    assert not low, low
    (shape, form, kind, _), params = done[0][0]     # (the walk can tell: the plain inputs under the default shift cost)
    assert vc.tie_density((shape, form, kind, False), vc.frozen(dict(dict(params), shift_cost=-150))) < 0.5
