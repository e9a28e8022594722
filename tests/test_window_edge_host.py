"""The cases of tests/window_edge.py are what they claim to be -- from the mirror and the CPU oracle alone, no GPU:
each sits at the last scale the int32 safety window admits, its finite values reach the magnitudes the module records,
its "-infinity" cells stay a class of their own, and scaling changed neither scores (beyond the factor) nor traces."""
import math

import numpy as np
import pytest

import window_edge as we
from window_edge import CASES, MEASURED, NEG, RAGGED, WINDOW

#: what the inputs must reach for the GPU tests to mean anything: finite magnitudes 10 - 100 x beyond the suite's
#: largest score elsewhere (761500 < 2^20); the two constant-table extremes realise more of the bound
FLOOR = {"const-positive": 1 << 26, "const-negative": 1 << 24}
SOLO = [name for name, p in CASES.items() if p not in RAGGED]
EXACT = [name for name in SOLO if CASES[name].form not in ("rna", "feature")]   # mu2 = int(sw * ...) does not scale exactly


def test_mirror_formula_and_edge_search():
    # PROTEIN_PARAMS with BLOSUM62 (|1100| at W/W), two 512-mers: colmax = 1100 + 800 + 2 (50 + 150) + 2 * 150
    assert we.window(512, 512, 1100, 800, -150, -50, -150) == (2600, 2056 * 2600)
    assert we.window(1, 1, 0, 0, 0, 0, 0) == (0, 0)
    for per_k in (1, 7, 76800, WINDOW - 1):
        k = we.edge_scale(lambda x: x * per_k)
        assert k * per_k < WINDOW <= (k + 1) * per_k
    with pytest.raises(AssertionError):
        we.edge_scale(lambda x: x * WINDOW)
    # bound^2 just below 2^56: 128 replicas and a few more; at the largest bound the window admits, 128 exactly
    assert we.sumsq_max_replicas(WINDOW - 1) == 128 and we.sumsq_max_replicas(WINDOW) == 127
    assert we.sumsq_max_replicas(WINDOW - 1) * (WINDOW - 1) ** 2 <= we.INT64_MAX < 129 * (WINDOW - 1) ** 2


def test_classes_split():
    lay = np.zeros((1, 2, 2, 1, 1), dtype=np.int64)
    lay[0, :, :, 0, 0] = [[5, -7], [NEG + 9, NEG - 4]]
    c = we.classes(lay, 1, 1, 0)
    assert sorted(c["finite"].tolist()) == [-7, 5] and sorted(c["inf"].tolist()) == [NEG - 4, NEG + 9]
    assert (c["magnitude"], c["drift"], c["between"]) == (7, 9, 0)
    lay[0, 0, 0, 0, 0] = -WINDOW
    lay[0, 0, 1, 0, 0] = NEG + WINDOW
    assert we.classes(lay, 1, 1, 0)["between"] == 2
    lay[0, 0, 0, 0, 0] = -WINDOW + 1
    lay[0, 0, 1, 0, 0] = NEG + WINDOW - 1
    assert we.classes(lay, 1, 1, 0)["between"] == 0


@pytest.mark.parametrize("name", SOLO)
def test_case_sits_at_the_edge_and_reaches_its_magnitude(name):
    p = CASES[name]
    k = p.k
    assert k >= 2 and p.product(k) < WINDOW <= p.product(k + 1)
    assert p.product(k) > WINDOW * 0.99        # (the scale is fine enough to come within a hundredth of the limit)
    ref = p.reference()
    c = ref["classes"]
    print(f"{name:34s} k={k:5d} finite=2^{math.log2(c['magnitude']):.2f} ({c['magnitude']}) drift={c['drift']} "
          f"({100 * c['drift'] / WINDOW:.2f} % of 2^28) score={ref['score']}")
    assert c["between"] == 0
    assert c["magnitude"] >= FLOOR.get(p.costs, 1 << 23)
    assert abs(ref["score"]) < p.product(k) and c["magnitude"] < p.product(k) and c["drift"] < p.product(k)
    assert (k, c["magnitude"], c["drift"]) == MEASURED[name]     # what the module records is what the oracle says
    # every table entry an int32, and the maxima of the mirror are the tables' own
    mu1, mu2 = p.tables(k)
    amax, bmax = p.maxima(k)
    assert int(np.abs(mu1).max()) <= amax < 2 ** 31 and int(np.abs(mu2).max()) <= bmax < 2 ** 31
    if p.form != "feature":                    # (FEATURE form: the bound is of the features' maxima, above every entry)
        assert int(np.abs(mu1).max()) == amax and int(np.abs(mu2).max()) == bmax


def test_measured_lists_every_case_and_no_other():
    assert set(MEASURED) == set(CASES)


@pytest.mark.parametrize("name", EXACT)
def test_scaling_is_exact_in_the_oracle(name):
    p = CASES[name]
    one, edge = p.reference(1), p.reference()
    assert edge["score"] == p.k * one["score"]
    assert edge["trace"] == one["trace"] and edge["complete"] == one["complete"]


def test_rna_and_feature_scale_by_their_actual_tables():
    """mu2 = int(sw * ...): not k times the table of scale 1 in general, so k comes from the table (or, FEATURE form,
    from the host's sqrt bound) at each scale."""
    rna = CASES["rna-55x50-s2-affine"]
    assert rna.maxima(rna.k)[1] == int(np.abs(rna.tables(rna.k)[1]).max()) == 400 * rna.k   # 0/1 features: exact after all
    for name in ("feature-61x50-s2-affine", "feature-40x45-s1-linear", "feature-24x27-s1-affine"):
        p = CASES[name]
        k = p.k
        fa, fb = p.features
        bound = abs(400.0 * k) * sum(math.sqrt(fa[x].max() * fb[x].max()) for x in range(3))
        assert p.maxima(k)[1] == math.ceil(bound) >= int(p.tables(k)[1].max())
        assert not np.array_equal(p.tables(k)[1], p.tables(1)[1] * k)                          # truncation after scaling
        assert np.abs(p.tables(k)[1] - p.tables(1)[1] * k).max() < k


def test_ragged_batch_is_scaled_by_its_longest_pair():
    k = we.batch_scale(RAGGED)
    longest = max(RAGGED, key=lambda p: p.n + p.m)
    assert (longest.n, longest.m) == (100, 100) and k == longest.k
    colmax = longest.window(k)[0]
    worst = 0
    for p in RAGGED:
        assert p.window(k)[0] == colmax and p.product(k) < WINDOW      # one column bound for the batch; all admitted
        c = p.reference(k)["classes"]
        assert c["between"] == 0
        assert (k, c["magnitude"], c["drift"]) == MEASURED[p.name]
        one = p.reference(1)
        assert p.reference(k)["score"] == k * one["score"] and p.reference(k)["trace"] == one["trace"]
        worst = max(worst, c["magnitude"])
    assert longest.product(k + 1) >= WINDOW and worst >= 1 << 23
