"""The wide-band affine sweep's ring inside the HBM budget: what the test_gpu_null*.py modules share to run a null batch at
max_shift > 5 under a budget that cuts its rings into chunks.  The ring (5 levels x 27 derived values per level point,
plan_host.ring_dwords) is all such a SCORE_ONLY batch keeps beside 64 bytes per pair, so it is what the budget is sized by."""
import numpy as np

from plan_host import ring_dwords


def ring_bytes(n, s):
    return 4 * ring_dwords(n, s)


def ring_budget(lens_a, s, rings=2):
    """Room for the rings of two pairs like the batch's largest, and 1 MiB for their layers and tables: a batch of more
    than two such pairs is cut, and every single pair fits."""
    return rings * max(ring_bytes(n, s) for n in lens_a) + (1 << 20)


def check_chunked_null(open_batch, zscores, lens_a, s, want, observed):
    """``open_batch(hbm_budget_bytes)`` -> a null batch, ``zscores(hbm_budget_bytes)`` -> the dict of significance.zscores*;
    ``lens_a``: the real pairs' len A; ``want``: [pair][replica] the oracle's scores on the mirror's shuffles.
    Under ring_budget the batch runs in several chunks, none of which asks for more than the budget, and gives the null
    scores of the unbudgeted batch and of the oracle, the same reductions against ``observed`` and the same z-scores."""
    budget = ring_budget(lens_a, s)
    got = []
    for bud in (0, budget):
        b = open_batch(bud)
        b.run()
        got.append((b.null_scores().copy(), dict(b.current_info()), b.null_stats(observed)))
        b.close()
    (base, info, stats), (chunked, info_c, stats_c) = got
    print("wide null batch: nchunks", info["nchunks"], "->", info_c["nchunks"], "under", budget, "bytes")
    assert info["nchunks"] == 1 and info_c["nchunks"] > 1
    assert info_c["hbm_layer_bytes"] <= info["hbm_layer_bytes"]   # (layers only: the ring is not part of this figure)
    np.testing.assert_array_equal(chunked, base)
    assert chunked.tolist() == [list(row) for row in want]
    assert set(stats) == set(stats_c)
    for k in stats:
        np.testing.assert_array_equal(stats_c[k], stats[k], err_msg=k)
    z, z_c = zscores(0), zscores(budget)
    assert set(z) == set(z_c)
    for k in z:
        np.testing.assert_array_equal(z_c[k], z[k], err_msg=k)
    return chunked
