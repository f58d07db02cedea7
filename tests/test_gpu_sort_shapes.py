"""The counting sort of the per-step statistics pass (hist_kernel, reset_recount_kernel, scan, scatter_kernel<TILE, STEP>) at the
smallest shapes that can break its vectorised tiles, against numpy: `perm` is the STABLE argsort of the points by bin = 2 (label - 1) +
(sub - 1) -- ascending point index inside a bin, the invariant every later kernel rests on --, the bin totals and starts are its counts and
their exclusive prefix, the bad-cluster flags are "a sub-cluster is empty", and the labels after the pass are the oracle's reset_sub of the
flagged clusters (the same Philox draw keyed by the global point index).  Everything is integer: equality, no tolerance.

Shapes: n in {1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4 * 2048 + 17} (a shard below one tile, a partial last vector, a partial last
tile, several tiles), both tile sizes (DPMM_OPT_SORT_TILE), K = 1, 2, 32, 64, 256 with empty clusters, one / several / all K clusters
one-sided, labels contiguous by cluster, in short runs and shuffled, a point whose label left for an out-of-range bin (the `dirty` rule: its
old cluster's cached row is stale), and every case a second pass later, so that prev_lab is read."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4 * 2048 + 17]
D, SEED, FIRST = 4, 77, 12345


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def _labels(rng, n, K, order, onesided):
    """Labels 1..K (the last cluster of K > 4 left empty) and sub-labels 1..2; the clusters in `onesided` get one sub-label only."""
    top = K - 1 if K > 4 else K
    if order == "sorted":
        lab = np.sort(rng.integers(1, top + 1, n))
    elif order == "runs":                                   # runs of 100 points, the clusters in turn
        lab = (np.arange(n) // 100) % top + 1
    else:
        lab = rng.integers(1, top + 1, n)
    sub = rng.integers(1, 3, n)
    for j, k in enumerate(onesided):
        sub[lab == k] = 1 + j % 2
    return lab.astype(np.int64), sub.astype(np.int64)


def _expect(lab, sub, K, epoch):
    """Host restatement of one pass: flags, the reset, then the stable sort of the in-range points."""
    inr = (lab >= 1) & (lab <= K)
    cnt = np.zeros((K, 2), np.int64)
    np.add.at(cnt, (lab[inr] - 1, sub[inr] - 1), 1)
    bad = ((cnt[:, 0] == 0) | (cnt[:, 1] == 0)).astype(np.uint8)
    sub = sub.copy()
    if bad.any():
        orc.reset_sub(lab, sub, np.flatnonzero(bad) + 1, SEED, epoch, FIRST)
    bins = 2 * (lab - 1) + (sub - 1)
    idx = np.flatnonzero(inr)
    perm = idx[np.argsort(bins[idx], kind="stable")].astype(np.int32)
    tot = np.bincount(bins[idx], minlength=2 * K).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(tot)]).astype(np.int32)
    return bad, sub, perm, tot, start


def _pass(wk, lab, sub, K, epoch, tag):
    bad, esub, perm, tot, start = _expect(lab, sub, K, epoch)
    packed, gbad = wk.step_stats(reset_epoch=epoch)
    gperm, gtot, gstart = wk.debug_sort_tables()
    glab, gsub = wk.get_labels()
    assert np.array_equal(gbad, bad), tag
    assert np.array_equal(glab, lab) and np.array_equal(gsub, esub), tag
    assert np.array_equal(gtot, tot) and np.array_equal(gstart, start), tag
    assert np.array_equal(gperm, perm), tag
    assert np.array_equal(packed[:, 0], tot.astype(np.float64)), tag
    # the rows (derived halves included: a stale cache -- the `dirty` rule -- shows here) against the library's from-scratch pass, whose
    # own sort (no prev_lab, scatter_kernel<TILE, false>) must give the same order
    full = wk.suffstats_packed(None)
    np.testing.assert_allclose(packed, full, rtol=1e-12, atol=1e-9, err_msg=tag)
    fperm, ftot, _ = wk.debug_sort_tables()
    assert np.array_equal(fperm, perm) and np.array_equal(ftot, tot), tag
    return esub


@pytest.mark.parametrize("tile", [512, 2048])
@pytest.mark.parametrize("n", SIZES)
def test_sort_is_the_stable_argsort(pkg, n, tile):
    from dpmmsubclusters_jl_amd import binding
    rng = np.random.default_rng(1000 * n + tile)
    X = rng.normal(size=(n, D)).astype(np.float32)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=FIRST, device=0, seed=SEED)
    wk.upload_points(X)
    wk.set_option(binding.OPT_SORT_TILE, tile)
    epoch = 10
    for K, nside in [(1, 1), (2, 1), (32, 3), (64, 64), (256, 5)]:          # one, several and all K clusters one-sided
        wk.set_num_clusters(K)
        for order in ("sorted", "runs", "shuffled"):
            tag = f"n={n} tile={tile} K={K} {order}"
            onesided = list(range(1, K + 1)) if nside >= K else list(rng.choice(np.arange(1, K + 1), nside, replace=False))
            lab, sub = _labels(rng, n, K, order, onesided)
            wk.set_labels(lab, sub)
            sub = _pass(wk, lab, sub, K, epoch, tag + " first pass")
            # a second pass: nothing moved except a few points that change cluster, one of them to an out-of-range bin (label K + 1),
            # and a sub-label flip -- prev_lab decides which cached rows survive
            lab2, sub2 = lab.copy(), sub.copy()
            moved = rng.choice(n, min(n, 5), replace=False)
            lab2[moved] = rng.integers(1, K + 1, len(moved))
            lab2[moved[0]] = K + 1
            sub2[moved[-1]] = 3 - sub2[moved[-1]]
            wk.set_labels(lab2, sub2)
            sub2 = _pass(wk, lab2, sub2, K, epoch + 1, tag + " second pass")
            # ... and the point comes back from the out-of-range bin
            lab3 = lab2.copy(); lab3[moved[0]] = lab[moved[0]]
            wk.set_labels(lab3, sub2)
            _pass(wk, lab3, sub2, K, epoch + 2, tag + " third pass")
            epoch += 3
    wk.close()
