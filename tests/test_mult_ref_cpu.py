"""tests/tools/mult_ref.py without a GPU: the instantiation arithmetic it restates gives the ranges the launchers document, the route
prediction does what its docstring says on a hand-made tile, and the CDF-edge bound holds for tables that differ within the tolerance."""
import numpy as np

from oracle import oracle as orc
from tools import mult_ref as mr


def test_instantiations_by_cluster_count():
    u8 = {K: mr.u8_instantiation(K) for K in range(1, 1025)}
    assert all(u8[K] == (2 if K <= 16 else 4 if K <= 48 else 6 if K <= 80 else 8) for K in u8)
    assert all(mr.u8_lds_table(K) == (K <= 152) for K in u8)
    assert [mr.u8_instantiation(K, table_mode=True) for K in (5, 6, 10, 11, 16, 17, 81, 1024)] == [2, 2, 4, 4, 4, 6, 8, 8]
    bf = {K: mr.bf16_instantiation(K) for K in range(1, 1025)}
    assert all(bf[K][0] == (2 if K <= 10 else 4 if K <= 21 else 6 if K <= 32 else 8) for K in bf)
    assert all((len(bf[K][2]) > 1) == (K >= 43) for K in bf)
    assert bf[100][1:] == (19, [8, 8, 3]) and bf[1024][1] == 192 and sum(bf[1024][2]) == 192
    assert mr.u8_blocks(1024) == (64, 128) and mr.u8_blocks(5) == (1, 0) and mr.u8_blocks(6) == (1, 1)


def test_routes_of_hand_made_tiles():
    K, n = 300, 600                                      # NRBc = 19, NRBs = 38, <8>, no LDS table; three tiles: 256, 256, 88 points
    prev = np.ones(n, np.int64); sub = np.ones(n, np.int64); new = np.ones(n, np.int64)
    prev[256:512] = 1 + 8 * (np.arange(256) % 38)        # tile 1 asks for every sub-cluster block
    new[0] = 300                                         # tile 0: a new label in block 37 (word 1) that nobody asked for
    r = mr.u8_routes(K, prev, sub, new, ordered=False)
    assert (r["B"], r["tiles"], r["single"], r["multi"], r["lds"], r["miss"]) == (8, 3, 0, 3, 0, 1)
    assert r["max_cnt"] == 19 + 38 and r["need_words"] == {0, 1} and r["miss_words"] == {1} and r["max_miss"] == 1
    # bin-sorted: the 344 + 7 points of cluster 1 lead, the others follow by cluster; a right sub-label sorts behind the left ones
    sub[0] = 2
    order = mr.visiting_order(prev, sub, ordered=True)
    ones = np.flatnonzero(prev == 1)
    assert order[len(ones) - 1] == 0 and np.array_equal(np.sort(order[:len(ones)]), ones) and np.all(np.diff(prev[order]) >= 0)
    # K = 40 (<4>, NRBc = 3): a tile inside one block of eight clusters takes one pass and draws from the LDS table
    r = mr.u8_routes(40, 1 + np.arange(256) % 8, np.ones(256, np.int64), 1 + np.arange(256) % 8, ordered=False)
    assert (r["B"], r["single"], r["lds"], r["multi"], r["miss"]) == (4, 1, 1, 0, 0)


def test_labels_of_two_tables_within_the_tolerance_differ_on_cdf_edges_only():
    rng = np.random.default_rng(3)
    K, n = 300, 20000
    t64 = rng.normal(-800.0, 3.0, (K, n))
    delta = mr.TABLE_ATOL + mr.TABLE_RTOL * np.abs(t64)
    a = (t64 + delta * rng.uniform(-0.9, 0.9, t64.shape)).astype(np.float32)      # (the Float32 rounding of the entries: 3e-5, inside the rest)
    b = (t64 + delta * rng.uniform(-0.9, 0.9, t64.shape)).astype(np.float32)
    u = orc.uniforms(5, 1, 0, 0, n)[0]
    la, lb = orc.sample_log_cat(a, u), orc.sample_log_cat(b, u)
    dist, bound = mr.cdf_edge(t64, u)
    flips = la != lb
    assert flips.sum() > 20 and np.all(dist[flips] <= bound[flips])
    assert (dist <= bound).mean() < 0.6                  # (the bound is not vacuous here: 0.49)
    t, t2 = mr.table_f64(np.array([[1.0, 2.0]], np.float32), np.log(np.array([[0.5, 0.5], [0.25, 0.75], [0.75, 0.25]], np.float32)),
                         np.array([1.0], np.float32), np.array([[0.5, 0.5]], np.float32))
    assert np.allclose(t, 3 * np.log(0.5)) and np.allclose(t2[:, 0], [np.log(0.25) + 2 * np.log(0.75) + np.log(0.5), np.log(0.75) + 2 * np.log(0.25) + np.log(0.5)])
