"""Every route of the NIW sampling sweep (csrc/niw_sweep.hip) at the cluster counts where the code changes, outside the band D 33 .. 64
that tests/test_gpu_niw.py covers densely: niw_sweep_direct_kernel<1,4,4> (D <= 16: no screen; 39 table rows in LDS, the global scratch
beyond), <2,4,3> (D 17 .. 32: screen operands in LDS up to K = 25, table in LDS up to K = 52, then the generic instantiation with 26
compact slots), <4,4,2> at both sides of its switches (38 | 39, 79 | 80), and niw_sweep_kernel<8> / <16> (D >= 65) with one, two, three,
five and all 32 words of its survm / surv2 / present bitmaps and one, two, three and 16 candidate chunks.

Problems: tools/niw_routes.paired_problem -- two clusters per site, sites far apart, so that the one neighbour that survives every screen
lies ceil(K / 2) indices away: another word and another chunk from K = 65 on.  Method, after ONE running-chain sweep (previous labels set,
the bin-sorted visiting order of a statistics pass, screens and -- D >= 65 -- the bracket launch active):
  * the kernel's tables against Float64 (tools/niw_routes.table_f64, which tests/test_niw_routes_cpu.py pins to the oracle's
    niw_loglik_f64) at 1e-3 + 2e-5 |value|, cluster rows and sub-cluster rows (K > 512: in two halves on a second worker,
    as tests/test_gpu_mult_variants.sub_table does);
  * labels and sub-labels bit-exact with the oracle's draw from the kernel's own tables;
  * against the oracle's independent Float32 table every differing label sits on a CDF edge of the Float64 table (within 1e-3 of the
    row mass); the count is printed, no budget is fixed;
  * sweep(final=True): the argmax of the kernel's table;
  * the route, from dpmm_last_sweep_work: without a screen (D <= 16; D >= 65 not a multiple of 4, where the tail records the screens
    start from do not exist) full_evals is EXACTLY K per wave tile plus two per distinct new label; with screens it lies between the
    number of clusters tools/niw_routes.tile_sets proves evaluated and the number it cannot prove dropped (equal, on these problems:
    two per site the tile touches), far below K and above the floor of a tile without survivors; D >= 65 with screens: brackets > 0
    in bin-sorted order (also with the labels rotated by a site), 0 in storage order of shuffled points.  D 33 .. 64: the lean launch
    changes the tiles, so the bounds there are per tile of at most 64 positions (check_route).  With hopeless references ("shuffled",
    "wrong") the evaluated set is not determined by the geometry: only the draws and "no more than without screens" are asserted.
No counter tells the LDS table from the global scratch, or a draw from the compact copy from one from the scratch rows (`from_lds`): those
cases sit at tools/niw_routes.budgets' thresholds and one beside them ("mixed": tiles that evaluate 25 .. 64 clusters around the 26
slots, predicted on the CPU), and the draw's bit-exactness is what is asserted there."""
import functools
import time

import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_niw import assert_sublabels_bit_exact, gpu_worker
from tools import niw_routes as nr

pytestmark = pytest.mark.gpu

SEED, FIRST, EPOCH = 17, 999, 4
WORST = dict(table=0.0, flips=0, ratio_of_k=0.0)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.time()
    yield
    print(f"\n[test_gpu_niw_routes] wall time of the module's tests: {time.time() - t:.1f} s; worst table error {WORST['table']:.3f} of the bar, "
          f"most CDF-edge flips in a case {WORST['flips']}, largest full_evals / wave_tiles / K of a screened case {WORST['ratio_of_k']:.3f}")


@functools.lru_cache(maxsize=2)
def reference(D, K, variant):
    P = nr.case_problem(D, K, variant)
    P["t64"] = nr.table_f64(P)
    t2 = np.empty((2 * K, P["n"]))
    t2[0::2] = nr.table_f64(P, 1)
    t2[1::2] = nr.table_f64(P, 2)
    P["t2_64"] = t2
    P["oracle"] = orc.sweep_niw(P["X"], D, P["mu"], P["invS"], P["logdet"], np.log(P["w"]), np.log(P["lr"]), seed=SEED, epoch=EPOCH,
                                first_idx=FIRST, want_parr=True)
    return P


def assert_table(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / (1e-3 + 2e-5 * np.abs(want))).max())
    print(f"{what}: table error {worst:.3f} of the bar 1e-3 + 2e-5 |value| (max |value| {np.abs(want).max():.3g})")
    WORST["table"] = max(WORST["table"], worst)
    assert worst <= 1.0, (what, worst)


def sub_table(pkg, wk, P):
    """(2K, n): the kernel's own sub-cluster values.  dpmm_debug_subloglik refuses 2K > 1024: then the left and the right rows as the cluster
    rows of a K-cluster parameter set on a second worker, the lr weights as weights -- the same kernel in table mode, the same
    -logdet/2 + logf(weight) in Float32."""
    K = P["K"]
    if 2 * K <= 1024:
        return wk.debug_subloglik()
    tab2 = np.empty((2 * K, P["n"]), np.float32)
    for s in (0, 1):
        Q = dict(P)
        Q["mu"] = np.repeat(P["mu"][1 + s::3], 3, axis=0)
        Q["invS"] = np.repeat(P["invS"][1 + s::3], 3, axis=0)
        Q["logdet"] = np.repeat(P["logdet"][1 + s::3], 3)
        Q["w"] = np.ascontiguousarray(P["lr"][:, s])
        w2 = gpu_worker(pkg, Q, seed=SEED, first_index=FIRST)
        tab2[s::2] = w2.debug_loglik()
        w2.close()
    return tab2


def check_route(P, variant, order, prev0, lab0, work):
    D, K, n = P["D"], P["K"], P["n"]
    NB = nr.nb_of(D)
    big = NB >= 8
    tiles = -(-n // nr.tile_points(NB))
    wave_tiles = 4 * tiles if big else tiles
    group = 32 if big else 64                             # points of one wave: the sub-label phase evaluates per wave and distinct label
    sub_evals = 2 * nr.distinct_labels(order, lab0, group)
    full, ratio = work["full_evals"], work["full_evals"] / work["wave_tiles"]
    what = f"D={D} K={K} {variant}"
    print(f"{what}: full_evals / wave_tiles {ratio:.2f} (K = {K}), screens16 / wave_tiles {work['screens16'] / work['wave_tiles']:.2f}, "
          f"tail pairs / wave_tiles {work['tail_pairs'] / work['wave_tiles']:.2f}, brackets {work['brackets']:.0f}, b3 {work['b3_evals']:.0f}")
    assert work["launches"] == 1
    if NB != 4:
        assert work["wave_tiles"] == wave_tiles, (what, work["wave_tiles"], wave_tiles)
    if not nr.screened(D, K):
        assert full == wave_tiles * K + sub_evals, (what, full, wave_tiles * K, sub_evals)
        assert work["brackets"] == 0
        return
    if big:
        # ("wrong": the labels are rotated by whole sites, so cluster 0's leading block still fills whole tiles with one label)
        assert (work["brackets"] > 0) if variant != "shuffled" else (work["brackets"] == 0), (what, work["brackets"])
    if variant in ("shuffled", "wrong"):
        # hopeless references: which clusters of neighbouring sites pass the screens is not determined by the geometry (a tie between the
        # sites on either side); the draws above are what is asserted, and that the screens cost no more evaluations than no screen
        assert full <= wave_tiles * K + sub_evals, (what, full)
        return
    if variant != "mixed":
        WORST["ratio_of_k"] = max(WORST["ratio_of_k"], ratio / K)
    if NB == 4:
        # The lean launch walks tiles aligned to the sort's bins (more, partly filled ones) and draws sub-labels from the bf16 planes
        # (b3_evals), so tile_sets' 64-aligned tiles do not apply.  From the geometry all the same: a tile -- at most 64 consecutive
        # positions -- touches at most s sites, evaluates at most their 2 s clusters and draws at most 2 s distinct labels, two
        # sub-cluster evaluations each: 6 s per tile.  And the partner survives every screen, so no tile is settled without an
        # evaluation: reference + partner + one label's two sub-clusters = 4 per tile, except in the tiles of the one cluster without a
        # partner (K odd; its points fill at most cnt / 64 + 4 tiles of either kind), where two sub-cluster evaluations remain.
        s_max = nr.max_sites_per_window(P, order, prev0)
        total = work["full_evals"] + work["b3_evals"]
        lone = (int((P["z"] == P["S"] - 1).sum()) // 64 + 4) if K % 2 else 0
        wt = work["wave_tiles"]
        print(f"{what}: full + b3 evaluations {total:.0f} in {wt:.0f} tiles; geometry: at least {4 * wt - 2 * lone:.0f}, at most {6 * s_max * wt:.0f} (sites per tile <= {s_max})")
        assert 6 * s_max < K
        assert 4 * wt - 2 * lone <= total <= 6 * s_max * wt, (what, total, wt, s_max)
        return
    U = nr.table_f64(P, screen_rows_from=16 * nr.screen_block(D))
    sets = nr.tile_sets(P, P["t64"], U, order, prev0, extra_refs=0 if big else 2)
    per = 4 if big else 1                                 # D >= 65: a cluster's evaluation is counted by each of the tile's four waves
    lo = per * sum(len(sure) if len(may) > 1 else 0 for _, sure, may in sets) + sub_evals
    hi = per * sum(len(may) for _, _, may in sets) + sub_evals
    floor = 3 * wave_tiles                                # no survivor anywhere: the reference + two sub-cluster evaluations per wave tile
    print(f"{what}: full_evals {full:.0f}, proved between {lo} and {hi}; floor {floor}, unscreened {wave_tiles * K + sub_evals}")
    assert floor < lo <= hi, (what, floor, lo, hi)        # (geometry: the partner survives in every tile -- its word is the far one)
    if variant != "mixed":
        assert hi < 0.6 * K * wave_tiles, (what, hi)
    assert lo <= full <= hi, (what, lo, full, hi)


@pytest.mark.parametrize("D,K,variant", nr.all_cases())
def test_route(pkg, D, K, variant):
    P = reference(D, K, variant)
    n = P["n"]
    what = f"D={D} K={K} {variant}"
    prev0 = nr.rotated_labels(P) if variant == "wrong" else P["z"]
    sub0 = 1 + (np.arange(n) & 1)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, first_index=FIRST, device=0, seed=SEED)
    wk.upload_points(P["X"])
    wk.set_labels(prev0 + 1, sub0)
    wk.set_num_clusters(K)
    if K == 1024:
        with pytest.raises(pkg.DpmmError):
            wk.set_num_clusters(K + 1)
    ordered = variant not in ("shuffled", "mixed")
    if ordered:
        wk.suffstats_packed()                             # leaves the bin-sorted visiting order of these labels
    order = nr.visiting_order(prev0, sub0) if ordered else np.arange(n)
    wk.set_params_niw(P["mu"], P["invS"], P["logdet"], P["lr"], P["w"])
    wk.last_sweep_work()
    wk.sweep(EPOCH)
    work = wk.last_sweep_work()
    lab, sub = wk.get_labels()
    assert lab.min() >= 1 and lab.max() <= K and set(np.unique(sub)) <= {1, 2}
    # the tables
    tab = wk.debug_loglik()
    assert_table(tab, P["t64"], f"{what} cluster rows")
    tab2 = sub_table(pkg, wk, P)
    assert_table(tab2, P["t2_64"], f"{what} sub-cluster rows")
    # the draws, from the kernel's own tables
    u0, u1 = orc.uniforms(SEED, EPOCH, 0, FIRST, n)
    want = orc.sample_log_cat(tab, u0)
    bad = np.flatnonzero(want != lab)
    assert len(bad) == 0, (what, len(bad), bad[:8], lab[bad[:8]], want[bad[:8]], prev0[bad[:8]] + 1)
    if 2 * K <= 1024:
        assert_sublabels_bit_exact(wk, lab, sub, u1)
    else:
        i = np.arange(n)
        assert np.array_equal(orc.sample_log_cat(np.stack([tab2[2 * (lab - 1), i], tab2[2 * (lab - 1) + 1, i]]), u1), sub), what
    # the oracle's independent Float32 table: every differing label on a CDF edge of the Float64 table
    olab, osub, _ = P["oracle"]
    flips = np.flatnonzero(lab != olab)
    p = np.exp(P["t64"] - P["t64"].max(0))
    cdf = np.cumsum(p, 0) / p.sum(0)
    same = lab == olab
    print(f"{what}: label flips vs oracle {len(flips)} of {n}, sub-label flips {int((sub[same] != osub[same]).sum())}; "
          f"labels equal to the generating cluster {(lab == P['z'] + 1).mean():.2f}")
    WORST["flips"] = max(WORST["flips"], len(flips))
    for i in flips:
        assert np.min(np.abs(cdf[:, i] - u0[i])) < 1e-3, (what, int(i), float(u0[i]))
    assert (P["site"][lab - 1] == P["site"][P["z"]]).all(), what       # no visible mass at another site: the draw cannot leave the point's own
    check_route(P, variant, order, prev0, lab - 1, work)
    wk.sweep(EPOCH + 1, final=True)
    assert np.array_equal(wk.get_labels()[0], orc.argmax_rows(tab)), what
    wk.close()
