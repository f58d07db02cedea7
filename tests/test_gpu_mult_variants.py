"""Every instantiation and route of the dense Multinomial sweep kernels (csrc/mult_sweep.hip) and the dense statistics kernels, up to
DPMM_MAX_CLUSTERS = 1024 clusters.  The launchers pick code by K: tests/test_gpu_mult.py stops at K = 70.

Method (that of tests/test_gpu_mult.py, at the K where the code changes): the kernel's table against numpy Float64 at rtol 1e-5 / atol 1e-3
(a contraction over D terms: the tolerance does not depend on K); labels and sub-labels bit-exact from the kernel's own tables with the
oracle's draw; against the oracle's independent Float32 table every differing label must sit on a CDF edge of the Float64 table
(tools/mult_ref.cdf_edge; the number of such points is printed, no budget is fixed).  tools/mult_ref.u8_routes predicts on the host which
route every tile of a running-chain sweep takes, so that a case cannot quietly miss the branch it was written for.

debug_subloglik evaluates the 2K sub-cluster rows as the cluster rows of a temporary 2K-cluster parameter set and refuses 2K > 1024.  For
K > 512 `sub_table` does the same thing in two halves on a second worker (left rows, then right rows, as the cluster rows of a K-cluster
set with the lr weights as weights): the same kernel in table mode, the same Float32 logf of the same weights -- the same values."""
import functools
import time

import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_mult import make_problem
from tools import mult_ref as mr

pytestmark = pytest.mark.gpu

N = 3000                         # 11 full tiles of 256 + one of 184
SEED, FIRST = 17, 999


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.time()
    yield
    print(f"\n[test_gpu_mult_variants] wall time of the module's tests: {time.time() - t:.1f} s")


# --------------------------------------------------------------------------- problems and references, computed once per (kind, K, D)
@functools.lru_cache(maxsize=3)                      # (a K = 1024 entry holds 74 MB of Float64 tables: consecutive cases share, old ones go)
def reference(kind, K, D, n=N):
    """kind: "bytes" (counts in 0..255, 255 present), "bf16" (the same with one 256.0: bf16-exact, not a byte), "f32" (0.3 added)."""
    P = make_problem(D, n, K, 60, seed=11 * K + D)
    P["X"][::7, 0] = 255.0
    if D == 1:
        # one feature: make_problem's rows are the one-point simplex (logp = 0, x = trials) and the contraction would vanish.  The
        # sweep takes any rows (set_params_mult does not normalise): one log-probability per row in (-3, -0.1), sub-cluster rows
        # beside their cluster's, and a count per point -- mostly 0..3, so that the draw spreads over the clusters, some anywhere
        # in 0..255.  table[k][i] = x_i logp_k + log w_k depends on the byte read AND on the row's fragment.
        rng = np.random.default_rng(7 * K + 1)
        a = rng.uniform(-3.0, -0.1, K)
        P["logp"] = np.stack([a, a * rng.uniform(0.8, 1.2, K), a * rng.uniform(0.8, 1.2, K)], 1).reshape(3 * K, 1).astype(np.float32)
        x = rng.integers(0, 4, n)
        x[::13] = rng.integers(0, 256, len(x[::13]))
        x[::50] = 255
        P["X"] = x.astype(np.float32).reshape(n, 1)
    if kind == "bf16":
        P["X"][5, D // 2] = 256.0
    elif kind == "f32":
        P["X"] = (P["X"] + np.float32(0.3)).astype(np.float32)
    P["t64"], P["t2_64"] = mr.table_f64(P["X"], P["logp"], P["w"], P["lr"])
    if D == 1:
        P["z"] = P["t64"].argmax(0)                  # (the "right" cluster of a point: its most probable one)
    P["oracle"] = {}
    return P


def oracle_sweep(P, epoch):
    if epoch not in P["oracle"]:
        P["oracle"][epoch] = orc.sweep_mult(P["X"], P["D"], P["logp"], np.log(P["w"]), np.log(P["lr"]), SEED, epoch, FIRST, want_parr=True)
    return P["oracle"][epoch]


def make_worker(pkg, P, no_u8=0, labels=None):
    from dpmmsubclusters_jl_amd import binding
    wk = pkg.Worker(pkg.PRIOR_MULT, P["D"], P["n"], first_index=FIRST, device=0, seed=SEED)
    wk.set_option(binding.OPT_MULT_NO_U8, no_u8)
    wk.upload_points(P["X"])
    if labels is not None:
        wk.set_labels(*labels)
        wk.set_num_clusters(P["K"])
    return wk


def sub_table(pkg, wk, P, no_u8=0):
    """(2K, n): the kernel's own sub-cluster values (module docstring)."""
    K = P["K"]
    if 2 * K <= 1024:
        return wk.debug_subloglik()
    tab2 = np.empty((2 * K, P["n"]), np.float32)
    w2 = make_worker(pkg, P, no_u8)
    for s in (0, 1):
        rows = np.zeros_like(P["logp"])
        rows[0::3] = P["logp"][1 + s::3]
        w2.set_params_mult(rows, np.full((K, 2), 0.5, np.float32), np.ascontiguousarray(P["lr"][:, s]))
        tab2[s::2] = w2.debug_loglik()
    w2.close()
    return tab2


def check_tables(pkg, wk, P, what, no_u8=0):
    tab = wk.debug_loglik()
    tab2 = sub_table(pkg, wk, P, no_u8)
    mr.assert_table(tab, P["t64"], f"{what} cluster rows")
    mr.assert_table(tab2, P["t2_64"], f"{what} sub-cluster rows")
    return tab, tab2


def check_draws(tab, tab2, lab, sub, epoch, what):
    u0, u1 = orc.uniforms(SEED, epoch, 0, FIRST, len(lab))
    assert np.array_equal(orc.sample_log_cat(tab, u0), lab), what              # draw arithmetic: bit-exact from the kernel's own table
    assert np.array_equal(orc.sample_log_cat(mr.sub_pair(tab2, lab), u1), sub), what
    return u0


def check_oracle(P, lab, sub, u0, epoch, what):
    """Labels against the oracle's own Float32 table: every differing point sits on a CDF edge of the Float64 table."""
    olab, osub, otab = oracle_sweep(P, epoch)
    flips = np.flatnonzero(lab != olab)
    dist, bound = mr.cdf_edge(P["t64"], u0)
    same = lab == olab
    otol = (np.abs(otab.astype(np.float64) - P["t64"]) / (mr.TABLE_ATOL + mr.TABLE_RTOL * np.abs(P["t64"]))).max()
    print(f"{what}: label flips vs oracle {len(flips)} of {len(lab)}, sub-label flips {int((sub[same] != osub[same]).sum())}; "
          f"points within the edge bound {int((dist <= bound).sum())}; oracle table at {otol:.2f} of the tolerance")
    assert otol <= 1.0, (what, otol)                 # the premise of the edge bound: BOTH tables are within the tolerance of Float64
    for i in flips:
        assert dist[i] <= bound[i], (what, int(i), float(dist[i]), float(bound[i]), int(lab[i]), int(olab[i]))
    return len(flips)


# --------------------------------------------------------------------------- 1. byte kernel, running chain
def start_labels(P, mode):
    """Previous labels of the first sweep.  "chain": the generating cluster for ~70 % of the points; the points of the first storage tile
    all in clusters 1..8 (one sub-cluster block: the tile's new labels -- clusters of every range -- are misses, in storage order and,
    these points leading the sorted order, in bin-sorted order); the other wrong ones uniform over 1..K, the first cluster of every set
    word (257, 513, 769) and cluster K among them, and one point generated by each of these starts in cluster 1.  "uniform": uniform everywhere, and the second storage tile holds a label of every
    sub-cluster block: its block list is full (NRBc + NRBs entries; 64 + 128 at K = 1024)."""
    K, n = P["K"], P["n"]
    rng = np.random.default_rng(K)
    sub0 = rng.integers(1, 3, n)
    if mode == "uniform":
        prev = rng.integers(1, K + 1, n)
        nrbs = max(mr.u8_blocks(K)[1], 1)
        prev[256:512] = 1 + np.minimum(8 * (np.arange(256) % nrbs) + rng.integers(0, 8, 256), K - 1)
        return prev, sub0
    prev = (P["z"] + 1).astype(np.int64)
    wrong = rng.random(n) < 0.25
    prev[wrong] = rng.integers(1, K + 1, wrong.sum())
    prev[:256] = rng.integers(1, min(K, 8) + 1, 256)
    tops = [k for k in (257, 513, 769, K) if k <= K]
    prev[300:300 + len(tops)] = tops
    for k in tops:                                     # ... and as NEW labels where the tile did not ask for them: one point of each starts in cluster 1
        pts = np.flatnonzero(P["z"][304:] + 1 == k)
        if len(pts):
            prev[304 + pts[0]] = 1
    return prev, sub0


def required_routes(K, mode, ordered):
    """What a case must reach, derived from the launch code and checked against the host-side prediction of tools/mult_ref (a prediction
    from the same code, not something the kernel reports: it rests on use_prev = 1 after set_labels, on the visiting order being on by
    default, and on the device's bin sort being stable).  In a running chain with 113 <= K <= 152, NRBc + 1 > 8: no first call fits one
    pass, so the LDS table of <8> is drawn from at K <= 112 only, although it is allocated up to K = 152."""
    nrbc, nrbs = mr.u8_blocks(K)
    B = mr.u8_instantiation(K)
    if nrbc + nrbs <= B:                               # K = 5, 6: every block in one pass whatever the labels are
        return {"single", "lds"}
    if mode == "uniform":
        return {"multi", "full_list"}
    req = {"miss"}
    if nrbc + 1 <= B:                                  # (K <= 112) a tile inside one block of eight clusters: one pass, table in LDS
        req |= {"single", "lds"}
    if not ordered or nrbc + 1 > B:
        req.add("multi")
    if K >= 257:
        req.add("words")
    return req


BYTE_CASES = [(5, 130), (6, 1), (6, 130), (16, 128), (17, 130), (33, 128), (48, 1), (48, 128), (49, 130), (80, 128), (81, 1), (81, 128), (152, 130),
              (153, 128), (256, 130), (257, 1), (257, 130), (513, 130), (769, 128), (1024, 130), (1024, 1)]
BYTE_RUNS = [(K, D, "chain", o) for K, D in BYTE_CASES for o in (False, True)] + [(81, 128, "uniform", False), (153, 128, "uniform", False), (1024, 130, "uniform", False)]


@pytest.mark.parametrize("K,D,mode,ordered", BYTE_RUNS)
def test_byte_kernel_running_chain(pkg, K, D, mode, ordered):
    """mult_sweep_u8_kernel<2 / 4 / 6 / 8> drawing labels: cluster values from the LDS table (K <= 152, first call in one pass) or from the
    global scratch (K >= 153, or a first call of several passes), first calls of one and of several passes, second calls for missed
    blocks, every word of the need / miss sets (K >= 257), a full block list (uniform previous labels).  Two sweeps, the second from the
    first one's labels, in storage order and in the bin-sorted order a statistics pass leaves."""
    P = reference("bytes", K, D)
    what = f"u8<{mr.u8_instantiation(K)}> K={K} D={D} {mode} {'sorted' if ordered else 'storage'}"
    before = start_labels(P, mode)
    wk = make_worker(pkg, P, labels=before)
    if ordered:
        wk.suffstats_packed()                          # leaves the bin-sorted order of these labels
    wk.set_params_mult(P["logp"], P["lr"], P["w"])
    tab, tab2 = check_tables(pkg, wk, P, what)
    seen = dict(single=0, multi=0, miss=0, lds=0, need_words=set(), miss_words=set(), max_cnt=0)
    for epoch in (1, 2):
        wk.sweep(epoch)
        lab, sub = wk.get_labels()
        u0 = check_draws(tab, tab2, lab, sub, epoch, (what, epoch))
        r = mr.u8_routes(K, before[0], before[1], lab, ordered)
        print(f"{what} sweep {epoch}: {mr.describe(r)}")
        if mode == "uniform" and epoch == 1:
            assert r["multi"] == r["tiles"], (what, r)           # every tile needs more blocks than the instantiation holds
        for key in ("single", "multi", "miss", "lds"):
            seen[key] += r[key]
        seen["need_words"] |= r["need_words"]; seen["miss_words"] |= r["miss_words"]; seen["max_cnt"] = max(seen["max_cnt"], r["max_cnt"])
        check_oracle(P, lab, sub, u0, epoch, f"{what} sweep {epoch}")
        before = (lab, sub)
        if ordered:
            wk.suffstats_packed()
            wk.set_params_mult(P["logp"], P["lr"], P["w"])
    wk.close()
    for key in required_routes(K, mode, ordered):
        if key == "words":
            words = set(range(((K - 1) >> 8) + 1))
            assert seen["need_words"] == words and seen["miss_words"] == words, (what, seen)
        elif key == "full_list":
            assert seen["max_cnt"] == sum(mr.u8_blocks(K)), (what, seen)
        else:
            assert seen[key] > 0, (what, key, seen)


# --------------------------------------------------------------------------- 2. byte kernel, final=True and predict
@pytest.mark.parametrize("K,D", [(33, 128), (81, 128), (153, 130), (1024, 130)])
def test_byte_kernel_final_argmax(pkg, K, D):
    """sweep(final=True): the argmax loop over the tile's LDS table (K = 33 in <4>, K = 81 in <8>: a converged chain in bin-sorted order,
    tiles inside one or two blocks of eight clusters) and over the global scratch (K = 153, 1024)."""
    P = reference("bytes", K, D)
    prev = ((P["z"] + 1).astype(np.int64), 1 + (np.arange(P["n"]) & 1))
    wk = make_worker(pkg, P, labels=prev)
    wk.suffstats_packed()
    wk.set_params_mult(P["logp"], P["lr"], P["w"])
    tab = wk.debug_loglik()
    mr.assert_table(tab, P["t64"], f"u8 final K={K}")
    wk.sweep(3, final=True)
    lab, _ = wk.get_labels()
    r = mr.u8_routes(K, prev[0], prev[1], lab, True)
    print(f"u8 final K={K}: {mr.describe(r)}")
    assert np.array_equal(lab, orc.argmax_rows(tab))
    assert (r["lds"] > 0) if K <= 81 else (r["lds"] == 0 and r["multi"] == r["tiles"])
    wk.close()


@pytest.mark.parametrize("K,D", [(81, 128), (1024, 130)])
def test_byte_kernel_predict_table(pkg, K, D):
    """predict: the table-mode launch (B from NRBc + NRBs: <8>, every block, ceil((NRBc + NRBs) / 8) passes)."""
    P = reference("bytes", K, D)
    assert mr.u8_instantiation(K, table_mode=True) == 8
    wk = make_worker(pkg, P)
    got = wk.predict_table_mult(np.ascontiguousarray(P["logp"][0::3]), P["w"])
    mr.assert_table(got, P["t64"], f"u8 predict K={K}")
    wk.close()


# --------------------------------------------------------------------------- 3. bf16 kernel
# (K, D, natural): natural = the data holds a 256.0 and reaches the kernel by itself; otherwise byte data under DPMM_OPT_MULT_NO_U8.
# D = 20 (ldx = 20, one k-step) is where the second half of a lane's eight features falls off the row (the `e + 4 < ldx` clamp); rows of
# D >= 32 are padded to a multiple of 32 features and never clamp.
BF16_CASES = [(10, 100, False), (11, 37, False), (11, 20, False), (21, 100, False), (22, 37, True), (33, 100, False), (42, 37, False), (43, 100, False),
              (100, 37, False), (100, 100, False), (1024, 100, False)]


@pytest.mark.parametrize("K,D,natural", BF16_CASES)
def test_bf16_kernel(pkg, K, D, natural):
    """mult_sweep_bf16_kernel<2 / 4 / 6 / 8>, one pass and several (K >= 43), a partial last pass (K = 100: 8 + 8 + 3 row blocks)."""
    P = reference("bf16" if natural else "bytes", K, D)
    B, nrb, passes = mr.bf16_instantiation(K)
    what = f"bf16<{B}> K={K} D={D} NRB={nrb} passes={passes if len(passes) <= 4 else str(len(passes)) + ' x 8'}{' (natural)' if natural else ''}"
    assert B == {10: 2, 11: 4, 21: 4, 22: 6, 33: 8, 42: 8, 43: 8, 100: 8, 1024: 8}[K] and (len(passes) > 1) == (K >= 43)
    no_u8 = 0 if natural else 1
    wk = make_worker(pkg, P, no_u8)
    wk.set_params_mult(P["logp"], P["lr"], P["w"])
    tab, tab2 = check_tables(pkg, wk, P, what, no_u8)
    epoch = 1
    wk.sweep(epoch)
    lab, sub = wk.get_labels()
    u0 = check_draws(tab, tab2, lab, sub, epoch, what)
    check_oracle(P, lab, sub, u0, epoch, what)
    if natural:
        # which kernel the upload chose cannot be asked; it can be told from the bits: the table is the one of the bf16 kernel on the
        # same data with the byte path switched off, and not the one of the Float32 kernel, which adds the features in another order
        from dpmmsubclusters_jl_amd import binding
        other = {}
        for opt in (binding.OPT_MULT_NO_U8, binding.OPT_MULT_FORCE_F32):
            w2 = pkg.Worker(pkg.PRIOR_MULT, D, P["n"], first_index=FIRST, device=0, seed=SEED)
            w2.set_option(opt, 1)
            w2.upload_points(P["X"])
            w2.set_params_mult(P["logp"], P["lr"], P["w"])
            other[opt] = w2.debug_loglik()
            w2.close()
        mr.assert_table(other[binding.OPT_MULT_FORCE_F32], P["t64"], f"{what}: the Float32 kernel on the same data")
        print(f"{what}: entries that differ from the Float32 kernel's table {int((other[binding.OPT_MULT_FORCE_F32] != tab).sum())} of {tab.size}")
        assert np.array_equal(other[binding.OPT_MULT_NO_U8], tab)
        assert not np.array_equal(other[binding.OPT_MULT_FORCE_F32], tab)
    if K in (43, 1024):
        wk.sweep(epoch + 1, final=True)
        assert np.array_equal(wk.get_labels()[0], orc.argmax_rows(tab))
    if K in (33, 100):
        # the same problem through the byte path: tables to summation-order rounding, statistics of one labelling bit-identical
        fixed = ((P["z"] + 1).astype(np.int64), 1 + (np.arange(P["n"]) & 1))
        wk.set_labels(*fixed)
        st = wk.suffstats_packed()
        w8 = make_worker(pkg, P, 0, labels=fixed)
        st8 = w8.suffstats_packed()
        w8.set_params_mult(P["logp"], P["lr"], P["w"])
        np.testing.assert_allclose(w8.debug_loglik(), tab, rtol=2e-6, atol=2e-4)
        assert np.array_equal(st8, st)
        want = np.zeros((2 * K, 1 + D))
        np.add.at(want, 2 * (fixed[0] - 1) + (fixed[1] - 1), np.concatenate([np.ones((P["n"], 1)), P["X"].astype(np.float64)], axis=1))
        assert np.array_equal(st, want)
        w8.close()
    wk.close()


# --------------------------------------------------------------------------- 4. FP32 fallback kernel
@pytest.mark.parametrize("K,D", [(5, 100), (6, 17), (40, 100), (40, 17), (300, 17), (1024, 100), (1024, 17)])
def test_f32_fallback_kernel(pkg, K, D):
    """mult_sweep_kernel (data that is not bf16-exact): one row block (K = 5), two (K = 6), one full pass of eight, and many passes."""
    P = reference("f32", K, D)
    what = f"f32 K={K} D={D} NRB={(3 * K + 15) // 16}"
    wk = make_worker(pkg, P)
    wk.set_params_mult(P["logp"], P["lr"], P["w"])
    tab, tab2 = check_tables(pkg, wk, P, what)
    wk.sweep(2)
    lab, sub = wk.get_labels()
    u0 = check_draws(tab, tab2, lab, sub, 2, what)
    check_oracle(P, lab, sub, u0, 2, what)
    wk.close()


# --------------------------------------------------------------------------- 5. dense statistics at large K
@pytest.mark.parametrize("K", [33, 600, 1024])
@pytest.mark.parametrize("kind", ["bytes", "f32"])
def test_dense_statistics_large_k(pkg, K, kind):
    """mult_stats_u8_kernel / mult_stats_kernel + mult_reduce_kernel with up to 2048 bins, some of them empty: Float64 numpy and the oracle.
    Count data: exact.  Shifted data: the kernels add Float64 in another order than numpy (rtol 1e-12 / atol 1e-9, the suite's tolerance
    for Float64 sums); the oracle adds in Float32, one point after the other: N 2^-24 times the sum is the bound of ITS rounding."""
    D, n = 40, 6000
    rng = np.random.default_rng(1000 + K)
    X = rng.poisson(0.3, size=(n, D)).astype(np.float32)
    X[::11, 3] = 255.0
    if kind == "f32":
        X = (X + np.float32(0.3)).astype(np.float32)
    lab = rng.integers(1, K + 1, n); sub = rng.integers(1, 3, n)
    empty = np.array([2, K // 2, K - 1])
    lab[np.isin(lab, empty)] = 1                               # some clusters empty
    sub[lab == 5] = 2                                          # ... and a cluster with an empty left side
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points(X)
    wk.set_labels(lab, sub)
    wk.set_num_clusters(K)
    st = wk.suffstats_packed()
    want = np.zeros((2 * K, 1 + D))
    np.add.at(want, 2 * (lab - 1) + (sub - 1), np.concatenate([np.ones((n, 1)), X.astype(np.float64)], axis=1))
    oN, os_ = orc.suffstats_mult(X, D, lab, sub, K)
    N, s = wk.unpack(st)
    assert np.array_equal(st[:, 0], want[:, 0]) and np.array_equal(N, oN.astype(np.float64))
    assert not st[2 * (empty - 1)].any() and not st[2 * (empty - 1) + 1].any() and not st[2 * 4].any()
    if kind == "bytes":
        assert np.array_equal(st, want) and np.array_equal(s, os_.astype(np.float64))
    else:
        np.testing.assert_allclose(st, want, rtol=1e-12, atol=1e-9)
        tol = 1.01 * N[:, :, None] * 2.0 ** -24 * np.abs(s) + 1e-30
        assert np.all(np.abs(s - os_.astype(np.float64)) <= tol), float((np.abs(s - os_) / tol).max())
    idx = np.unique(np.concatenate([rng.integers(1, K, 4), [K]]))          # a subset pass, the last cluster in it
    part = wk.suffstats_packed(idx)
    rows = np.concatenate([2 * (idx - 1), 2 * (idx - 1) + 1])
    if kind == "bytes":
        assert np.array_equal(part[rows], st[rows])
    else:
        np.testing.assert_allclose(part[rows], st[rows], rtol=1e-12, atol=1e-9)
    rest = np.setdiff1d(np.arange(2 * K), rows)
    assert not part[rest].any()
    with pytest.raises(pkg.DpmmError):
        wk.set_num_clusters(1025)
    wk.close()
