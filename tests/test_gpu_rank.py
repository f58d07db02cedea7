"""GPU tests of include/dpmm_hip_rank.h (csrc/rank.hip) and of host/score.py's Predictor.exemplars.

Expected values come from the context's OWN table (dpmm_predict, as reference() in tests/test_gpu_score.py does) through the numpy
restatement of the definitions, tests/tools/rank_ref.py, and are compared bit for bit: indices, scores (equal to the table entry), the
-1 / NaN fill, counts and `skipped`.  The table itself is pinned by the predictive tests.  Shapes: 3 tiles + 5 points of the path's tile
as in test_gpu_score.py; 20 tiles + 5 where slabs of a Predictor matter; one case just above the 262144 points of a candidate buffer,
the only size at which the chunk loop of dpmm_rank_accumulate runs twice."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import test_gpu_score as S
from tools import rank_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K0 = S.K0
STORAGE = ["niw2", "niw64", "niw128", "mult_u8", "mult_sparse"]
KEYS = ("typ_idx", "typ_score", "fringe_idx", "fringe_score", "count", "skipped")


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def binding(pkg):
    return importlib.import_module(pkg.__name__ + ".binding")


@pytest.fixture(scope="module")
def host(pkg):
    return importlib.import_module(pkg.__name__ + ".host")


def table(wk):
    tab = np.empty((wk.K, wk.n), np.float32)
    wk._chk(wk._lib.dpmm_predict(wk._h, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return tab


_cache = {}


def cached(pkg, name, **kw):
    """(worker, its table) of a case of test_gpu_score.make_worker, built once and shared; the table is never modified."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _cache:
        wk = S.make_worker(pkg, name, **kw)
        _cache[key] = (wk, table(wk))
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_workers():
    yield
    for wk, _ in _cache.values():
        wk.close()
    _cache.clear()


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def bits(a):
    a = np.ascontiguousarray(as_np(a))
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def run(wk, m, which=3, device=None, n_valid=None, base=0):
    wk.rank_begin(m, which)
    wk.rank_accumulate(base, wk.n if n_valid is None else n_valid)
    return wk.rank_read(device=device)


def check(got, want, what=""):
    for k in KEYS:
        g = as_np(got[k])
        w = np.asarray(want[k]).reshape(g.shape).astype(g.dtype)
        assert same(g, w), (what, k)


def check_tuple(ex, want, what=""):
    """An `Exemplars` result against a rank_ref dict."""
    got = dict(typ_idx=ex.typical_idx, typ_score=ex.typical_score, fringe_idx=ex.fringe_idx, fringe_score=ex.fringe_score, count=ex.count,
               skipped=np.array([ex.skipped], np.int64))
    check(got, want, what)


# ------------------------------------------------------------------------------------------------ per storage path
@pytest.mark.parametrize("name", STORAGE)
def test_both_lists_on_every_storage_path(pkg, name):
    wk, tab = cached(pkg, name)
    assert np.isfinite(tab).all()
    for m in (1, 4, 64):
        want = rank_ref.rank(tab, m)
        got = run(wk, m)
        check(got, want, m)
        check(wk.rank_read(device=DEV), want, (m, "device"))                  # the device read writes the same bits
        assert want["count"].sum() == wk.n and want["skipped"] == 0
    print("counts:", want["count"].tolist())
    only = run(wk, 4, which=1)                                                  # one list: the other is all unused slots
    w4 = rank_ref.rank(tab, 4)
    assert same(only["typ_idx"], w4["typ_idx"]) and np.all(only["fringe_idx"] == -1) and np.isnan(only["fringe_score"]).all()
    only = run(wk, 4, which=2, device=DEV)
    assert same(only["fringe_score"], w4["fringe_score"]) and np.all(as_np(only["typ_idx"]) == -1) and same(only["count"], w4["count"])


@pytest.mark.parametrize("name", STORAGE)
def test_lists_do_not_depend_on_the_table_budget(pkg, binding, name):
    wk, tab = cached(pkg, name)
    kind, D = S.PATHS[name]
    rows = K0 * (1 if kind == "niw" else 3)
    want = rank_ref.rank(tab, 4)
    try:
        for mb in (0.0, 2 * rows * S.tile_of(kind, D) * 4 / 2.0 ** 20):      # one-tile slabs | two-tile slabs: the last is one tile + 5 points
            wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
            check(run(wk, 4), want, mb)
    finally:
        wk.set_option(binding.OPT_SCORE_TABLE_MB, -1)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("K,n", [(1, 261), (70, 261), (5, 1), (5, 256)])
def test_edges_of_K_and_n(pkg, K, n):
    wk, tab = cached(pkg, "niw2", n=n, K=K)
    for m in (1, 4, 64):
        want = rank_ref.rank(tab, m)
        check(run(wk, m), want, m)
        check(run(wk, m, device=DEV), want, (m, "device"))
    if K == 70 or n == 1:
        assert (want["count"] < 64).any() and (want["typ_idx"] == -1).any()   # the -1 / NaN fill is covered


def test_more_points_than_one_candidate_buffer(pkg):
    n = 262144 + 300
    wk, tab = cached(pkg, "niw2", n=n, K=5)
    want = rank_ref.rank(tab, 16)
    check(run(wk, 16), want)
    assert want["count"].sum() == n


def test_a_cluster_that_no_point_chooses(pkg):
    D, K, n = 2, 5, 261
    rng = np.random.default_rng(21)
    par = list(S.niw_params(rng, D, K))
    X = S.niw_points(rng, D, n, par[0])
    par[0][2] += 1000.0                                       # cluster 3 sits far from every point
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_niw(*par)
    want = rank_ref.rank(table(wk), 4)
    assert want["count"][2] == 0
    got = run(wk, 4)
    check(got, want)
    assert np.all(got["typ_idx"][2] == -1) and np.isnan(got["typ_score"][2]).all() and np.all(got["fringe_idx"][2] == -1) and got["count"][2] == 0
    wk.close()


# ------------------------------------------------------------------------------------------------ ties, skipped points, padding
def test_equal_scores_go_to_the_lower_index(pkg):
    D, K, n = 2, 5, 773
    rng = np.random.default_rng(23)                           # (a seed at which the twins own points: 356 of them by the Float64 closed form)
    par = S.niw_params(rng, D, K, twins=True)                 # clusters 2 and 4 identical: every point of theirs is labelled 2
    X = S.niw_points(rng, D, n, par[0])
    X[[7, 300, 600]] = par[0][1]                              # the same point at three indices, at a cluster's mean: the head of a typical list
    X[[11, 311, 611]] = par[0][0] + 9.0                       # and far out: the head of a fringe list
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_niw(*par)
    tab = table(wk)
    assert same(tab[1], tab[3])
    for m in (1, 4, 64):
        want = rank_ref.rank(tab, m)
        check(run(wk, m), want, m)
    assert want["count"][3] == 0 and want["count"][1] > 0
    got = run(wk, 4)
    assert any(row[:3].tolist() == [7, 300, 600] for row in got["typ_idx"]), got["typ_idx"]
    assert any(row[:3].tolist() == [11, 311, 611] for row in got["fringe_idx"]), got["fringe_idx"]
    one = run(wk, 1)                                          # m = 1: of three equal keys' points the lowest index stays
    assert 7 in one["typ_idx"] and 11 in one["fringe_idx"] and 300 not in one["typ_idx"] and 311 not in one["fringe_idx"]
    wk.close()


def test_a_niw_point_with_a_nan_feature_is_skipped(pkg):
    D, K, n = 2, 5, 261
    rng = np.random.default_rng(7)
    par = S.niw_params(rng, D, K)
    X = S.niw_points(rng, D, n, par[0])
    X[7, 0] = np.nan
    X[258, 1] = np.nan
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_niw(*par)
    tab = table(wk)
    assert np.isnan(tab[:, 7]).all() and np.isnan(tab[:, 258]).all()
    for m in (4, 64):
        want = rank_ref.rank(tab, m)
        got = run(wk, m)
        check(got, want, m)
        assert got["skipped"][0] == 2 and got["count"].sum() == n - 2
        for k in ("typ_idx", "fringe_idx"):
            assert 7 not in got[k] and 258 not in got[k]
    wk.close()


def test_a_multinomial_row_of_nan_or_minus_inf_is_skipped(pkg):
    D, K, n = 40, 5, 261
    rng = np.random.default_rng(8)
    logp, w = S.mult_params(rng, D, K)
    X = rng.poisson(0.8, (n, D)).astype(np.float32) + np.float32(0.3) * (rng.random((n, D)) < 0.3)
    X[3, 5] = np.inf            # inf * log p = -Inf under every cluster
    X[200, 0] = np.nan          # NaN under every cluster
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_mult(logp, w)
    tab = table(wk)
    assert np.isneginf(tab[:, 3]).all() and np.isnan(tab[:, 200]).all()
    want = rank_ref.rank(tab, 64)
    got = run(wk, 64)
    check(got, want)
    assert got["skipped"][0] == 2 and got["count"].sum() == n - 2
    for k in ("typ_idx", "fringe_idx"):
        assert 3 not in got[k] and 200 not in got[k]
    wk.close()


def write_model(path, kind, D, K, rng, zero_mean=False):
    """A model file as Predictor.save writes it, without a fit."""
    if kind == "niw":
        m = rng.standard_normal((K, D)) * 3
        if zero_mean:
            m[0] = 0.0
        U = np.triu(rng.standard_normal((K, D, D)) * 0.1) + 2 * np.eye(D)
        post = dict(post_kappa=1 + 50 * rng.random(K), post_nu=D + 3 + 50 * rng.random(K), post_m=m, post_U=U)
    else:
        post = dict(post_alpha=(0.2 + rng.random((K, D)) * np.exp(rng.standard_normal((K, D)))).astype(np.float32))
    np.savez(path, kind=np.int64(0 if kind == "niw" else 1), D=np.int64(D), alpha=np.float64(10.0), points_count=rng.integers(50, 500, K).astype(np.float64), **post)
    return post


def test_the_zero_padding_of_a_short_slab_takes_no_part(host, tmp_path):
    D, K, n, cap = 4, 4, 300, 256
    rng = np.random.default_rng(23)
    path = str(tmp_path / "m.npz")
    post = write_model(path, "niw", D, K, rng, zero_mean=True)
    X = (post["post_m"][rng.integers(0, K, n)] + rng.standard_normal((n, D))).T.astype(np.float32)      # (D, n); no point at the origin
    with host.Predictor.load(path, capacity=n) as p:
        p.predict_labels(X)
        want = rank_ref.rank(table(p._wk), 8)
    with host.Predictor.load(path, capacity=cap) as p:
        got = p.exemplars(X, 8)
        # what the worker holds now: the short slab, 44 points and 212 rows of zeros -- ranked whole, a row of zeros heads cluster 1
        padded = rank_ref.rank(table(p._wk), 8)
        assert padded["typ_idx"][0, 0] >= n - cap
    check_tuple(got, want)
    assert max(int(got.typical_idx.max()), int(got.fringe_idx.max())) < n and int(got.count.sum()) + got.skipped == n


# ------------------------------------------------------------------------------------------------ accumulation, allocation, refusals
def test_accumulation_over_calls_reading_twice_and_beginning_again(pkg):
    wk, tab = cached(pkg, "niw64")
    n, m = wk.n, 16
    wk.rank_begin(m)
    wk.rank_accumulate(0, 500)
    wk.rank_accumulate(100000, n)                              # the same upload again, as other global indices
    first, second, dev = wk.rank_read(), wk.rank_read(), wk.rank_read(device=DEV)
    want = rank_ref.merge([rank_ref.rank(tab, m, 0, 500), rank_ref.rank(tab, m, 100000)], m)
    check(first, want)
    for k in KEYS:
        assert same(first[k], second[k]) and same(first[k], dev[k]), k
    wk.rank_accumulate(7, 0)                                   # nothing
    check(wk.rank_read(), want)
    check(run(wk, m), rank_ref.rank(tab, m), "begin clears")
    # a second pass of the same shape allocates nothing (free bytes unchanged), host and device reads included
    outs = wk.rank_read(device=DEV)
    ptr = {k: v.data_ptr() for k, v in outs.items()}
    houts = {k: np.empty(tuple(v.shape), as_np(v).dtype) for k, v in outs.items()}

    def one_pass():
        wk.rank_begin(m)
        wk.rank_accumulate(0, n)
        wk.rank_read_raw(True, **ptr)
        wk.rank_read_raw(False, **{k: v.ctypes.data for k, v in houts.items()})
        torch.cuda.synchronize()

    one_pass()
    before = torch.cuda.mem_get_info(0)[0]
    one_pass()
    assert torch.cuda.mem_get_info(0)[0] == before
    check(outs, rank_ref.rank(tab, m))
    check(houts, rank_ref.rank(tab, m))


def test_refusals_come_before_any_launch(pkg):
    n = 300
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_NIW, 2, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, 2)).astype(np.float32))

    def refused(code, fn, *a, what=(), **kw):
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a, **kw)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    refused(-4, wk.rank_begin, 4, 3)                                   # DPMM_ESTATE: no predictive parameters yet
    refused(-4, wk.rank_accumulate, 0, n)                              # no dpmm_rank_begin
    refused(-4, wk.rank_read_raw, False)
    wk.set_predictive_niw(*S.niw_params(rng, 2, 3))
    for m in (0, 65):
        refused(-1, wk.rank_begin, m, 3, what=("m must",))
    for which in (0, 4):
        refused(-1, wk.rank_begin, 4, which, what=("which",))
    refused(-4, wk.rank_accumulate, 0, n)                              # a refused begin starts nothing
    wk.rank_begin(4, 3)
    refused(-1, wk.rank_accumulate, 0, n + 1, what=("n_valid",))
    refused(-1, wk.rank_accumulate, 0, -1, what=("n_valid",))
    refused(-1, wk.rank_accumulate, -1, n, what=("indices",))
    refused(-1, wk.rank_accumulate, 2 ** 32 - n + 1, n, what=("indices",))
    wk.rank_accumulate(2 ** 32 - n, n)                                 # the last index a key holds
    got = wk.rank_read()
    assert got["typ_idx"].max() < 2 ** 32 and got["typ_idx"][got["typ_idx"] >= 0].min() >= 2 ** 32 - n and got["count"].sum() == n
    hostbuf = np.empty(64, np.int64)
    fl = torch.empty(3 * 4 + 1, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    refused(-1, wk.rank_read_raw, True, what=("count",), count=hostbuf.ctypes.data)               # a host pointer given to the device variant
    refused(-1, wk.rank_read_raw, True, what=("fringe_score", "aligned"), fringe_score=fl.data_ptr() + 2)
    wk.set_predictive_niw(*S.niw_params(rng, 2, 4))                   # another K than begin saw
    refused(-4, wk.rank_accumulate, 0, n)
    wk.close()


def test_ranking_ignores_lds_and_register_contents(pkg, binding):
    """Filter, merge and read kernels under tests/tools/poison.py (their launches go through the library's pre-launch hook): same bits."""
    from tools import poison
    poison.build()
    wk, tab = cached(pkg, "niw2", n=261, K=70)
    clean = run(wk, 64)
    with poison.poisoned_kernel_launches(binding, 0xffffffff) as launches:
        dirty = run(wk, 64)
    assert launches[0] >= 4                                            # the sweep, the filter, the merge, the read
    for k in KEYS:
        assert same(clean[k], dirty[k]), k
    check(dirty, rank_ref.rank(tab, 64))


# ------------------------------------------------------------------------------------------------ Predictor.exemplars
NP = 20 * 256 + 5


@pytest.fixture(scope="module")
def niw_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rank") / "niw.npz")
    post = write_model(path, "niw", 8, 6, np.random.default_rng(31))
    return path, post


def full_table(host, path, X):
    """(K, n) table of all points at once: a Predictor of capacity n after one upload."""
    with host.Predictor.load(path, capacity=X.shape[1]) as p:
        p.predict_labels(X)
        return table(p._wk)


def test_exemplars_do_not_depend_on_the_capacity_or_the_order_of_the_points(host, niw_file):
    path, post = niw_file
    rng = np.random.default_rng(32)
    X = (post["post_m"][rng.integers(0, 6, NP)] + 1.5 * rng.standard_normal((NP, 8))).T.astype(np.float32)      # (D, n)
    s = full_table(host, path, X).max(0)
    up = np.argsort(s, kind="stable")
    # as given | by ascending score: every point beats the running typical threshold | by descending score: none does after the first slab
    for what, perm in (("given", np.arange(NP)), ("ascending", up), ("descending", up[::-1])):
        Xp = np.ascontiguousarray(X[:, perm])
        want = rank_ref.rank(full_table(host, path, Xp), 16)
        assert want["skipped"] == 0 and want["count"].min() >= 16
        for cap in (NP, 256, 1000):
            with host.Predictor.load(path, capacity=cap) as p:
                check_tuple(p.exemplars(Xp, 16), want, (what, cap))


def test_exemplars_of_device_tensors_equal_those_of_host_arrays(host, niw_file, tmp_path):
    import scipy.sparse as sp
    path, post = niw_file
    rng = np.random.default_rng(33)
    n = 5 * 256 + 5
    x = (post["post_m"][rng.integers(0, 6, n)] + 1.5 * rng.standard_normal((n, 8))).astype(np.float32)      # (n, D)
    bf = torch.from_numpy(x).to(DEV).to(torch.bfloat16)                        # contiguous (n, D); .T is the (D, n) view
    xh = np.ascontiguousarray(bf.float().cpu().numpy().T)                      # the same values as a host array
    with host.Predictor.load(path, capacity=512) as p:
        a, b = p.exemplars(xh, 16), p.exemplars(bf.T, 16)
        lab = p.predict_labels(xh)
    assert torch.is_tensor(b.typical_idx) and b.typical_idx.device == bf.device and torch.is_tensor(b.count) and isinstance(b.skipped, int)
    assert isinstance(a.typical_idx, np.ndarray)
    for f in ("typical_idx", "typical_score", "fringe_idx", "fringe_score", "count"):
        assert same(getattr(a, f), getattr(b, f)), f
    assert a.skipped == b.skipped == 0
    for k in range(6):                                                         # indices are 0-based positions, labels 1-based
        assert np.all(lab[a.typical_idx[k]] == k + 1) and np.all(lab[a.fringe_idx[k]] == k + 1)
    assert np.all(np.diff(a.typical_score, axis=1) <= 0) and np.all(np.diff(a.fringe_score, axis=1) >= 0)
    # sparse counts: scipy CSC on the host, torch.sparse_csc on the device
    D, K = 60, 5
    mpath = str(tmp_path / "mult.npz")
    write_model(mpath, "mult", D, K, rng)
    C = rng.poisson(0.3, (D, n)).astype(np.float32)
    csc = sp.csc_matrix(C)
    tcsc = torch.sparse_csc_tensor(torch.from_numpy(csc.indptr.astype(np.int64)).to(DEV), torch.from_numpy(csc.indices.astype(np.int64)).to(DEV),
                                   torch.from_numpy(csc.data).to(DEV), size=(D, n))
    with host.Predictor.load(mpath, capacity=512) as p:
        a, b = p.exemplars(csc, 16), p.exemplars(tcsc, 16)
        lab = p.predict_labels(csc)
        whole = p.exemplars(csc, 16, which="fringe")
    with host.Predictor.load(mpath, capacity=n) as p:
        c = p.exemplars(csc, 16)
    assert torch.is_tensor(b.fringe_idx) and isinstance(a.fringe_idx, np.ndarray)
    for f in ("typical_idx", "typical_score", "fringe_idx", "fringe_score", "count"):
        assert same(getattr(a, f), getattr(b, f)) and same(getattr(a, f), getattr(c, f)), f
    assert whole.typical_idx is None and same(whole.fringe_idx, a.fringe_idx)
    for k in range(K):
        i = a.typical_idx[k][a.typical_idx[k] >= 0]
        assert np.all(lab[i] == k + 1)
    assert int(a.count.sum()) + a.skipped == n
