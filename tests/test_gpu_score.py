"""GPU tests of include/dpmm_hip_score.h (csrc/score.hip, the slabbed table mode of run_sweep) and of host/score.py's Predictor.

The reference of every case is the context's OWN dpmm_predict table and dpmm_predict_points output on the same points, post-processed in
numpy: labels, probabilities and the top-m are compared bit for bit; the log-density against the Float64 log-sum-exp of the Float32
table within 2^-23 (K + 16) + 2^-23 |ref| -- K terms of at most 1 from a few-ulp expf, K - 1 Float32 additions, one logf, one final
addition; about a factor of two of margin.  Shapes: 3 tiles + 5 points of the path's tile, the smallest that has whole tiles, a ragged
end and more than one slab at the small budgets.
The NIW table these cases bootstrap from has its independent anchor in tests/test_gpu_predictive.py (a Float64 closed form, a derived bound)."""
import ctypes
import importlib
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K0 = 5
EPS = 2.0 ** -23


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


# ------------------------------------------------------------------------------------------------ problems
def niw_params(rng, D, K, twins=False):
    m = (rng.standard_normal((K, D)) * 0.2).astype(np.float32)
    R = np.triu(rng.standard_normal((K, D, D)) * 0.05) + np.eye(D)
    logdet = (-2 * np.log(np.abs(np.einsum("kii->ki", R))).sum(1)).astype(np.float32)
    df = (5 + rng.random(K)).astype(np.float32)
    w = rng.dirichlet(np.full(K, 20.0)).astype(np.float32)
    R = R.astype(np.float32)
    if twins:                                   # clusters 2 and 4 (1-based) identical: an exact tie in every row
        m[3], R[3], logdet[3], df[3] = m[1], R[1], logdet[1], df[1]
        w[3] = w[1]
    return m, R.reshape(K, -1), logdet, df, w


def niw_points(rng, D, n, m):
    z = rng.integers(0, len(m), n)
    return (m[z] + rng.standard_normal((n, D))).astype(np.float32)


def mult_params(rng, D, K):
    base = rng.dirichlet(np.full(D, 5.0))
    p = base[None, :] * np.exp(0.2 * rng.standard_normal((K, D)))
    p /= p.sum(1, keepdims=True)
    return np.log(p).astype(np.float32), rng.dirichlet(np.full(K, 20.0)).astype(np.float32)


def tile_of(kind, D):
    return 128 if (kind == "niw" and D > 64) else 256


PATHS = {      # name -> (kind, D)
    "niw2": ("niw", 2), "niw64": ("niw", 64), "niw128": ("niw", 128),
    "mult_f32": ("mult", 40), "mult_bf16": ("mult", 40), "mult_u8": ("mult", 40), "mult_sparse": ("mult", 5000),
}


def make_worker(pkg, name, n=None, K=K0, seed=0, twins=False):
    """A worker with points and predictive parameters of the named storage path."""
    kind, D = PATHS[name]
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    n = 3 * tile_of(kind, D) + 5 if n is None else n
    if kind == "niw":
        par = niw_params(rng, D, K, twins)
        wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
        wk.upload_points(niw_points(rng, D, n, par[0]))
        wk.set_predictive_niw(*par)
        return wk
    logp, w = mult_params(rng, D, K)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    if name == "mult_sparse":
        cnt = rng.integers(15, 26, n)
        cp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        rv = np.concatenate([np.sort(rng.choice(D, c, replace=False)) for c in cnt]).astype(np.int64)
        nz = rng.integers(1, 6, rv.size).astype(np.float32)
        wk.upload_points_csc(cp, rv, nz, index_base=0)
    else:
        X = rng.poisson(0.8, (n, D)).astype(np.float32)                # counts: the byte kernel
        if name == "mult_f32":
            X += np.float32(0.3) * (rng.random((n, D)) < 0.3)          # 0.3 is not a bf16 value: the Float32 kernel
        elif name == "mult_bf16":
            X += np.float32(0.5) * (rng.random((n, D)) < 0.3)          # halves are bf16-exact, not integers: the bf16 kernel
        wk.upload_points(X)
    wk.set_predictive_mult(logp, w)
    return wk


_cache = {}


def cached(pkg, name, **kw):
    """(worker, reference) of a case, built once and shared; the reference is never modified."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _cache:
        wk = make_worker(pkg, name, **kw)
        _cache[key] = (wk, reference(wk))
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_workers():
    yield
    for wk, _ in _cache.values():
        wk.close()
    _cache.clear()


def reference(wk):
    """The context's own table and predict_points output, and what the definitions make of them."""
    K, n = wk.K, wk.n
    tab = np.empty((K, n), np.float32)
    wk._chk(wk._lib.dpmm_predict(wk._h, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    lab, probs = wk._predict_points(K)
    with np.errstate(all="ignore"):
        a = np.where(np.isnan(tab), -np.inf, tab).astype(np.float64)
        M = a.max(0)
        ld = np.where(np.isneginf(M), -np.inf, M + np.log(np.exp(a - np.where(np.isfinite(M), M, 0.0)).sum(0)))
    nanrow = np.isnan(probs).all(1)
    order = np.argsort(-probs, axis=1, kind="stable")
    order[nanrow] = np.arange(K)[None, :]                # a row without a finite entry: indices 1..m, the NaNs probs holds
    return dict(tab=tab, labels=lab, probs=probs, logdens=ld, order=order, nanrow=nanrow)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check(out, ref, m, K):
    if "labels" in out:
        assert np.array_equal(out["labels"], ref["labels"])
    if "probs" in out:
        assert same(out["probs"], ref["probs"])
    if "logdens" in out:
        got, want = out["logdens"].astype(np.float64), ref["logdens"]
        inf = np.isneginf(want)
        assert np.array_equal(np.isneginf(got), inf)
        d = np.abs(got[~inf] - want[~inf])
        bound = EPS * (K + 16) + EPS * np.abs(want[~inf])
        print("logdens: max |d| / bound = %.3f" % (float((d / bound).max()) if d.size else 0.0))
        assert np.all(d <= bound)
    if m:
        want_idx = ref["order"][:, :m] + 1
        assert np.array_equal(out["top_idx"], want_idx)
        assert same(out["top_prob"], np.take_along_axis(ref["probs"], want_idx - 1, axis=1))


def no_ties(ref, m):
    """Apart from the deliberate rows the reference has no two equal probabilities among the best m (and the one behind them)."""
    p = -np.sort(-ref["probs"][~ref["nanrow"]], axis=1)[:, :m + 1]
    return bool(np.all(np.diff(p, axis=1) < 0))


def run_all(wk, m):
    return wk.score_points(labels=True, logdens=True, m=m, probs=True)


# ------------------------------------------------------------------------------------------------ per storage path
@pytest.mark.parametrize("name", list(PATHS))
def test_every_output_on_every_storage_path(pkg, name):
    wk, ref = cached(pkg, name)
    assert not ref["nanrow"].any() and np.isfinite(ref["tab"]).all()
    for m in (1, 4, K0):
        assert no_ties(ref, min(m, K0 - 1)), "the case has ties among its best probabilities: choose other inputs"
        check(run_all(wk, m), ref, m, K0)
    dev = wk.score_points(labels=True, logdens=True, m=4, probs=True, device=DEV)        # the device variant writes the same bits
    host_out = run_all(wk, 4)
    for k, v in dev.items():
        assert same(v.cpu().numpy(), host_out[k]), k


@pytest.mark.parametrize("name", list(PATHS))
def test_results_do_not_depend_on_the_table_budget(pkg, binding, name):
    wk, ref = cached(pkg, name)
    kind, D = PATHS[name]
    rows = K0 * (1 if kind == "niw" else 3)
    base = run_all(wk, 4)
    check(base, ref, 4, K0)
    try:
        for mb in (0.0, 2 * rows * tile_of(kind, D) * 4 / 2.0 ** 20):      # one-tile slabs | two-tile slabs: the last is one tile + 5 points
            wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
            got = run_all(wk, 4)
            for k in base:
                assert same(got[k], base[k]), (mb, k)
            gd = wk.score_points(labels=True, logdens=True, m=4, probs=True, device=DEV)
            for k in base:
                assert same(gd[k].cpu().numpy(), base[k]), (mb, k, "device")
    finally:
        wk.set_option(binding.OPT_SCORE_TABLE_MB, -1)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("K,n", [(1, 261), (2, 261), (70, 261), (5, 1), (5, 256)])
def test_edges_of_K_and_n(pkg, binding, K, n):
    wk, ref = cached(pkg, "niw2", n=n, K=K)
    for m in sorted({1, min(4, K), min(K, 16)}):
        assert no_ties(ref, min(m, K - 1))
        check(run_all(wk, m), ref, m, K)
    if K == 1:
        out = run_all(wk, 1)
        assert np.all(out["probs"] == 1.0) and same(out["logdens"], ref["tab"][0])
    if K == 70:                                   # more than one transposition tile, also with one-tile slabs
        wk.set_option(binding.OPT_SCORE_TABLE_MB, 0.0)
        try:
            check(run_all(wk, 16), ref, 16, K)
        finally:
            wk.set_option(binding.OPT_SCORE_TABLE_MB, -1)


def test_niw_point_with_a_nan_feature(pkg):
    D, K, n = 2, 5, 261
    rng = np.random.default_rng(7)
    par = niw_params(rng, D, K)
    X = niw_points(rng, D, n, par[0])
    X[7, 0] = np.nan
    X[258, 1] = np.nan
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_niw(*par)
    ref = reference(wk)
    assert np.isnan(ref["tab"][:, 7]).all() and list(np.flatnonzero(ref["nanrow"])) == [7, 258]
    for m in (1, 4, 5):
        out = run_all(wk, m)
        check(out, ref, m, K)
        assert out["labels"][7] == 1 and np.isneginf(out["logdens"][7])          # the first NaN row; M = -Inf
        assert list(out["top_idx"][7]) == list(range(1, m + 1)) and np.isnan(out["top_prob"][7]).all()
    wk.close()


def test_multinomial_row_where_every_cluster_is_nan_or_minus_inf(pkg):
    D, K, n = 40, 5, 261
    rng = np.random.default_rng(8)
    logp, w = mult_params(rng, D, K)
    X = rng.poisson(0.8, (n, D)).astype(np.float32) + np.float32(0.3) * (rng.random((n, D)) < 0.3)
    X[3, 5] = np.inf            # inf * log p = -Inf under every cluster
    X[200, 0] = np.nan          # NaN under every cluster
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points(X)
    wk.set_predictive_mult(logp, w)
    ref = reference(wk)
    assert np.isneginf(ref["tab"][:, 3]).all() and np.isnan(ref["tab"][:, 200]).all()
    out = run_all(wk, 4)
    check(out, ref, 4, K)
    assert np.isneginf(out["logdens"][3]) and np.isneginf(out["logdens"][200])
    assert same(out["probs"][[3, 200]], ref["probs"][[3, 200]])
    wk.close()


def test_an_exact_tie_goes_to_the_lower_index(pkg):
    wk, ref = cached(pkg, "niw2", n=261, K=5, twins=True)
    p = ref["probs"]
    assert same(p[:, 1], p[:, 3])                                   # clusters 2 and 4 are the same distribution with the same weight
    out = run_all(wk, 5)
    check(out, ref, 5, 5)
    pos2 = np.argmax(out["top_idx"] == 2, axis=1)
    pos4 = np.argmax(out["top_idx"] == 4, axis=1)
    assert np.all(pos4 == pos2 + 1)
    best_is_twin = ref["order"][:, 0] == 1
    assert best_is_twin.any() and np.all(out["labels"][best_is_twin] == 2)


# ------------------------------------------------------------------------------------------------ output selection, allocation
def test_single_outputs_match_the_full_call_and_a_second_call_allocates_nothing(pkg):
    wk, ref = cached(pkg, "niw64")
    full = run_all(wk, 4)
    singles = [dict(labels=True), dict(logdens=True), dict(probs=True), dict(m=4, top_prob=False), dict(m=4, top_idx=False), dict(m=4)]
    for kw in singles:
        for device in (None, DEV):
            got = wk.score_points(device=device, **kw)
            for k, v in got.items():
                assert same(v if device is None else v.cpu().numpy(), full[k]), (kw, k, device)
    # second call of the same shape: no device allocation (free bytes unchanged)
    outs = dict(labels=torch.empty(wk.n, dtype=torch.int64, device=DEV), logdens=torch.empty(wk.n, dtype=torch.float32, device=DEV),
                top_idx=torch.empty((wk.n, 4), dtype=torch.int64, device=DEV), top_prob=torch.empty((wk.n, 4), dtype=torch.float32, device=DEV),
                probs=torch.empty((wk.n, K0), dtype=torch.float32, device=DEV))
    houts = {k: np.empty(tuple(v.shape), full[k].dtype) for k, v in outs.items()}
    for o in (outs, houts):
        wk.score_points_into(o, m=4)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info(0)[0]
        wk.score_points_into(o, m=4)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == before
    for k in full:
        assert same(outs[k].cpu().numpy(), full[k]) and same(houts[k], full[k])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(pkg, binding):
    n = (1 << 21) + 1
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_NIW, 2, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, 2)).astype(np.float32))
    torch.cuda.empty_cache()
    short = torch.empty(n - 1, dtype=torch.int64, device=DEV)          # exactly 16 MiB: an allocation of its own, one row short
    good = torch.empty(n, dtype=torch.int64, device=DEV)
    fl = torch.empty((n, 2), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    hostbuf = np.empty(n, np.int64)

    def refused(code, *what, device=True, **kw):
        with pytest.raises(pkg.DpmmError) as e:
            wk.score_points_raw(device, **kw)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    refused(-4, labels=good.data_ptr())                                 # DPMM_ESTATE: no predictive parameters yet
    wk.set_predictive_niw(*niw_params(rng, 2, 2))
    refused(-1, "labels", labels=hostbuf.ctypes.data)                   # a host pointer given to the device variant
    refused(-1, "labels", "allocation", labels=short.data_ptr())        # too small by one row
    refused(-1, "probs", "aligned", labels=good.data_ptr(), probs=fl.data_ptr() + 2)
    refused(-1, "m = 0", labels=good.data_ptr(), m=0, top_idx=good.data_ptr())
    refused(-1, "m must", labels=good.data_ptr(), m=17, top_idx=good.data_ptr())
    refused(-1, "m exceeds", labels=good.data_ptr(), m=3, top_idx=good.data_ptr())      # K = 2
    refused(-1, "null")                                                 # all-NULL
    refused(-1, "null", device=False)
    wk.score_points_raw(True, labels=good.data_ptr(), logdens=fl.data_ptr())      # the valid call still works
    assert np.array_equal(good.cpu().numpy(), wk._predict_points(2)[0])
    wk.close()


def test_scoring_ignores_lds_and_register_contents(pkg, binding):
    """The finish kernel under tests/tools/poison.py (its launches go through the library's generic pre-launch hook): same bits."""
    from tools import poison
    poison.build()
    wk, ref = cached(pkg, "niw2", n=261, K=70)
    clean = run_all(wk, 16)
    with poison.poisoned_kernel_launches(binding, 0xffffffff) as launches:
        dirty = run_all(wk, 16)
    assert launches[0] >= 2
    for k in clean:
        assert same(clean[k], dirty[k]), k


# ------------------------------------------------------------------------------------------------ Predictor
@pytest.fixture(scope="module")
def niw_model(host):
    x, _, _, _ = host.generate_gaussian_data(3000, 8, 4, 20.0, seed=5)
    return host.fit(x, 10.0, iters=25, seed=11, burnout=5, verbose=False)[-1]


@pytest.fixture(scope="module")
def mult_model(host):
    x = host.generate_mnmm_data(3000, 40, 4, 60, seed=6)[0]
    hyper = host.multinomial_hyper(np.ones(40, np.float32))
    return host.fit(x, hyper, 10.0, iters=25, seed=11, burnout=5, verbose=False)[-1]


CAP = 2 * 256 + 3
NP = 2 * CAP + 7


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def test_predictor_equals_predict_for_every_kind_of_input(host, niw_model, mult_model):
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((NP, 8)) * 4).astype(np.float32)                   # (N, D)
    bf = torch.from_numpy(x).to(DEV).to(torch.bfloat16)                         # contiguous (N, D); .T is the (D, N) view
    f16 = torch.from_numpy(x).to(DEV).to(torch.float16)
    wide = torch.zeros((2 * 8, 3 * NP + 1), dtype=torch.float16, device=DEV)
    wide[::2, ::3][:, :NP] = f16.T
    inputs = [np.ascontiguousarray(x.T), bf.T, wide[::2, ::3][:, :NP]]
    assert not inputs[2].is_contiguous()
    with host.Predictor(niw_model, capacity=CAP) as p:
        for data in inputs:
            lab, probs = host.predict(niw_model, data)
            got_lab, got_probs = p.predict(data)
            assert torch.is_tensor(got_lab) == torch.is_tensor(data) and torch.is_tensor(got_probs) == torch.is_tensor(data)
            if torch.is_tensor(data):
                assert got_lab.device == data.device and got_probs.device == data.device
            assert np.array_equal(as_np(got_lab), as_np(lab)) and same(as_np(got_probs), as_np(probs))
            assert np.array_equal(as_np(p.predict_labels(data)), as_np(lab))
            l3, idx, tp = p.predict_topk(data, 3)
            want = np.argsort(-as_np(probs), axis=1, kind="stable")[:, :3] + 1
            assert np.array_equal(as_np(idx), want) and same(as_np(tp), np.take_along_axis(as_np(probs), want - 1, axis=1))
            assert np.array_equal(as_np(l3), as_np(lab))
            ld = as_np(p.score_samples(data))
            assert ld.shape == (NP,) and ld.dtype == np.float32 and np.isfinite(ld).all()
        # one Predictor, consecutive calls of different n, n < capacity included
        for n in (CAP - 200, CAP, NP - 1):
            for data in (inputs[0][:, :n], inputs[1][:, :n]):
                lab, probs = host.predict(niw_model, data)
                got = p.predict(data)
                assert as_np(got[0]).shape == (n,) and as_np(got[1]).shape == (n, as_np(probs).shape[1])
                assert np.array_equal(as_np(got[0]), as_np(lab)) and same(as_np(got[1]), as_np(probs))
        ld_p = p.score_samples(inputs[0])
    # the module-level conveniences; the slab size changes nothing
    assert same(host.score_samples(niw_model, inputs[0], capacity=CAP), ld_p)
    assert same(host.score_samples(niw_model, inputs[0], capacity=4 * CAP), ld_p)
    li, ii, pi = host.predict_topk(niw_model, inputs[0], 2, capacity=CAP)
    assert ii.shape == (NP, 2) and pi.shape == (NP, 2)


def test_predictor_sparse_columns_and_save_load(host, mult_model, niw_model):
    import scipy.sparse as sp
    rng = np.random.default_rng(10)
    X = rng.poisson(0.6, (40, NP)).astype(np.float32)                           # (D, N) counts
    csc = sp.csc_matrix(X)
    lab, probs = host.predict(mult_model, csc)
    with host.Predictor(mult_model, capacity=CAP) as p:
        got = p.predict(csc)
        assert np.array_equal(got[0], lab) and same(got[1], probs)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "model.npz")
            p.save(path)
            with host.Predictor.load(path, capacity=CAP) as q:
                again = q.predict(csc)
                assert np.array_equal(again[0], lab) and same(again[1], probs)
                assert same(q.score_samples(csc), p.score_samples(csc))
    x = (rng.standard_normal((8, 300)) * 4).astype(np.float32)
    with host.Predictor(niw_model, capacity=CAP) as p, tempfile.TemporaryDirectory() as d:
        p.save(os.path.join(d, "m.npz"))
        with host.Predictor.load(os.path.join(d, "m.npz"), device=0, capacity=128) as q:
            a, b = p.predict(x), q.predict(x)
            assert np.array_equal(a[0], b[0]) and same(a[1], b[1])
        with pytest.raises(TypeError):
            p.predict(sp.csc_matrix(np.abs(x)))


@pytest.mark.parametrize("kind", ["counts", "halves", "fractions"])
def test_predictor_dense_multinomial_input(host, mult_model, kind):
    """Dense Multinomial data of one kind throughout -- counts (byte kernel), bf16-exact halves (bf16 kernel), other fractions (Float32
    kernel): every slab takes the storage path `predict` takes for the whole data, so the results agree bit for bit for any capacity."""
    rng = np.random.default_rng(12)
    X = rng.poisson(0.6, (40, NP)).astype(np.float32)
    if kind != "counts":
        X += np.float32(0.5 if kind == "halves" else 0.3)              # every value: no slab can look like another kind
    lab, probs = host.predict(mult_model, X)
    dev_in = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV).T
    for cap in (CAP, 300):
        with host.Predictor(mult_model, capacity=cap) as p:
            got = p.predict(X)
            assert np.array_equal(got[0], lab) and same(got[1], probs), cap
            gd = p.predict(dev_in)
            assert np.array_equal(as_np(gd[0]), lab) and same(as_np(gd[1]), probs), cap

