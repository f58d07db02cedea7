"""GPU tests of include/dpmm_hip_recommend.h (csrc/recommend.hip) and of host/score.py's Predictor.recommend.

The reference is numpy Float64 (tests/tools/recommend_ref.py) on what the library's own `predict` returns for the same data and
Predictor: r* = P.double() @ theta with theta = alpha' / sum(alpha') in Float64 and eps = (K + 2) 2^-24.  For EVERY point: every returned
prob within eps r* of r* at its feature, prob non-increasing, equal bits in increasing feature order, no feature twice, no seen feature
under exclude_seen, every candidate left out no better than the worst one returned (to within eps on both sides), -1 / NaN exactly behind
the candidates, labels those of `predict_labels` bit for bit, skipped the count of NaN rows.  Models are made through Predictor._setup from
posteriors written by hand, no fit.  One sweep per axis around D = 8, K = 5, n = 1000, m = 3: D across the 32-feature blocks and the four
waves of a workgroup, on the byte, Float32 and sparse stores up to D = 65536; K across the padded odd step, the score kernels' 16- and
64-cluster groups and DPMM_MAX_CLUSTERS; n across the 32-point tile; m across the two list widths of the kernel."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_gpu_score as S
import test_gpu_countstats as G
from tools import recommend_ref as RR

pytestmark = pytest.mark.gpu

DEV = G.DEV
as_np, same = G.as_np, G.same


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


def same_rec(a, b):
    return same(a.features, b.features) and same(a.prob, b.prob) and same(a.labels, b.labels) and a.skipped == b.skipped


def check(p, X, m, what, exclude=True, model_X=None, on_device=False):
    """One call checked against `predict` of the same Predictor on the same input; returns the Recommendation."""
    Xm = X if model_X is None else model_X
    n = Xm.shape[1]
    K, D = p.post["alpha"].shape
    lab, P = p.predict(X)
    got = p.recommend(X, m, exclude_seen=exclude)
    for a, shape in ((got.features, (n, m)), (got.prob, (n, m)), (got.labels, (n,))):
        assert tuple(a.shape) == shape, what
        assert (isinstance(a, torch.Tensor) and a.device == torch.device(DEV)) if on_device else isinstance(a, np.ndarray), what
    P = as_np(P)
    skip = np.isnan(P).any(1)
    worst = RR.check(as_np(got.features), as_np(got.prob), np.where(skip[:, None], 0, P), RR.theta_of(p.post["alpha"]), RR.seen_of(Xm) if exclude else None, m,
                     skip_rows=skip, what=what)
    print(what, "K", K, "D", D, "n", n, "m", m, "largest |prob - r*| in units of (K + 2) 2^-24 r*:", worst)
    assert same(got.labels, lab) and same(got.labels, p.predict_labels(X)), what
    assert isinstance(got.skipped, int) and got.skipped == int(skip.sum()), what
    return got


def run_case(host, post, X, cap, m, what, exclude=True, model_X=None, mb=None, binding=None, no_u8=False, on_device=False):
    with G.open_predictor(host, post, cap, no_u8=no_u8, binding=binding) as p:
        if mb is not None:
            p._wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
        return check(p, X, m, what, exclude=exclude, model_X=model_X, on_device=on_device)


# ------------------------------------------------------------------------------------------------ one sweep per axis
@pytest.mark.parametrize("D", [5, 32, 33, 64, 65, 1000])
def test_every_block_layout_of_dense_D(host, D):
    rng = np.random.default_rng(100 + D)
    post = G.posterior(D, 5, rng)
    got = run_case(host, post, G.counts_data(post, 1000, rng), 1000, 3, ("byte D", D))
    assert (got.features[:, 0] >= 0).sum() > 900 and got.skipped == 0


def test_float32_store_of_integer_counts(host, binding):
    rng = np.random.default_rng(1100)
    post = G.posterior(1000, 5, rng)
    X = G.counts_data(post, 1000, rng)
    got = run_case(host, post, X, 1000, 3, "Float32 store D 1000", no_u8=True, binding=binding)
    assert got.skipped == 0 and (got.features >= 0).all()


@pytest.mark.parametrize("D", [7169, 65536])
def test_sparse_D_up_to_the_widest(host, D):
    rng = np.random.default_rng(200 + D % 1000)
    post = G.posterior(D, 5, rng)
    X = G.sparse_data(D, 200, rng)
    got = run_case(host, post, X, 200, 3, ("sparse D", D))
    assert (np.diff(X.indptr) == 0).sum() > 0 and (got.features >= 0).all()         # a point without entries is an ordinary point
    got = run_case(host, post, X, 200, 3, ("sparse D, all features", D), exclude=False)
    assert (got.features >= 0).all()


@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 64, 65])
def test_every_K(host, K):
    rng = np.random.default_rng(300 + K)
    post = G.posterior(8, K, rng)
    run_case(host, post, G.counts_data(post, 1000, rng), 1000, 3, ("byte K", K))
    post = G.posterior(300, K, rng)
    run_case(host, post, G.sparse_data(300, 1000, rng), 1000, 3, ("sparse K", K))


def test_the_most_clusters(host):
    rng = np.random.default_rng(399)
    post = G.posterior(8, 1024, rng)
    run_case(host, post, G.counts_data(post, 100, rng), 100, 3, "K 1024")


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 2049])
def test_n_across_the_tiles(host, n):
    rng = np.random.default_rng(400 + n)
    post = G.posterior(8, 5, rng)
    run_case(host, post, G.counts_data(post, n, rng), n, 3, ("byte n", n))
    run_case(host, post, G.sparse_data(8, n, rng), n, 3, ("sparse n", n))


@pytest.mark.parametrize("m,D", [(1, 8), (5, 8), (16, 64)])
def test_every_m(host, m, D):
    rng = np.random.default_rng(500 + m)
    post = G.posterior(D, 5, rng)
    X = G.counts_data(post, 1000, rng)
    run_case(host, post, X, 1000, m, ("byte m", m))
    run_case(host, post, X, 1000, m, ("byte m, all features", m), exclude=False)
    run_case(host, post, sp.csc_matrix(X), 1000, m, ("sparse m", m))


def test_every_input_kind_of_one_matrix(host):
    D, K, n = 8, 5, 1000
    rng = np.random.default_rng(600)
    post = G.posterior(D, K, rng)
    X = G.counts_data(post, n, rng)
    Xs = sp.csc_matrix(X)
    emb = torch.from_numpy(X.T.copy()).to(DEV)                                     # (n, D): emb.T is the (D, n) view, read in place
    outs = {}
    outs["numpy"] = run_case(host, post, X, 256, 3, "numpy array")
    outs["strided"] = run_case(host, post, emb.T, 256, 3, "strided device tensor", model_X=X, on_device=True)
    outs["scipy"] = run_case(host, post, Xs, 256, 3, "scipy CSC")
    outs["torch"] = run_case(host, post, G.torch_csc(Xs), 256, 3, "torch.sparse_csc on the device", model_X=Xs, on_device=True)
    # (the byte and the sparse store evaluate the table with different kernels: each answer was checked against its own `predict`; the
    # two inputs that share a store agree to the bit)
    assert same(as_np(outs["strided"].features), outs["numpy"].features) and same(as_np(outs["strided"].prob), outs["numpy"].prob)
    assert same(as_np(outs["torch"].features), outs["scipy"].features) and same(as_np(outs["torch"].prob), outs["scipy"].prob)


def test_capacities_and_ranges_of_a_small_table_budget_agree(host, binding):
    D, K, n = 8, 5, 1000
    rng = np.random.default_rng(650)
    post = G.posterior(D, K, rng)
    for name, X in (("byte", G.counts_data(post, n, rng)), ("sparse", G.sparse_data(D, n, rng))):
        outs = {cap: run_case(host, post, X, cap, 3, (name, "capacity", cap)) for cap in (64, 1000, 1500)}
        assert S.tile_of("mult", D) < n                                            # budget 0: ranges of one tile, several per upload
        outs["ranges"] = run_case(host, post, X, 1000, 3, (name, "one-tile ranges"), mb=0.0, binding=binding)
        for key in (64, 1500, "ranges"):
            assert same_rec(outs[key], outs[1000]), (name, key)


# ------------------------------------------------------------------------------------------------ named cases
def test_ties_come_back_adjacent_lower_index_first(host):
    D, K, n = 40, 5, 300
    rng = np.random.default_rng(700)
    post = G.posterior(D, K, rng)
    a, b = 7, 35                                                                   # in different blocks of 32 features: different waves hold them
    post["alpha"][:, a] = post["alpha"][:, b] = np.array([40.0, 44.0, 48.5, 52.0, 33.25], np.float32)      # dyadic, the largest of every cluster
    X = G.counts_data(post, n, rng)
    X[a] = X[b] = 0                                                                # nobody has seen them
    for name, data in (("byte", X), ("sparse", sp.csc_matrix(X))):
        got = run_case(host, post, data, 128, 3, ("ties", name))
        assert (got.features[:, 0] == a).all() and (got.features[:, 1] == b).all(), name
        assert np.array_equal(got.prob[:, 0].view(np.uint32), got.prob[:, 1].view(np.uint32)), name


def test_one_hot_points_return_the_rounded_theta_row(host):
    D, K, n, m = 12, 4, 200, 5
    rng = np.random.default_rng(710)
    post = G.separated(D, K)
    post["alpha"] = post["alpha"] + (np.arange(D, dtype=np.float32) % 3) / 4.0       # not all equal off the preferred features
    X = G.counts_data(post, n, rng, trials=200)
    with G.open_predictor(host, post, 64, no_u8=False) as p:
        lab, P = p.predict(X)
        assert np.array_equal(np.sort(P, 1)[:, -1], np.ones(n, np.float32)) and (P.sum(1) == 1).all()      # exactly one-hot
        got = check(p, X, m, "one-hot")
    th32 = RR.theta_of(post["alpha"]).astype(np.float32)
    want_f, want_p = RR.topm(th32[lab - 1], RR.seen_of(X), m)
    assert np.array_equal(got.features, want_f) and same(got.prob, want_p)


@pytest.mark.parametrize("order", ["increasing", "decreasing"])
def test_every_block_beats_the_threshold(host, order):
    D, K, n = 1000, 5, 300
    rng = np.random.default_rng(720)
    alpha = (1.0 + np.arange(D)[None, :] * (np.arange(K)[:, None] + 1) / 8.0).astype(np.float32)
    post = dict(alpha=alpha if order == "increasing" else np.ascontiguousarray(alpha[:, ::-1]))
    X = G.counts_data(post, n, rng)
    got = run_case(host, post, X, 300, 3, ("adversarial", order))
    edge = got.features >= D - 40 if order == "increasing" else got.features < 40
    assert edge.all()


def test_few_candidates(host):
    D, K = 5, 3
    rng = np.random.default_rng(730)
    post = G.posterior(D, K, rng)
    X = np.zeros((D, 40), np.float32)
    X[[1, 3], 0::2] = 2.0                                                          # points holding 2 features
    X[:, 1::2] = 1.0                                                               # ... and all 5
    for name, data in (("byte", X), ("sparse", sp.csc_matrix(X))):
        got = run_case(host, post, data, 64, 5, ("few", name))
        assert (np.sort(got.features[0::2, :3], 1) == [0, 2, 4]).all() and (got.features[0::2, 3:] == -1).all() and np.isnan(got.prob[0::2, 3:]).all()
        assert (got.features[1::2] == -1).all() and np.isnan(got.prob[1::2]).all() and got.skipped == 0
        got = run_case(host, post, data, 64, 5, ("few, all features", name), exclude=False)
        assert (np.sort(got.features, 1) == np.arange(5)).all()


def test_a_nan_point_is_skipped_and_counted(host):
    D, K, n = 8, 5, 300
    rng = np.random.default_rng(740)
    post = G.posterior(D, K, rng)
    X = G.counts_data(post, n, rng)
    X[2, 17] = np.nan
    X[:, 130] = np.nan
    got = run_case(host, post, X, 128, 3, "NaN points")
    assert got.skipped == 2 and (got.features[[17, 130]] == -1).all() and np.isnan(got.prob[[17, 130]]).all()
    assert (got.features[np.setdiff1d(np.arange(n), [17, 130]), 0] >= 0).sum() > 250


def test_absorb_counts_save_and_load(host, tmp_path):
    D, K, n = 12, 4, 600
    rng = np.random.default_rng(750)
    post = G.separated(D, K)
    counts = rng.integers(50, 500, K).astype(np.float64)
    X = G.counts_data(post, n, rng)
    Y = G.counts_data(post, 300, rng)
    with G.open_predictor(host, post, 256, counts=counts) as p:
        before = check(p, Y, 3, "before absorb")
        p.absorb_counts(X, assign="soft")
        assert p._recommend_set is False
        after = check(p, Y, 3, "after absorb")
        assert not same(before.prob, after.prob)
        with G.open_predictor(host, p.post, 256, counts=p.points_count) as fresh:
            assert same_rec(fresh.recommend(Y, 3), after)
        path = str(tmp_path / "model.npz")
        p.save(path)
    with host.Predictor.load(path, capacity=64) as q:
        assert same_rec(q.recommend(Y, 3), after)
    with pytest.raises(RuntimeError, match="closed"):
        q.recommend(Y, 3)


def test_refusals_come_before_any_launch(pkg, host, binding):
    n, D = 300, 8
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points(rng.poisson(0.8, (n, D)).astype(np.float32))
    views = dict(features=np.full((n, 3), 77, np.int32), prob=np.full((n, 3), 7.0, np.float32), labels=np.full(n, 7, np.int64))

    def refused(code, fn, *a, what=()):
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    theta = np.full((3, D), 1.0 / D)
    refused(-4, wk.recommend_points_into, views, 3)                                # DPMM_ESTATE: no predictive parameters
    assert wk._lib.dpmm_set_recommend(wk._h, theta.ctypes.data_as(binding.ABI_RECOMMEND[0][2][1])) == -4
    wk.set_predictive_mult(*S.mult_params(rng, D, 3))
    refused(-4, wk.recommend_points_into, views, 3, what=("dpmm_set_recommend",))
    assert wk._lib.dpmm_set_recommend(wk._h, None) == -1
    wk.set_recommend(theta)
    for m in (0, 4, 17):                                                           # m = 4: ld = 3 < m
        refused(-1, wk.recommend_points_into, views, m)
    assert (views["features"] == 77).all() and (views["prob"] == 7.0).all() and (views["labels"] == 7).all()      # nothing was written
    assert wk.recommend_points_into(views, 3) == 0 and (views["features"] != 77).all() and (views["labels"] != 7).all()
    wk.set_predictive_mult(*S.mult_params(rng, D, 3))                              # a later set_predictive_* invalidates the table
    refused(-4, wk.recommend_points_into, views, 3, what=("dpmm_set_recommend",))
    bad = torch.empty((n, 3), dtype=torch.float32)                                 # host memory handed to the device variant
    wk.set_recommend(theta)
    with pytest.raises(pkg.DpmmError) as e:
        wk._chk(wk._lib.dpmm_recommend_points_device(wk._h, 3, 1, bad.data_ptr(), bad.data_ptr(), 3, None, None))
    assert e.value.code == -1 and "d_features" in str(e.value)
    wk.close()
    niw = pkg.Worker(pkg.PRIOR_NIW, 2, n, device=0, seed=1)
    assert niw._lib.dpmm_set_recommend(niw._h, theta.ctypes.data_as(binding.ABI_RECOMMEND[0][2][1])) == -1      # DPMM_EINVAL, whatever its state
    niw.close()
    with host.Predictor(_niw_model(), capacity=64) as p:
        with pytest.raises(ValueError, match="regressor"):
            p.recommend(np.zeros((3, 5), np.float32), 1)


def _niw_model():
    """What a Predictor reads of a fitted NIW model (tests/test_rank_cpu.py writes one by hand)."""
    import test_rank_cpu as R
    return R.model(3, 2)


def test_poisoned_lds_and_registers_change_no_bit(host, binding):
    from tools import poison
    poison.build()
    rng = np.random.default_rng(760)
    post = G.posterior(70, 7, rng)
    X = G.counts_data(post, 500, rng)
    Xs = G.sparse_data(70, 500, rng)
    with G.open_predictor(host, post, 256) as p:
        clean = [p.recommend(X, 5), p.recommend(Xs, 5)]
        with poison.poisoned_kernel_launches(binding, 0xffffffff) as launches:
            dirty = [p.recommend(X, 5), p.recommend(Xs, 5)]
        assert launches[0] >= 4
    assert same_rec(clean[0], dirty[0]) and same_rec(clean[1], dirty[1])
