"""GPU tests of include/dpmm_hip_count_explain.h (csrc/count_explain.hip) and of host/score.py's Predictor.explain_counts.

The reference is tests/tools/count_explain_ref.py: the definitions in extended precision on the dense matrix, from the labels and totals
the call itself returns (labels are checked against `predict_labels`, totals against the exact column sums).  For EVERY point of every
case: the residual inside the header's bound, the tail inside the contract of `typicality` (scipy's incomplete beta function for all,
mpmath at 50 digits for a sample of each case), the order, ties to the lower index, no better candidate left out, -1 / NaN exactly behind
the candidates, and the two counters.  Models are made through Predictor._setup from posteriors written by hand, no fit."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_gpu_score as S
import test_gpu_countstats as G
from tools import count_explain_ref as CR

pytestmark = pytest.mark.gpu

DEV = G.DEV
as_np, same = G.as_np, G.same
FIELDS = ("features", "count", "expected", "residual", "feature_tail", "labels", "total")


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


def same_exp(a, b):
    return all(same(getattr(a, f), getattr(b, f)) for f in FIELDS) and (a.skipped, a.incomplete) == (b.skipped, b.incomplete)


def to_np(host, got):
    return host.CountExplanation(*[as_np(getattr(got, f)) for f in FIELDS], got.skipped, got.incomplete)


def check(host, p, X, top, what, side="both", model_X=None, on_device=False, integer=True):
    """One call checked against the reference on the same input; returns the CountExplanation as numpy arrays."""
    Xm = X if model_X is None else model_X
    got = p.explain_counts(X, top, side=side)
    for f in FIELDS:
        a = getattr(got, f)
        assert (isinstance(a, torch.Tensor) and a.device == torch.device(DEV)) if on_device else isinstance(a, np.ndarray), (what, f)
    lab, P = (as_np(a) for a in p.predict(X))
    got = to_np(host, got)
    assert same(got.labels, lab) and same(got.labels, as_np(p.predict_labels(X))), what
    worst = CR.check(got, Xm, CR.theta_of(p.post["alpha"]), top, side, what=what, skip_rows=np.isnan(P).any(1), integer=integer)
    print(what, "top", top, side, "worst ratio to the residual bound, to the tail bound (mpmath sample):", worst)
    return got


def run_case(host, post, X, cap, top, what, side="both", mb=None, binding=None, no_u8=False, **kw):
    with G.open_predictor(host, post, cap, no_u8=no_u8, binding=binding) as p:
        if mb is not None:
            p._wk.set_option(binding.OPT_SCORE_TABLE_MB, mb)
        return check(host, p, X, top, what, side=side, **kw)


def counts_data(post, n, rng, trials=40):
    """(D, n) float32 counts drawn from the clusters, a tenth of the points with one feature pushed far out."""
    X = G.counts_data(post, n, rng, trials=trials)
    out = rng.choice(n, max(1, n // 10), replace=False)
    X[rng.integers(0, X.shape[0], len(out)), out] += rng.integers(5, 60, len(out)).astype(np.float32)
    return X


def sparse_data(D, n, rng, most=200):
    """scipy CSC (D, n): 0 .. `most` entries per point with integer values 1 .. 9; point 0 holds rows 0 and D - 1, point 3 none."""
    cnt = rng.integers(0, min(most, D) + 1, n)
    cnt[0] = min(2, D)
    if n > 3:
        cnt[3] = 0
    rows = [np.sort(rng.choice(D, c, replace=False)) for c in cnt]
    rows[0] = np.array([0, D - 1][:cnt[0]])
    val = [rng.integers(1, 10, c).astype(np.float32) for c in cnt]
    cp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return sp.csc_matrix((np.concatenate(val).astype(np.float32), np.concatenate(rows).astype(np.int64), cp), shape=(D, n))


# ------------------------------------------------------------------------------------------------ one sweep per axis
@pytest.mark.parametrize("D", [2, 33, 64, 65, 1000])
def test_every_dense_D_on_the_byte_store(host, D):
    rng = np.random.default_rng(100 + D)
    post = G.posterior(D, 3, rng)
    X = counts_data(post, 130, rng)
    for side in ("both", "over", "under"):
        got = run_case(host, post, X, 130, min(D, 16), ("byte D", D, side), side=side)
        assert got.skipped == 0 and got.incomplete == 0 and (got.features[:, 0] >= 0).all()
    run_case(host, post, X, 130, 1, ("byte D, top 1", D))


def test_float32_store(host, binding):
    rng = np.random.default_rng(110)
    post = G.posterior(65, 3, rng)
    X = counts_data(post, 130, rng)
    run_case(host, post, X, 130, 16, "Float32 store", no_u8=True, binding=binding)
    run_case(host, post, X * np.float32(0.25), 130, 5, "Float32 store, no integers", no_u8=True, binding=binding, integer=False)


@pytest.mark.parametrize("D", [20000, 65536])
def test_sparse_D(host, D):
    rng = np.random.default_rng(200 + D % 1000)
    post = G.posterior(D, 3, rng)
    X = sparse_data(D, 70, rng)
    for side, top in (("both", 16), ("over", 16), ("under", 1)):
        got = run_case(host, post, X, 70, top, ("sparse D", D, side), side=side)
        assert got.incomplete == int((np.diff(X.indptr) == 0).sum()) >= 1 and got.skipped == 0


@pytest.mark.parametrize("K", [1, 3, 33])
def test_every_K(host, K):
    rng = np.random.default_rng(300 + K)
    post = G.posterior(40, K, rng)
    run_case(host, post, counts_data(post, 200, rng), 200, 5, ("byte K", K))
    run_case(host, post, sparse_data(40, 200, rng, most=12), 200, 5, ("sparse K", K))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_n_across_the_tiles_and_one_point_past_the_capacity(host, n):
    rng = np.random.default_rng(400 + n)
    post = G.posterior(8, 3, rng)
    cap = 128 if n == 129 else n                                                   # n = capacity + 1: a full slab and a short one
    run_case(host, post, counts_data(post, n, rng), cap, 8, ("byte n", n))
    run_case(host, post, sparse_data(8, n, rng, most=8), cap, 3, ("sparse n", n))


# ------------------------------------------------------------------------------------------------ identical bits
def test_capacities_table_budgets_and_stores_give_the_same_bits(host, binding):
    D, K, n = 70, 4, 300
    rng = np.random.default_rng(500)
    post = G.separated(D, K)
    X = counts_data(post, n, rng)
    Xs = sp.csc_matrix(X)
    for side in ("both", "under"):
        outs = {cap: run_case(host, post, X, cap, 7, ("byte capacity", cap), side=side) for cap in (64, 300)}
        assert S.tile_of("mult", D) < n
        outs["ranges"] = run_case(host, post, X, 300, 7, "byte, one-tile ranges", side=side, mb=0.0, binding=binding)
        outs["f32"] = run_case(host, post, X, 300, 7, "Float32 store", side=side, no_u8=True, binding=binding)
        outs["sparse"] = run_case(host, post, Xs, 300, 7, "sparse store", side=side)
        outs["sparse 64"] = run_case(host, post, Xs, 64, 7, "sparse store, capacity 64", side=side)
        for key in (64, "ranges", "f32", "sparse", "sparse 64"):
            assert same_exp(outs[key], outs[300]), (side, key)


def test_every_input_kind_of_one_matrix(host):
    D, K, n = 8, 3, 200
    rng = np.random.default_rng(510)
    post = G.posterior(D, K, rng)
    X = counts_data(post, n, rng)
    Xs = sp.csc_matrix(X)
    emb = torch.from_numpy(X.T.copy()).to(DEV)
    a = run_case(host, post, X, 64, 3, "numpy array")
    b = run_case(host, post, emb.T, 64, 3, "strided device tensor", model_X=X, on_device=True)
    c = run_case(host, post, Xs, 64, 3, "scipy CSC")
    d = run_case(host, post, G.torch_csc(Xs), 64, 3, "torch.sparse_csc on the device", model_X=Xs, on_device=True)
    assert same_exp(a, b) and same_exp(c, d)


def test_pitched_rows_on_the_host_and_on_the_device(host):
    D, K, n, top, ld = 33, 3, 100, 5, 8
    rng = np.random.default_rng(520)
    post = G.posterior(D, K, rng)
    X = counts_data(post, n, rng)
    with G.open_predictor(host, post, n) as p:
        plain = to_np(host, p.explain_counts(X, top))                              # (uploads the points: one full slab)
        for dev in (False, True):
            new = (lambda shape, dt: torch.full(shape, 9, dtype=getattr(torch, dt), device=DEV)) if dev else (lambda shape, dt: np.full(shape, 9, dt))
            views = dict(features=new((n, ld), "int32"), labels=new((n,), "int64"), total=new((n,), "float64"), **{f: new((n, ld), "float32") for f in FIELDS[1:5]})
            assert p._wk.count_explain_points_into(views, top) == (0, 0)
            for f in FIELDS:
                a = as_np(views[f])
                if a.ndim == 2:
                    assert (a[:, top:] == 0).all(), (dev, f)                       # the columns [top, ld) are written as zeros
                    a = a[:, :top]
                assert same(a, getattr(plain, f)), (dev, f)


# ------------------------------------------------------------------------------------------------ named cases
def test_a_uniform_cluster_returns_the_lowest_unseen_indices(host):
    D, n = 300, 40
    post = dict(alpha=np.full((1, D), 2.0, np.float32))                            # theta = 1 / D for every feature: every unseen feature ties
    rng = np.random.default_rng(600)
    X = np.zeros((D, n), np.float32)
    X[:70] = 1.0                                                                   # the first 70 features held: the walk's first 64 positions yield nothing
    for i in range(n):
        X[70 + rng.choice(D - 70, 5, replace=False), i] = 1.0
    for data in (X, sp.csc_matrix(X)):
        got = run_case(host, post, data, n, 16, "uniform alpha'", side="under")
        for i in range(n):
            assert got.features[i].tolist() == np.flatnonzero(X[:, i] == 0)[:16].tolist(), i
        both = run_case(host, post, data, n, 16, "uniform alpha', both sides")
        assert (both.features >= 0).all()


def tie_tables(D, lead, a, b):
    """Tables written by hand for one cluster: features 0 .. lead - 1 share the largest theta, then b, then a < b -- log1p(-theta_b) ONE
    Float64 ulp below log1p(-theta_a), so that both round to one Float32 residual -- then the rest.  In the list b stands at position
    `lead`, a at position lead + 1."""
    th = np.full(D, 0.0)
    th[:lead] = 0.01
    th[[a, b]] = 1.0 / 256
    rest = np.setdiff1d(np.arange(lead, D), [a, b])
    th[rest] = (1.0 - th.sum()) / len(rest)
    assert th[rest[0]] < 1.0 / 256 < 0.01
    lth, l1m = np.log(th[None]), np.log1p(-th[None])
    l1m[0, b] = np.nextafter(l1m[0, a], -np.inf)
    th[b] = -np.expm1(l1m[0, b])
    lth[0, b] = np.log(th[b])
    order = np.argsort(l1m, axis=1, kind="stable").astype(np.int32)
    assert order[0, :lead + 2].tolist() == list(range(lead)) + [b, a]
    return th[None], lth, l1m, order


def test_two_features_one_ulp_apart_across_a_chunk_of_the_sparse_walk(host):
    # the higher index b at list position 63, the last of the walk's first 64 positions, the lower index a at position 64.  Both round to
    # one Float32 residual, so a must come first: a walk that ended when `top` candidates were AT the next position's residual, not
    # strictly above it, would return b.
    D, n, a, b, lead = 200, 20, 100, 150, 63
    th, lth, l1m, order = tie_tables(D, lead, a, b)
    X = np.zeros((D, n), np.float32)
    X[:lead] = 10.0                                                                # the point holds the leading features, a little over their expectation
    t = 10.0 * lead
    r32 = np.sqrt(2 * (t * -l1m[0, [a, b]])).astype(np.float32)
    assert r32[0] == r32[1] and l1m[0, a] != l1m[0, b]
    post = dict(alpha=(th * 4096).astype(np.float32))
    for data in (X, sp.csc_matrix(X)):
        with G.open_predictor(host, post, n) as p:
            p.explain_counts(data, 1)                                              # (uploads the points: one full slab)
            p._wk.set_count_explain(lth, l1m, order)
            for side in ("under", "both"):
                for top in (1, 2, 16):
                    views = dict(features=np.empty((n, top), np.int32), total=np.empty(n), labels=np.empty(n, np.int64),
                                 **{f: np.empty((n, top), np.float32) for f in FIELDS[1:5]})
                    sk, inc = p._wk.count_explain_points_into(views, top, side)
                    got = host.CountExplanation(*[views[f] for f in FIELDS], sk, inc)
                    CR.check(got, X, th, top, side, what=("one ulp apart", lead, side, top), l1m=l1m)
                    assert (views["features"][:, 0] == a).all(), (lead, side, top)          # the lower index first
                    if top > 1:
                        assert (views["features"][:, 1] == b).all()
                        assert (views["residual"][:, 0].view(np.uint32) == views["residual"][:, 1].view(np.uint32)).all()


def test_all_mass_on_one_feature_and_few_candidates(host):
    D, K = 6, 2
    rng = np.random.default_rng(620)
    post = G.posterior(D, K, rng)
    X = np.zeros((D, 30), np.float32)
    X[2] = 9.0                                                                     # all the mass on one feature: x = t
    for data in (X, sp.csc_matrix(X)):
        got = run_case(host, post, data, 30, 6, "all mass on one feature", side="over")
        assert (got.features[:, 0] == 2).all() and (got.features[:, 1:] == -1).all() and np.isnan(got.feature_tail[:, 1:]).all()
        th = CR.theta_of(post["alpha"])[got.labels - 1, 2]
        assert np.allclose(got.feature_tail[:, 0], th ** 9, rtol=2.0 ** -20)
        got = run_case(host, post, data, 30, 6, "all mass on one feature, under", side="under")
        assert (np.sort(got.features[:, :5], 1) == [0, 1, 3, 4, 5]).all() and (got.features[:, 5] == -1).all()


def test_empty_nan_and_negative_points_and_a_nan_row(host, binding):
    D, K, n = 8, 3, 100
    rng = np.random.default_rng(630)
    post = G.posterior(D, K, rng)
    X = counts_data(post, n, rng)
    X[:, 5] = 0.0                                                                  # empty: incomplete
    X[3, 17] = np.nan                                                              # a NaN: its row of the table is NaN, skipped
    X[2, 40] = -1.0                                                                # negative: incomplete (or skipped, if the table says so)
    got = run_case(host, post, X, 64, 3, "NaN, negative, empty", no_u8=True, binding=binding)
    assert got.skipped + got.incomplete == 3 and got.incomplete >= 1
    for i in (5, 17, 40):
        assert (got.features[i] == -1).all() and np.isnan(got.residual[i]).all()
    Xs = sp.csc_matrix((np.array([2.0, np.nan, 1.0, -3.0], np.float32), np.array([1, 4, 2, 6]), np.array([0, 2, 2, 4])), shape=(D, 3))
    got = run_case(host, post, Xs, 3, 3, "sparse NaN, empty, negative")
    assert got.skipped + got.incomplete == 3 and (got.features == -1).all()


def test_after_absorb_counts_the_explanation_follows_the_new_alpha(host):
    D, K = 12, 4
    rng = np.random.default_rng(640)
    post = G.separated(D, K)
    X, Y = G.counts_data(post, 400, rng), counts_data(post, 150, rng)
    with G.open_predictor(host, post, 128, counts=rng.integers(50, 500, K).astype(np.float64)) as p:
        before = check(host, p, Y, 3, "before absorb")
        p.absorb_counts(X, assign="soft")
        assert p._count_explain_set is False
        after = check(host, p, Y, 3, "after absorb")                               # against the NEW alpha'
        assert not same(before.expected, after.expected)
        with G.open_predictor(host, p.post, 128, counts=p.points_count) as fresh:
            assert same_exp(to_np(host, fresh.explain_counts(Y, 3)), after)


def test_refusals_come_before_any_launch(pkg, host, binding):
    n, D = 100, 8
    rng = np.random.default_rng(3)
    wk = pkg.Worker(pkg.PRIOR_MULT, D, n, device=0, seed=1)
    wk.upload_points(rng.poisson(0.8, (n, D)).astype(np.float32))
    views = dict(features=np.full((n, 3), 77, np.int32), total=np.full(n, 7.0), labels=np.full(n, 7, np.int64), **{f: np.full((n, 3), 7.0, np.float32) for f in FIELDS[1:5]})

    def refused(code, fn, *a, what=()):
        with pytest.raises(pkg.DpmmError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)
        for w in what:
            assert w in str(e.value), str(e.value)

    th = np.full((3, D), 1.0 / D)
    tables = (np.log(th), np.log1p(-th), np.tile(np.arange(D, dtype=np.int32), (3, 1)))
    refused(-4, wk.count_explain_points_into, views, 3)                            # DPMM_ESTATE: no predictive parameters
    wk.set_predictive_mult(*S.mult_params(rng, D, 3))
    refused(-4, wk.count_explain_points_into, views, 3, what=("dpmm_set_count_explain",))
    refused(-1, wk.set_count_explain, tables[0], tables[1], tables[2][:, ::-1])    # ties must come in increasing index order
    refused(-1, wk.set_count_explain, tables[0], tables[1], np.zeros((3, D), np.int32), what=("permutation",))
    refused(-1, wk.set_count_explain, -tables[0], tables[1], tables[2])
    wk.set_count_explain(*tables)
    for top in (0, 4, 17):                                                         # top = 4: ld = 3 < top
        refused(-1, wk.count_explain_points_into, views, top)
    assert (views["features"] == 77).all() and (views["residual"] == 7.0).all() and (views["labels"] == 7).all()      # nothing was written
    sk, inc = wk.count_explain_points_into(views, 3)
    assert sk == 0 and (views["labels"] != 7).all()
    wk.set_predictive_mult(*S.mult_params(rng, D, 3))                              # a later set_predictive_* invalidates the tables
    refused(-4, wk.count_explain_points_into, views, 3, what=("dpmm_set_count_explain",))
    wk.close()
    niw = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    ptr = [a.ctypes.data_as(t) for a, t in zip(tables, binding.ABI_COUNT_EXPLAIN[0][2][1:])]
    assert niw._lib.dpmm_set_count_explain(niw._h, *ptr) == -1                     # DPMM_EINVAL, whatever its state
    niw.close()
    import test_rank_cpu as R
    with host.Predictor(R.model(3, 2), capacity=64) as p:
        with pytest.raises(ValueError, match="Multinomial"):
            p.explain_counts(np.zeros((3, 5), np.float32), 1)


# ------------------------------------------------------------------------------------------------ the law, on the GPU's own draws
def test_tails_of_points_drawn_from_the_model_are_conservative(host):
    D, K, n = 8, 3, 20000
    post = G.separated(D, K)
    with G.open_predictor(host, post, n) as p:
        X, _ = p.sample(n, seed=5, trials=60)
        got = p.explain_counts(X, D)
    tail = as_np(got.feature_tail)
    ok = ~np.isnan(tail)
    share, N = float((tail[ok] < 0.01).mean()), int(ok.sum())
    # a one-sided discrete tail is conservative: P(tail < a) <= a on each side; the features of a point are dependent, so the band is that
    # of n points, not of n D entries
    assert N > n * D // 2 and share <= 0.01 + 3 * np.sqrt(0.01 * 0.99 / n), (share, N)
