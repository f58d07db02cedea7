"""GPU tests of include/dpmm_hip_explain.h (csrc/explain.hip) and of host/score.py's Predictor.explain.

The reference is numpy Float64 (tests/tools/explain_ref.py) from the Float32 m, R, df the worker is given.  Models are made through
Predictor._setup from posteriors written by hand (tests/tools/sample_ref.py's niw_model), no fit.  Shapes (D, K, n): (1, 2, 130),
(2, 3, 300), (17, 3, 300), (64, 2, 257), (65, 2, 200), (130, 2, 130), (256, 2, 70), each at df = D + 3 and df = 1e5: every NT instantiation
of the kernel, the tile edge r = 63 / 64 of miss_rty, a partial last wave of a workgroup, a short last slab (capacity 64).  With u = 2^-24
and b_d, dg, dq, h as the header defines them:

  residual      |e_d - ref| <= (2 D + 6) u b_d / A_dd
  zscore        |t_d - ref| <= 2 (sqrt((df + D - 1) / (A_dd h)) dg + |t_d| / (2 h) (dq + 2 |g_d| dg / A_dd) + 16 u |t_d|)
  feature_tail  against 2 t.sf(|t_d|, df + D - 1) in Float64 on the RETURNED t_d: relative 2^-20 (the allowance tests/test_gpu_typicality.py
                uses for `tail`) wherever the reference is at least 1e-30; both at most 1e-29 below.

The collapse at D = 1 (check 3) is asserted on EVERY scored point with the bounds include/dpmm_hip_explain.h derives ("One feature"):
with E = (11 + 6 q / df) u and B = E (1 + E),
  |zscore^2 / mahalanobis - 1| <= B                                    (eleven roundings, and q - s cancels where h damps it by df only)
  |feature_tail - tail| / tail <= exp(S B) - 1 + 2 u + 2e-9            S = |d log tail / d log q| of the Float64 reference at q (1 + B),
                                                                        wherever the tail is at least 1e-30; both at most 1e-29 below
and, as the issue states it, within 8 ulp and within the tail allowance 2^-20 on the points where those follow from the bounds: q <= df / 8
for the first (the cancellation is below one u there) and q <= min(df / 8, 1) for the second (S <= 0.76).  Measured on an MI355X: at
df = 4 2.8 ulp at most on the 66 points with q <= df / 8 and 259 ulp (tails 64 2^-20 apart) at q / df = 464, where B allows 2800 u; at
df = 1e5 2.9 ulp on all 130 points and tails up to 2.75 2^-20 apart."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_score as S
from tools import explain_ref as E
from tools import sample_ref as SR
from tools import typicality_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 2, 130), (2, 3, 300), (17, 3, 300), (64, 2, 257), (65, 2, 200), (130, 2, 130), (256, 2, 70)]
TAIL_REL = 2.0 ** -20
ROWS = ("residual", "zscore", "feature_tail")


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


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(a, b):
    """Equal shapes, types and bits (None equals None)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(as_np(a)), np.ascontiguousarray(as_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_exp(a, b):
    return all(same(x, y) for x, y in zip(a[:7], b[:7])) and a[7:] == b[7:]


def model(D, K, df, seed):
    """(post, m, A, df): the cluster centres are spread so that most points keep the cluster they were drawn from."""
    post, m, A, df = SR.niw_model(D, K, df, seed)
    post["m"] = m = (m * 4.0).astype(np.float32).astype(np.float64)
    return post, m, A, df


def open_predictor(host, post, cap, **kw):
    K, D = post["m"].shape
    p = host.Predictor.__new__(host.Predictor)
    p._setup(0, D, 10.0, np.full(K, 100.0), post, cap, 0, None, **kw)
    return p


def points(m, A, n, rng):
    """(D, n) Float32: the K centres first, then normal draws around the centres scaled by 0.3 .. 20 (near points and far ones: tails down
    to nothing), in an order that mixes the clusters."""
    K, D = m.shape
    z = rng.integers(0, K, n - K)
    scale = rng.choice([0.3, 1.0, 1.0, 1.0, 3.0, 20.0], n - K)
    x = m[z] + scale[:, None] * np.einsum("nij,nj->ni", A[z], rng.standard_normal((n - K, D)))
    return np.concatenate([m, x]).T.astype(np.float32)


def worker_params(p):
    which, (m, R, logdet, df, w) = p._predictive_args()
    return T.worker_params(m, R, df)


def check_rows(got, X, params, what):
    """Check 2 on a full (top=None) result; returns the scored mask."""
    lab, q = as_np(got.labels), as_np(got.mahalanobis)
    e, t, ft = (as_np(getattr(got, name)) for name in ROWS)
    D, n = X.shape
    assert got.features is None and all(a.dtype == np.float32 and a.shape == (D, n) for a in (e, t, ft)), what
    ok = ~np.isnan(q)
    assert int((~ok).sum()) == got.skipped + got.incomplete, what
    assert all(np.isnan(a[:, ~ok]).all() and not np.isnan(a[:, ok]).any() for a in (e, t, ft)), what
    ref = E.reference(X[:, ok], lab[ok] - 1, *params)
    e, t, ft = (a[:, ok].T.astype(np.float64) for a in (e, t, ft))
    re_, rt = np.abs(e - ref.e) / np.maximum(ref.e_bound, 1e-300), np.abs(t - ref.t) / np.maximum(2 * ref.t_bound, 1e-300)
    print(what, "D", D, "largest error in units of its bound: residual", float(re_.max()), "zscore (twice the first-order bound)", float(rt.max()))
    assert np.all(np.abs(e - ref.e) <= ref.e_bound) and np.all(np.abs(t - ref.t) <= 2 * ref.t_bound), what
    dof = (params[2].astype(np.float64)[lab[ok] - 1] + D - 1)[:, None]
    tr = E.feature_tail_of(t, dof)                                                                       # of the RETURNED zscore
    big = tr >= 1e-30
    rel = np.abs(ft[big] - tr[big]) / tr[big]
    print(what, "largest relative feature_tail error in units of 2^-20:", float(rel.max() * 2 ** 20), "tails below 1e-30:", int((~big).sum()))
    assert np.all(rel <= TAIL_REL) and np.all(ft[~big] <= 1e-29) and np.all(tr[~big] <= 1e-29) and np.all((ft >= 0) & (ft <= 1)), what
    assert np.all(ft[t == 0] == 1.0), what
    return ok


def check_top(full, top, m, what):
    """Check 4: the m features of largest |zscore| of the full result, in the order of a stable argsort, and the same bits gathered."""
    t = as_np(full.zscore)                                                                               # (D, n)
    n = t.shape[1]
    feats = as_np(top.features)
    assert feats.dtype == np.int32 and feats.shape == (n, m) and all(as_np(getattr(top, name)).shape == (n, m) for name in ROWS), what
    ok = ~np.isnan(as_np(full.mahalanobis))
    want = np.argsort(-np.abs(t.T), axis=1, kind="stable")[:, :m]                                        # (NaN sorts last)
    assert np.array_equal(feats[ok], want[ok]) and np.all(feats[~ok] == -1), what
    for name in ROWS:
        a, b = as_np(getattr(full, name)).T, as_np(getattr(top, name))
        assert same(np.take_along_axis(a[ok], want[ok], 1), b[ok]) and np.isnan(b[~ok]).all(), (what, name)
    assert all(same(x, y) for x, y in zip(full[:3], top[:3])) and full[7:] == top[7:], what


# ------------------------------------------------------------------------------------------------ every shape
@pytest.mark.parametrize("heavy", [True, False], ids=["df=D+3", "df=1e5"])
@pytest.mark.parametrize("D,K,n", SHAPES)
def test_every_shape(host, binding, D, K, n, heavy):
    rng = np.random.default_rng(1000 * D + K + heavy)
    post, m, A, df = model(D, K, D + 3.0 if heavy else 1e5, 7 * D + K)
    X = points(m, A, n, rng)
    what = ("D", D, "df", float(df[0]))
    with open_predictor(host, post, 64) as p:                                                            # a short last slab: n is no multiple of 64
        params = worker_params(p)
        typ = p.typicality(X)
        full = p.explain(X)
        assert all(same(x, y) for x, y in zip(full[:3], typ[:3])) and full[7:] == typ[3:] == (0, 0)      # 1: typicality's values, to the bit
        ok = check_rows(full, X, params, what)                                                           # 2
        assert ok.all()
        lab, t, ft = as_np(full.labels), as_np(full.zscore), as_np(full.feature_tail)
        own = lab[:K] == np.arange(1, K + 1)                                                             # the centres that keep their label
        assert own.sum() >= 1 and np.all(t[:, :K][:, own] == 0) and np.all(ft[:, :K][:, own] == 1)
        tops = {mm: p.explain(X, top=mm) for mm in sorted({1, min(3, D), min(D, 16)})}                   # 4
        for mm, top in tops.items():
            check_top(full, top, mm, what + ("top", mm))
        xd = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV).T                                       # 5: a device tensor, full slabs read in place
        dfull, dtop = p.explain(xd), p.explain(xd, top=min(D, 16))
        assert all(torch.is_tensor(v) and v.device == torch.device(DEV) for v in dfull[:6] + dtop[:7])
        assert same_exp(full, dfull) and same_exp(tops[min(D, 16)], dtop)
    with open_predictor(host, post, n + 7) as p:                                                         # 5: one slab; then ranges of one tile
        one = p.explain(X)
        p._wk.set_option(binding.OPT_SCORE_TABLE_MB, 0.0)
        ranges, rtop = p.explain(X), p.explain(X, top=1)
    assert same_exp(full, one) and same_exp(full, ranges) and same_exp(tops[1], rtop)
    if D == 1:                                                                                           # 3: the collapse t^2 = q, feature_tail = tail
        q, tail = as_np(full.mahalanobis).astype(np.float64), as_np(full.tail).astype(np.float64)
        t2 = t[0].astype(np.float64) ** 2                                                                # (exact)
        ulps = np.abs(t2 - q) / np.spacing(as_np(full.mahalanobis)).astype(np.float64)
        from scipy.stats import t as student
        u = 2.0 ** -24
        Eb = (11 + 6 * q / df[0]) * u
        B = Eb * (1 + Eb)                                                                                # the header's bound on |t^2 / q - 1|
        pos = q > 0
        ratio = np.abs(t2[pos] / q[pos] - 1)
        tt = np.sqrt(q * (1 + B))
        ref = 2 * student.sf(np.sqrt(q), df[0])
        big = ref >= 1e-30
        Sq = np.where(big, tt * student.pdf(tt, df[0]) / np.maximum(2 * student.sf(tt, df[0]), 1e-300), 0.0)
        tail_bound = np.expm1(Sq * B) + 2 * u + 2e-9
        rel = np.abs(ft[0].astype(np.float64) - tail) / np.maximum(tail, 1e-300)
        near = q <= df[0] / 8                                                                            # the cancellation of q - s is below one u
        flat = near & (q <= 1)                                                                           # S <= 0.76: 8 ulp of q move the tail by less than 2^-20
        print(what, "D = 1: largest |zscore^2 / q - 1| in units of its bound:", float((ratio / B[pos]).max()), "largest |feature_tail - tail| / tail in units of its bound:",
              float((rel[big] / tail_bound[big]).max()), "; largest q / df", float((q / df[0]).max()), "largest S", float(Sq.max()), "tails below 1e-30:", int((~big).sum()))
        print(what, "D = 1,", int(near.sum()), "points with q <= df / 8: in ulp", float(ulps[near].max()), ";", int(flat.sum()), "with q <= 1 too: tails apart in units of 2^-20",
              float(rel[flat].max() * 2 ** 20), "; all points: in ulp", float(ulps.max()), "in units of 2^-20", float(rel[big].max() * 2 ** 20))
        assert np.all(t2[~pos] == 0) and np.all(ratio <= B[pos])                                         # every point
        assert np.all(rel[big] <= tail_bound[big]) and np.all(ft[0][~big] <= 1e-29) and np.all(tail[~big] <= 1e-29)
        assert flat.sum() >= 20 and np.all(ulps[near] <= 8) and np.all(rel[flat] <= TAIL_REL)            # the issue's figures where the bounds imply them


# ------------------------------------------------------------------------------------------------ the classes
def test_skipped_and_incomplete_points(host):
    D, K, n = 6, 3, 300
    rng = np.random.default_rng(7)
    post, m, A, df = model(D, K, 9.0, 70)
    X = points(m, A, n, rng)
    clean = X.copy()
    X[0, 7] = np.nan                                                                                     # one gap
    X[2, 250] = np.nan
    X[1, 100] = np.inf                                                                                   # no finite entry in its row
    X[:, 290] = np.nan                                                                                   # nothing left to marginalise over
    gaps, lost = [7, 250], [100, 290]
    rest = np.setdiff1d(np.arange(n), gaps + lost)
    for missing, counts in (("propagate", (len(gaps) + len(lost), 0)), ("marginalize", (len(lost), len(gaps)))):
        with open_predictor(host, post, 64, missing=missing) as p:
            base = p.explain(clean)
            got, top = p.explain(X), p.explain(X, top=2)
            typ = p.typicality(X)
            assert (got.skipped, got.incomplete) == counts == (top.skipped, top.incomplete) == typ[3:], missing      # exact counters
            assert all(same(x, y) for x, y in zip(got[:3], typ[:3])), missing
            for name in ROWS:
                a, b, c = as_np(getattr(got, name)), as_np(getattr(top, name)), as_np(getattr(base, name))
                assert np.isnan(a[:, gaps + lost]).all() and np.isnan(b[gaps + lost]).all(), (missing, name)
                assert same(a[:, rest], c[:, rest]), (missing, name)                                     # every other point untouched
            assert np.all(as_np(top.features)[gaps + lost] == -1) and np.all(as_np(top.features)[rest] >= 0), missing
            check_top(got, top, 2, missing)
            if missing == "marginalize":
                assert np.all(as_np(got.labels)[gaps] >= 1)                                              # the gap points are labelled


# ------------------------------------------------------------------------------------------------ the case the feature exists for
def test_planted_cause_in_a_correlated_cluster(host):
    """One cluster, D = 17, correlation 0.99 between features 0 and 1.  Point j is the centre with feature j moved by 12 conditional
    standard deviations (at the centre q_-j = 0: delta = 12 / sqrt(A_jj (df + D - 1) / df)).  explain(top=1) names j for every j; for
    j in {0, 1} the marginal z-score of the moved feature is below 2."""
    D, df, rho = 17, 50.0, 0.99
    Sigma = np.eye(D)
    Sigma[0, 1] = Sigma[1, 0] = rho
    A = np.linalg.cholesky(Sigma[::-1, ::-1])[::-1, ::-1]                                                # upper triangular, A A' = Sigma
    assert np.allclose(A @ A.T, Sigma) and np.allclose(A, np.triu(A))
    kappa, nu = 5.0, df + D - 1
    c = (kappa + 1) / (kappa * df)
    m = np.linspace(-1, 1, D).astype(np.float32).astype(np.float64)[None]
    post = dict(kappa=np.array([kappa]), nu=np.array([nu]), m=m, U=(A / np.sqrt(c))[None])
    prec = np.linalg.inv(Sigma)
    delta = 12.0 / np.sqrt(np.diag(prec) * (df + D - 1) / df)
    X = (m[0][:, None] + np.diag(delta)).astype(np.float32)                                              # column j: feature j moved
    marginal = delta / np.sqrt(np.diag(Sigma))
    assert marginal[0] < 2 and marginal[1] < 2
    with open_predictor(host, post, 64) as p:
        got = p.explain(X, top=1)
        full = p.explain(X)
    feats, t = as_np(got.features)[:, 0], as_np(got.zscore)[:, 0]
    print("planted: features", feats.tolist(), "zscores", np.round(t, 3).tolist(), "marginal z of features 0, 1:", marginal[:2].round(3).tolist())
    assert np.array_equal(feats, np.arange(D)) and np.allclose(t, 12.0, rtol=1e-3)
    assert np.all(as_np(got.feature_tail)[:, 0] < 1e-12) and np.all(as_np(full.feature_tail)[:2, 2:] > 0.5)      # features 0, 1 of the other points are ordinary


# ------------------------------------------------------------------------------------------------ through a projection
def test_projected_data_is_explained_in_the_projected_space(host):
    D, K, n, D_in = 8, 3, 300, 40
    rng = np.random.default_rng(6)
    post, m, A, df = model(D, K, 11.0, 60)
    X = points(m, A, n, rng)
    proj = host.random_projection(D_in, D, seed=3)
    Xs = (proj.basis @ X.astype(np.float64)).astype(np.float32)                                          # (D_in, n) source rows
    Z = as_np(proj.transform(Xs))                                                                        # the coordinates the worker computes
    with open_predictor(host, post, 64, projection=proj) as p:
        a, b = p.explain(Xs), p.explain(Z)
        top = p.explain(Xs, top=3)
        assert same_exp(a, b) and as_np(a.zscore).shape == (D, n)
        check_rows(a, Z, worker_params(p), "projected")
        check_top(a, top, 3, "projected")
        assert as_np(top.features).max() < D


# ------------------------------------------------------------------------------------------------ the one-shot call and the raw rows
def test_one_shot_explain_equals_the_predictor(host):
    """explain(dp_model, data, top, **kw) over a fitted model's surface (sampler.post with three rows per cluster, prior, alpha, counts)."""
    import types
    D, K, n = 5, 3, 200
    rng = np.random.default_rng(11)
    post, m, A, df = model(D, K, 8.0, 110)
    X = points(m, A, n, rng)
    X[3, 17] = np.nan
    post3 = {k: np.repeat(np.asarray(v), 3, axis=0) for k, v in post.items()}                            # rows 3k: the clusters
    sampler = types.SimpleNamespace(K=K, post=post3, prior=types.SimpleNamespace(kind=0, dim=D), alpha=10.0, points_count=np.full(K, 100.0))
    dp_model = types.SimpleNamespace(sampler=sampler)
    for kw in (dict(), dict(missing="marginalize")):
        with open_predictor(host, post, 64, **kw) as p:
            want, wtop = p.explain(X), p.explain(X, top=2)
        got, gtop = host.explain(dp_model, X, capacity=64, device=0, **kw), host.explain(dp_model, X, top=2, capacity=96, device=0, **kw)
        assert same_exp(want, got) and same_exp(wtop, gtop), kw
        assert (got.skipped, got.incomplete) == ((0, 1) if kw else (1, 0))


def test_host_rows_wider_than_their_content_keep_the_words_behind(pkg):
    """dpmm_explain_points with ld > top and ld > D: the first entries of a row are those of the dense call, the words behind are not touched."""
    D, K, n, ld = 5, 3, 300, 9
    rng = np.random.default_rng(12)
    wk = pkg.Worker(pkg.PRIOR_NIW, D, n, device=0, seed=1)
    wk.upload_points(rng.standard_normal((n, D)).astype(np.float32))
    wk.set_predictive_niw(*S.niw_params(rng, D, K))
    for top, width in ((0, D), (2, 2)):
        dense = {name: np.empty((n, width), np.float32) for name in ROWS}
        wide = {name: np.full((n, ld), -7.0, np.float32) for name in ROWS}
        if top:
            dense["features"], wide["features"] = np.empty((n, width), np.int32), np.full((n, ld), -7, np.int32)
        assert wk.explain_points_into(dense, top=top) == wk.explain_points_into(wide, top=top) == (0, 0)
        for name in dense:
            assert same(dense[name], wide[name][:, :width]) and np.all(wide[name][:, width:] == -7), (top, name)
    wk.close()
