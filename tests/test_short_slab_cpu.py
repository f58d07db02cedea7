"""The short-slab rule of the Python point calls (host/score.py, `Predictor._walk`) over a stand-in worker, no GPU: a short last slab is
zero padded to `capacity`, the worker scores the padding too, and the walk takes the padding that took no part off `skipped`.  Here the
padding itself takes no part -- the stand-in drops every row whose first value is 0 -- which no GPU model does: the branch no GPU test
reaches.  For the eight calls with a closure of their own: the counters are those of the real rows, the outputs the stand-in's values row
for row, and the worker is called once per slab with `capacity` rows."""
import importlib

import numpy as np
import pytest

from __graft_entry__ import load_package
from fake_worker import FakeWorker
from tools import regress_ref as rr

CAP = 8
SIZES = [0, 1, 7, 8, 9, 19]
ABSENT = (0, 6, 8, 18)            # first value 0: took no part -- in the first slab, the second, the short one (n = 9, 19)
INCOMPLETE = (3, 10)              # first value < 0: incomplete (typicality, explain), never the padding
LEVELS = (0.25, 0.5, 0.75)
SEED = 5


@pytest.fixture(scope="module")
def score():
    return importlib.import_module(load_package().__name__ + ".host.score")


def points(n, D):
    """(D, n): first value 1 (0: takes no part, -1: incomplete), second value i + 1/2, the row's name; the others i + d."""
    X = (np.arange(n, dtype=np.float32)[None, :] + np.arange(D, dtype=np.float32)[:, None])
    X[0] = 1.0
    X[0, [i for i in ABSENT if i < n]] = 0.0
    X[0, [i for i in INCOMPLETE if i < n]] = -1.0
    X[1] = np.arange(n, dtype=np.float32) + 0.5
    return X


# ---- what the stand-in answers, from the rows (m, D) it holds: the same functions give the expectation from all n rows at once
def part(X):
    return X[:, 0] != 0


def label(X):
    return (2 * X[:, 1]).astype(np.int64)


def column(X, base, width, keep):
    """(m, width) float32: name + base + d, NaN where `keep` is false."""
    out = (X[:, 1:2] + np.float32(base) + np.arange(width, dtype=np.float32)[None, :]).astype(np.float32)
    out[~keep] = np.nan
    return out


class StandIn(FakeWorker):
    """Every `*_into` call a Predictor or a Regressor makes, answered from the rows in place; `seen`: (call, rows held, rows of the output)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def set_predictive_niw(self, *a):
        pass

    def set_predictive_mult(self, *a):
        pass

    def set_option(self, *a):
        pass

    def set_recommend(self, theta):
        pass

    def set_regression(self, B, c, V, h):
        self.Dt = c.shape[1]

    def set_regression_factor(self, W):
        pass

    def set_regression_levels(self, levels, z):
        self.levels = np.array(levels, np.float32)

    def score_missing_counts(self):
        return 0, 0

    def note(self, call, out):
        assert self.X.shape == (self.n, self.D) and len(out) == self.n, call
        self.seen.append((call, self.X.shape[0], len(out)))

    def score_points_into(self, outs, m=0):
        outs["labels"][:] = label(self.X)

    def typicality_points_into(self, outs):
        self.note("typicality", outs["labels"])
        X = self.X
        scored = part(X) & (X[:, 0] > 0)
        outs["labels"][:] = label(X)
        outs["mahalanobis"][:] = column(X, 3, 1, scored)[:, 0]
        outs["tail"][:] = column(X, 4, 1, scored)[:, 0]
        return int((~part(X)).sum()), int((X[:, 0] < 0).sum())

    def explain_points_into(self, outs, top=0):
        sk, inc = self.typicality_points_into({k: outs[k] for k in ("labels", "mahalanobis", "tail")})
        self.seen[-1] = ("explain",) + self.seen[-1][1:]
        scored = part(self.X) & (self.X[:, 0] > 0)
        for j, name in enumerate(("residual", "zscore", "feature_tail")):
            outs[name][:] = column(self.X, 10 * (j + 1), outs[name].shape[1], scored)
        if top:
            outs["features"][:] = np.where(scored[:, None], np.arange(top)[None, :], -1)
        return sk, inc

    def recommend_points_into(self, views, m, exclude_seen=True):
        self.note("recommend", views["labels"])
        keep = part(self.X)
        views["features"][:] = np.where(keep[:, None], np.arange(m)[None, :], -1)
        views["prob"][:] = column(self.X, 1, m, keep)
        views["labels"][:] = label(self.X)
        return int((~keep).sum())

    def regress_points_into(self, mean, std=None, labels=None):
        self.note("predict", mean)
        keep = part(self.X)
        mean[:] = column(self.X, 1, self.Dt, keep)
        if std is not None:
            std[:] = column(self.X, 2, self.Dt, keep)
        labels[:] = label(self.X)
        return int((~keep).sum())

    def draws(self, out, seed, i0, comp, keep):
        real = self.X[:, 1] != 0                                           # (the padding has no name)
        assert np.array_equal(self.X[real, 1] - 0.5, i0 + np.flatnonzero(real))      # the global index of a point is its position in the data
        for j in range(out.shape[1]):
            out[:, j] = column(self.X, 100 * j + seed, out.shape[2], keep)
            if comp is not None:
                comp[j] = np.where(keep, j, -1)

    def regress_draw_points_into(self, out, seed, i0, draw0=0, comp=None):
        self.note("sample", out)
        assert comp is not None and comp.shape == (out.shape[1], self.n)
        self.draws(out, seed, i0, comp, part(self.X))
        return int((~part(self.X)).sum())

    def impute_draws_into(self, out, seed, i0, draw0=0, comp=None):
        self.note("impute", out)
        self.draws(out, seed, i0, comp, part(self.X))

    def regress_cdf_points_into(self, y, cdf, sf=None, labels=None):
        self.note("cdf", cdf)
        assert y.dtype == np.float32 and y.shape == cdf.shape and not y[self.X[:, 1] == 0].any()      # zeros behind the slab's points
        keep = part(self.X)
        cdf[:] = np.where(keep[:, None], y + self.X[:, 1:2], np.nan)
        sf[:] = np.where(keep[:, None], y - self.X[:, 1:2], np.nan)
        labels[:] = label(self.X)
        return int((~keep).sum())

    def regress_quantile_points_into(self, out, labels=None):
        self.note("quantile", out)
        keep = part(self.X)
        for q, lv in enumerate(self.levels):
            out[:, q] = column(self.X, lv, self.Dt, keep)
        labels[:] = label(self.X)
        return int((~keep).sum())


def open_niw(score):
    post, _ = rr.make_posterior(4, 3, 11)
    return score.Predictor(rr.dummy_model(post, 3, 4), capacity=CAP, worker_factory=StandIn)


def open_regressor(score):
    parent = open_niw(score)
    return parent, parent.regressor([0, 1, 2], [3], worker_factory=StandIn)


def open_mult(score):
    p = score.Predictor.__new__(score.Predictor)
    p._setup(1, 5, 10.0, np.full(3, 20.0), dict(alpha=np.ones((3, 5), np.float32)), CAP, 0, StandIn)
    return p


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def walked(wk, call, n):
    """One call per slab, `capacity` rows in and out each time."""
    return [s for s in wk.seen if s[0] == call] == [(call, CAP, CAP)] * -(-n // CAP)


def absent(n):
    return sum(i < n for i in ABSENT)


@pytest.mark.parametrize("n", SIZES)
def test_typicality_and_explain(score, n):
    X = points(n, 4)
    R = X.T
    scored = part(R) & (R[:, 0] > 0)
    with open_niw(score) as p:
        t = p.typicality(X)
        assert (t.skipped, t.incomplete) == (absent(n), sum(i < n for i in INCOMPLETE)) and isinstance(t.skipped, int)
        assert same(t.labels, label(R)) and same(t.mahalanobis, column(R, 3, 1, scored)[:, 0]) and same(t.tail, column(R, 4, 1, scored)[:, 0])
        assert walked(p._wk, "typicality", n)
        for top in (None, 2):
            p._wk.seen.clear()
            e = p.explain(X, top=top)
            assert (e.skipped, e.incomplete) == (t.skipped, t.incomplete)
            assert same(e.labels, t.labels) and same(e.mahalanobis, t.mahalanobis) and same(e.tail, t.tail)
            for j, rows in enumerate((e.residual, e.zscore, e.feature_tail)):
                want = column(R, 10 * (j + 1), top or 4, scored)
                assert same(rows, want if top else want.T), (top, j)
            assert e.features is None if top is None else same(e.features, np.where(scored[:, None], np.arange(top)[None, :], -1).astype(np.int32))
            assert walked(p._wk, "explain", n)


@pytest.mark.parametrize("n", SIZES)
def test_recommend(score, n):
    X = points(n, 5)
    R = X.T
    with open_mult(score) as p:
        r = p.recommend(X, 2)
        assert r.skipped == absent(n) and isinstance(r.skipped, int)
        assert same(r.features, np.where(part(R)[:, None], np.arange(2)[None, :], -1).astype(np.int32))
        assert same(r.prob, column(R, 1, 2, part(R))) and same(r.labels, label(R))
        assert walked(p._wk, "recommend", n)


@pytest.mark.parametrize("n", SIZES)
def test_regressor_calls(score, n):
    X = points(n, 3)
    R = X.T
    keep = part(R)
    y = (np.arange(n, dtype=np.float64)[None, :] * 0.125 + 1.0)
    parent, reg = open_regressor(score)
    with parent, reg:
        wk = reg.marginal._wk
        got = reg.predict(X, return_std=True)
        assert got.skipped == absent(n) and isinstance(got.skipped, int)
        assert same(got.mean, column(R, 1, 1, keep).T) and same(got.std, column(R, 2, 1, keep).T) and same(got.labels, label(R))
        assert walked(wk, "predict", n)

        for components in (False, True):
            wk.seen.clear()
            got = reg.sample(X, draws=2, seed=SEED, return_components=components)
            assert got.skipped == absent(n) and isinstance(got.skipped, int)
            assert same(got.values, np.stack([column(R, 100 * j + SEED, 1, keep).T for j in range(2)])) and same(got.labels, label(R))
            assert got.components is None if not components else same(got.components, np.stack([np.where(keep, j, -1) for j in range(2)]).astype(np.int32))
            assert walked(wk, "sample", n)

        got = reg.cdf(X, y)
        y32 = y.T.astype(np.float32)
        assert got.skipped == absent(n) and isinstance(got.skipped, int)
        assert same(got.cdf, np.where(keep[:, None], y32 + R[:, 1:2], np.nan).astype(np.float32).T)
        assert same(got.sf, np.where(keep[:, None], y32 - R[:, 1:2], np.nan).astype(np.float32).T) and same(got.labels, label(R))
        assert walked(wk, "cdf", n)

        got = reg.quantile(X, LEVELS)
        assert got.skipped == absent(n) and isinstance(got.skipped, int)
        assert same(got.values, np.stack([column(R, np.float32(lv), 1, keep).T for lv in LEVELS])) and same(got.labels, label(R))
        assert walked(wk, "quantile", n)


@pytest.mark.parametrize("n", SIZES)
def test_impute_draws(score, n):
    X = points(n, 4)
    R = X.T
    keep = part(R)
    with open_niw(score) as p:
        for components in (False, True):
            p._wk.seen.clear()
            got = p.impute(X, draws=2, seed=SEED, return_components=components)
            vals, comp = got if components else (got, None)
            assert same(vals, np.stack([column(R, 100 * j + SEED, 4, keep).T for j in range(2)]))
            assert comp is None or same(comp, np.stack([np.where(keep, j, -1) for j in range(2)]).astype(np.int32))
            assert walked(p._wk, "impute", n) and p.missing_counts == (0, 0)
