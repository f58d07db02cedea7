"""numpy Float64 reference of include/dpmm_hip_recommend.h: the next-count probabilities r*_id = sum_k p_ik theta_kd of a Multinomial
mixture, the header's bound and a checker of what `Predictor.recommend` returns.

  exact(P, theta)                       r* (n, D) float64 from the Float32 probabilities `predict` returns and the Float64 theta
  eps(K)                                (K + 2) 2^-24: theta rounded once, a chain of K steps, one inner sum -- every term non-negative
  topm(r, seen, m)                      the definition on given values: (features (n, m) int32, values (n, m)) by (r descending, feature
                                        ascending) over the candidates, -1 / NaN behind them
  check(features, prob, ...)            every property the header states, for every point; returns the largest |prob - r*| / (eps r*)
"""
import numpy as np


def theta_of(alpha):
    a = np.asarray(alpha, np.float64)
    return a / a.sum(1, keepdims=True)


def exact(P, theta):
    return np.asarray(P, np.float32).astype(np.float64) @ np.asarray(theta, np.float64)


def eps(K):
    return (K + 2) * 2.0 ** -24


def seen_of(X):
    """(n, D) bool from (D, n) data: dense array or scipy sparse (a stored entry that is not 0)."""
    if hasattr(X, "tocsc"):
        X = X.tocsc()
        out = np.zeros((X.shape[1], X.shape[0]), bool)
        cols = np.repeat(np.arange(X.shape[1]), np.diff(X.indptr))
        keep = X.data != 0
        out[cols[keep], X.indices[keep]] = True
        return out
    return (np.asarray(X) != 0).T


def topm(r, seen, m):
    r = np.asarray(r)
    n, D = r.shape
    feats = np.full((n, m), -1, np.int32)
    vals = np.full((n, m), np.nan, r.dtype)
    for i in range(n):
        cand = np.flatnonzero(~seen[i]) if seen is not None else np.arange(D)
        order = cand[np.argsort(-r[i, cand], kind="stable")][:m]          # stable: ties keep the lower feature first
        feats[i, :len(order)] = order
        vals[i, :len(order)] = r[i, order]
    return feats, vals


def check(features, prob, P, theta, seen, m, skip_rows=None, what=""):
    """Asserts the properties of the header for every point.  seen: (n, D) bool or None (exclude_seen=False); skip_rows: (n,) bool, the
    points that take no part.  Returns the largest error in units of the bound."""
    features, prob = np.asarray(features), np.asarray(prob)
    n, K = np.asarray(P).shape
    D = np.asarray(theta).shape[1]
    assert features.shape == prob.shape == (n, m) and features.dtype == np.int32 and prob.dtype == np.float32, what
    r = exact(P, theta)
    e = eps(K)
    skip_rows = np.zeros(n, bool) if skip_rows is None else np.asarray(skip_rows, bool)
    worst = 0.0
    for i in range(n):
        f, p = features[i], prob[i]
        if skip_rows[i]:
            assert (f == -1).all() and np.isnan(p).all(), (what, i, "a skipped point")
            continue
        cand = ~seen[i] if seen is not None else np.ones(D, bool)
        nc = min(m, int(cand.sum()))
        assert (f[nc:] == -1).all() and np.isnan(p[nc:]).all(), (what, i, "slots beyond the candidates")
        f, p = f[:nc], p[:nc]
        assert ((f >= 0) & (f < D)).all() and not np.isnan(p).any(), (what, i)
        assert len(set(f.tolist())) == nc, (what, i, "a feature is repeated")
        assert cand[f].all(), (what, i, "a seen feature is returned")
        rs = r[i, f]
        err = np.abs(p.astype(np.float64) - rs)
        assert (err <= e * rs).all(), (what, i, "prob is outside the bound", p, rs)
        if nc:
            worst = max(worst, float((err / np.maximum(e * rs, 1e-300)).max()))
        bits = p.view(np.uint32)
        assert (np.diff(p) <= 0).all(), (what, i, "prob increases")
        tie = bits[1:] == bits[:-1]
        assert (np.diff(f)[tie] > 0).all(), (what, i, "equal bits, decreasing feature")
        rest = cand.copy()
        rest[f] = False
        if nc and rest.any():
            assert (r[i, rest] * (1 - e) <= (1 + e) * rs.min()).all(), (what, i, "a better candidate was left out")
    return worst
