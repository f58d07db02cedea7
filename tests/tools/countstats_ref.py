"""The definitions of include/dpmm_hip_countstats.h in numpy Float64 (and Int64 where they are exact).

Given the points X (D, n) as the model sees them -- a dense array of Float32 values or a scipy CSC matrix, a NaN or Inf entry being a
value that is not finite -- and what the library's own `predict` / `score_samples` return for them -- 1-based labels (n,), Float32
probabilities P (n, K), Float32 logdens (n,):

  classes    skipped: a NaN in the row of P (`predict` writes NaN rows for exactly the points whose table row holds a NaN or no finite
             entry); else held out: logdens < min_logdens; else incomplete: a (stored) value that is not finite; else it takes part
  weights    hard: w_ik = [labels_i == k + 1]; soft: w_ik = (double)P_ik
  N, sums    sum_i w_ik (1, x_i) over the points that take part, W' X
  T1         the magnitude sum_i w_ik |x_id| the error bound is stated in
Any two Float64 evaluations of these sums agree within 2 gamma(n + 2) (T1, N): `gamma`, `within`.  `exact` is the Int64 evaluation for
integer data and hard weights, where every Float64 addition is exact and the answer has one value."""
import numpy as np

U = 2.0 ** -53


def gamma(m):
    return m * U / (1 - m * U)


def is_sparse(X):
    return hasattr(X, "indptr")


def finite_points(X):
    """(n,) bool: every (stored) value of the point is finite."""
    if not is_sparse(X):
        return np.isfinite(np.asarray(X)).all(0)
    X = X.tocsc()
    ok = np.ones(X.shape[1], bool)
    cols = np.repeat(np.arange(X.shape[1]), np.diff(X.indptr))
    ok[cols[~np.isfinite(X.data)]] = False
    return ok


def classes(X, P, logdens=None, min_logdens=None):
    """(skipped, held_out, incomplete, part): boolean (n,) each, exactly one true per point."""
    P = np.asarray(P)
    skipped = np.isnan(P).any(1)
    held = np.zeros_like(skipped)
    if min_logdens is not None:
        with np.errstate(invalid="ignore"):
            held = ~skipped & (np.asarray(logdens) < np.float32(min_logdens))
    incomplete = ~skipped & ~held & ~finite_points(X)
    return skipped, held, incomplete, ~(skipped | held | incomplete)


def stats(X, labels, P, mode, logdens=None, min_logdens=None):
    """dict(N, sums, T1, count, skipped, incomplete, held_out) of the n points; mode "hard" or "soft"."""
    labels, P = np.asarray(labels), np.asarray(P)
    assert P.dtype == np.float32 and X.shape[1] == P.shape[0] == labels.shape[0]
    K = P.shape[1]
    skipped, held, incomplete, part = classes(X, P, logdens, min_logdens)
    lab = labels[part] - 1
    w = np.eye(K)[lab] if mode == "hard" else P[part].astype(np.float64)              # (n_part, K)
    if is_sparse(X):
        x = X.tocsc()[:, np.flatnonzero(part)].astype(np.float64)
        sums, T1 = np.asarray((x @ w).T), np.asarray((abs(x) @ w).T)
    else:
        x = np.asarray(X)[:, part].astype(np.float64)
        sums, T1 = (x @ w).T, (np.abs(x) @ w).T
    return dict(N=w.sum(0), sums=sums.reshape(K, X.shape[0]), T1=T1.reshape(K, X.shape[0]), count=np.bincount(lab, minlength=K).astype(np.int64)[:K],
                skipped=int(skipped.sum()), incomplete=int(incomplete.sum()), held_out=int(held.sum()))


def exact(X, labels, P, logdens=None, min_logdens=None):
    """(N, sums) in Int64 for integer data and hard weights: the one value every exact evaluation has."""
    labels = np.asarray(labels)
    K = np.asarray(P).shape[1]
    part = classes(X, P, logdens, min_logdens)[3]
    w = np.eye(K, dtype=np.int64)[labels[part] - 1]
    if is_sparse(X):
        x = X.tocsc()[:, np.flatnonzero(part)]
        assert (x.data == np.rint(x.data)).all()
        sums = np.asarray((x.astype(np.int64) @ w).T)
    else:
        x = np.asarray(X)[:, part]
        assert (x == np.rint(x)).all()
        sums = (x.astype(np.int64) @ w).T
    return w.sum(0), sums.reshape(K, X.shape[0])


def add(results):
    """The result for the union of disjoint pieces."""
    return {k: sum(r[k] for r in results) for k in results[0]}


def within(got, want, n):
    """The largest of |got - want| / (2 gamma(n + 2) magnitude) over N and sums -- at most 1 inside the bound; got: anything with N, sums."""
    get = (lambda f: got[f]) if isinstance(got, dict) else (lambda f: getattr(got, f))
    b = 2 * gamma(n + 2)
    worst = 0.0
    for f, mag in (("N", "N"), ("sums", "T1")):
        d, m = np.abs(np.asarray(get(f), np.float64) - want[f]), b * want[mag]
        if (d[m == 0] != 0).any():
            return np.inf
        worst = max(worst, float((d[m > 0] / m[m > 0]).max()) if (m > 0).any() else 0.0)
    return worst
