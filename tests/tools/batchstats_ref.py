"""The definitions of include/dpmm_hip_batchstats.h and the conjugate NIW update of host/absorb.py in numpy Float64.

Given the points X (D, n) as the model sees them (Float32 values) and what the library's own `predict` / `score_samples` return for
them -- 1-based labels (n,), Float32 probabilities P (n, K), Float32 logdens (n,):

  classes    skipped: a NaN in the row of P (`predict` writes NaN rows for exactly the points whose table row holds a NaN or no finite
             entry); else held out: logdens < min_logdens; else incomplete: a feature that is not finite; else the point takes part
  weights    hard: w_ik = [labels_i == k + 1]; soft: w_ik = (double)P_ik
  N, sums, S = sum_i w_ik (1, x_i, x_i x_i') over the points that take part, by einsum
  T, T1      the magnitudes sum_i w_ik |x_id| |x_ie| and sum_i w_ik |x_id| the error bound is stated in
Any two Float64 evaluations of these sums agree within 2 gamma(n + 2) (T, T1, N): `gamma`, `within`.

The conjugate update in two formulations that differ only in rounding: `update_uncentred` from (N, sums, S) as host/absorb.py states it
and `update_centred` from the weighted points, Psi' = Psi + sum w (x - xbar)(x - xbar)' + kappa N / (kappa + N) (xbar - m)(xbar - m)'."""
import numpy as np

U = 2.0 ** -53


def gamma(m):
    return m * U / (1 - m * U)


def classes(X, P, logdens=None, min_logdens=None):
    """(skipped, held_out, incomplete, part): boolean (n,) each, exactly one true per point."""
    X, P = np.asarray(X), np.asarray(P)
    skipped = np.isnan(P).any(1)
    held = np.zeros_like(skipped)
    if min_logdens is not None:
        with np.errstate(invalid="ignore"):
            held = ~skipped & (np.asarray(logdens) < np.float32(min_logdens))
    incomplete = ~skipped & ~held & ~np.isfinite(X).all(0)
    return skipped, held, incomplete, ~(skipped | held | incomplete)


def stats(X, labels, P, mode, logdens=None, min_logdens=None):
    """dict(N, sums, S, T, T1, count, skipped, incomplete, held_out) of the n points; mode "hard" or "soft"."""
    X, labels, P = np.asarray(X), np.asarray(labels), np.asarray(P)
    assert P.dtype == np.float32 and X.shape[1] == P.shape[0] == labels.shape[0]
    K = P.shape[1]
    skipped, held, incomplete, part = classes(X, P, logdens, min_logdens)
    x = X[:, part].T.astype(np.float64)                                                   # (n_part, D)
    lab = labels[part] - 1
    w = np.eye(K)[lab] if mode == "hard" else P[part].astype(np.float64)
    ax = np.abs(x)
    return dict(N=w.sum(0), sums=np.einsum("ik,id->kd", w, x), S=np.einsum("ik,id,ie->kde", w, x, x, optimize=True),
                T=np.einsum("ik,id,ie->kde", w, ax, ax, optimize=True), T1=np.einsum("ik,id->kd", w, ax),
                count=np.bincount(lab, minlength=K).astype(np.int64)[:K], skipped=int(skipped.sum()), incomplete=int(incomplete.sum()),
                held_out=int(held.sum()))


def add(results):
    """The result for the union of disjoint pieces."""
    return {k: sum(r[k] for r in results) for k in results[0]}


def within(got, want, n):
    """The largest of |got - want| / (2 gamma(n + 2) magnitude) over N, sums and S -- at most 1 inside the bound; got: anything with N, sums, S."""
    get = (lambda f: got[f]) if isinstance(got, dict) else (lambda f: getattr(got, f))
    b = 2 * gamma(n + 2)
    worst = 0.0
    for f, mag in (("N", "N"), ("sums", "T1"), ("S", "T")):
        d, m = np.abs(np.asarray(get(f), np.float64) - want[f]), b * want[mag]
        if (d[m == 0] != 0).any():
            return np.inf
        worst = max(worst, float((d[m > 0] / m[m > 0]).max()) if (m > 0).any() else 0.0)
    return worst


def update_uncentred(kappa, nu, m, Psi, N, sums, S):
    """(kappa', nu', m', Psi') with Psi = nu psi the scale matrix: Psi' = Psi + S + kappa m m' - kappa' m' m''."""
    k1 = kappa + N
    m1 = (kappa * m + sums) / k1
    return k1, nu + N, m1, Psi + S + kappa * np.outer(m, m) - k1 * np.outer(m1, m1)


def update_centred(kappa, nu, m, Psi, w, x):
    """The same from the weights w (n,) and the points x (n, D): Psi' = Psi + sum w (x - xbar)(x - xbar)' + kappa N / (kappa + N) (xbar - m)(xbar - m)'."""
    N = w.sum()
    xbar = (w[:, None] * x).sum(0) / N
    c = x - xbar
    k1 = kappa + N
    return k1, nu + N, m + (N / k1) * (xbar - m), Psi + (w[:, None] * c).T @ c + (kappa * N / k1) * np.outer(xbar - m, xbar - m)


def rel(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())
