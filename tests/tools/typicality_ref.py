"""The definitions of include/dpmm_hip_typicality.h in numpy Float64, from the Float32 m, R, df the worker is given.

  q_i    = |R_k (x_i - m_k)|^2 for the cluster k the point is given (0-based `lab0`), R_k upper triangular;
  a_i    = sum_r (sum_c |R_rc| |z_c|)^2, the quantity the Float32 error bound of q is stated in;
  tail_i = I_{df / (df + q)}(df / 2, D / 2) by scipy.special.betainc."""
import numpy as np


def worker_params(m, R, df):
    """(m (K, D), R (K, D, D) upper triangular, df (K,)) as Float32 -- what binding.Worker.set_predictive_niw hands the library."""
    m = np.asarray(m, np.float32)
    K, D = m.shape
    return m, np.triu(np.asarray(R, np.float32).reshape(K, D, D)), np.asarray(df, np.float32)


def tail_of(q, df, D):
    """I_{df / (df + q)}(df / 2, D / 2) in Float64; q, df broadcast."""
    from scipy.special import betainc
    q, df = np.asarray(q, np.float64), np.asarray(df, np.float64)
    return betainc(0.5 * df, 0.5 * D, df / (df + q))


def reference(X, lab0, m, R, df):
    """X (D, n) the points as the model sees them (Float32), lab0 (n,) their 0-based clusters; m, R, df: `worker_params`.
    Returns (q, a, tail), Float64 (n,)."""
    X = np.asarray(X, np.float32).astype(np.float64)
    D, n = X.shape
    lab0 = np.asarray(lab0, np.int64)
    m64, R64, df64 = m.astype(np.float64), R.astype(np.float64), df.astype(np.float64)
    q, a = np.zeros(n), np.zeros(n)
    for k in np.unique(lab0):
        idx = np.flatnonzero(lab0 == k)
        z = X[:, idx].T - m64[k]
        y = z @ R64[k].T
        q[idx] = (y * y).sum(1)
        a[idx] = ((np.abs(z) @ np.abs(R64[k]).T) ** 2).sum(1)
    return q, a, tail_of(q, df64[lab0], D)


def ks_uniform(u):
    """sup |F_n - F| of a sample against U(0, 1)."""
    s = np.sort(np.asarray(u, np.float64))
    n = len(s)
    return max(np.max(np.arange(1, n + 1) / n - s), np.max(s - np.arange(n) / n))
