"""The definitions of include/dpmm_hip_explain.h in numpy Float64, from the Float32 m, R, df the worker is given (tools/typicality_ref.py's
`worker_params`).  For a point of cluster k, z = x - m_k, A = R_k' R_k, y = R_k z, q = |y|^2:

  g_d = sum_{r <= d} R_rd y_r,   a_d = A_dd = sum_{r <= d} R_rd^2,
  e_d = g_d / a_d,   q_-d = q - g_d^2 / a_d,   t_d = g_d sqrt((df + D - 1) / (a_d (df + max(q_-d, 0)))),
  tail_d = 2 P(T >= |t_d|) for T ~ Student-t(df + D - 1), by scipy.stats.t.sf,

and the quantities the Float32 error bounds are stated in, u = 2^-24:
  b_d     = sum_{r <= d} |R_rd| sum_{c >= r} |R_rc| |z_c|
  e_bound = (2 D + 6) u b_d / a_d
  t_bound = sqrt((df + D - 1) / (a_d h)) dg + |t_d| / (2 h) (dq + 2 |g_d| dg / a_d) + 16 u |t_d|,
            dg = (2 D + 3) u b_d, dq = (3 D + 4) u a_i (a_i of typicality_ref.reference), h = df + q_-d   -- the first-order bound; the tests
            allow twice it."""
import collections

import numpy as np

from . import typicality_ref as T

U32 = 2.0 ** -24

Reference = collections.namedtuple("Reference", "e t tail q b e_bound t_bound")


def feature_tail_of(t, dof):
    """2 P(T >= |t|), T ~ Student-t(dof), in Float64; t, dof broadcast."""
    from scipy.stats import t as student
    return 2.0 * student.sf(np.abs(np.asarray(t, np.float64)), np.asarray(dof, np.float64))


def reference(X, lab0, m, R, df):
    """X (D, n) the points as the model sees them (Float32), lab0 (n,) their 0-based clusters; m, R, df: `typicality_ref.worker_params`.
    Returns a `Reference` of Float64 arrays, (n, D) each but q (n,)."""
    X = np.asarray(X, np.float32).astype(np.float64)
    D, n = X.shape
    lab0 = np.asarray(lab0, np.int64)
    m64, R64, df64 = m.astype(np.float64), R.astype(np.float64), df.astype(np.float64)
    q, ai, _ = T.reference(X, lab0, m, R, df)
    e, t, b, eb, tb = (np.zeros((n, D)) for _ in range(5))
    for k in np.unique(lab0):
        idx = np.flatnonzero(lab0 == k)
        Rk, dfk = R64[k], df64[k]
        z = X[:, idx].T - m64[k]
        g = (z @ Rk.T) @ Rk                                              # g = R' (R z)
        a = (Rk * Rk).sum(0)                                             # a_d = sum_r R_rd^2
        bk = (np.abs(z) @ np.abs(Rk).T) @ np.abs(Rk)
        qm = q[idx, None] - g * g / a
        h = dfk + np.maximum(qm, 0.0)
        tk = g * np.sqrt((dfk + D - 1) / (a * h))
        dg = (2 * D + 3) * U32 * bk
        dq = (3 * D + 4) * U32 * ai[idx, None]
        e[idx], t[idx], b[idx] = g / a, tk, bk
        eb[idx] = (2 * D + 6) * U32 * bk / a
        tb[idx] = np.sqrt((dfk + D - 1) / (a * h)) * dg + np.abs(tk) / (2 * h) * (dq + 2 * np.abs(g) * dg / a) + 16 * U32 * np.abs(tk)
    tail = feature_tail_of(t, (df64[lab0] + D - 1)[:, None])
    return Reference(e, t, tail, q, b, eb, tb)


def direct_conditional(x, m, R, df):
    """(t_d) of ONE point by the textbook route, no shortcut through R: Sigma = (R'R)^-1; feature d given the rest x_o has conditional mean
    m_d + S_do S_oo^-1 (x_o - m_o), and under t_df(m, Sigma) the conditional law is Student-t with df + D - 1 degrees of freedom and scale^2
    (df + q_o) / (df + D - 1) (S_dd - S_do S_oo^-1 S_od), q_o the squared distance of x_o under its marginal."""
    x, m, R = (np.asarray(v, np.float64) for v in (x, m, R))
    D = len(x)
    S = np.linalg.inv(R.T @ R)
    out = np.zeros(D)
    for d in range(D):
        o = np.array([j for j in range(D) if j != d], np.int64)
        if len(o) == 0:
            out[d] = (x[d] - m[d]) / np.sqrt(S[d, d])
            continue
        w = np.linalg.solve(S[np.ix_(o, o)], x[o] - m[o])
        mean = m[d] + S[d, o] @ w
        var = S[d, d] - S[d, o] @ np.linalg.solve(S[np.ix_(o, o)], S[o, d])
        qo = (x[o] - m[o]) @ w
        out[d] = (x[d] - mean) / np.sqrt((df + qo) / (df + D - 1) * var)
    return out
