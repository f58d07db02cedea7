"""The marginal definitions of include/dpmm_hip_typicality.h and include/dpmm_hip_explain.h ("Points with gaps") in numpy Float64, built
from the complete-case references: for a cluster k and a gap pattern M (the NaN features of a point, O the others, D_o = |O|)

  Sigma = (R_k' R_k)^-1,  P = (Sigma_OO)^-1,  R_o = chol(P)' (upper triangular, R_o' R_o = P),

and `typicality_ref.reference` / `explain_ref.reference` are called at D_o with (m_O, R_o, df_k) on the observed rows of the points.  What
the complete-case references cannot give -- the Float32 error bounds, which are stated in the FULL factor R_k -- is formed here, u = 2^-24:

  a_i     = sum_r (sum_{c in O} |R_rc| |z_c|)^2
  F       = 2 r (D + 8 r + 16) 2^-52 cond(A_MM)                                           A = R_k' R_k, A_MM = C'C
  q_bound = (3 D + 4) u a_i + F a_i
  dg      = ((2 D + 3) u + F) sqrt(A_dd a_i)
  ra      = (A_dd / a'_d) (u (1 + 2 D sqrt(r cond(A_MM))) + F)                            relative, on a'_d = P_dd
  e_bound = dg / a'_d + |e_d| (ra + u)
  t_bound = sqrt((df + D_o - 1) / (a'_d h)) dg + |t_d| ra / 2 + |t_d| / (2 h) (q_bound + 2 |g'_d| dg / a'_d + g'_d^2 / a'_d ra) + 2 u |t_d|
            -- the first-order bound; the tests allow twice it, as they do for complete points."""
import collections

import numpy as np

from . import explain_ref as E
from . import typicality_ref as T

U32 = 2.0 ** -24
U64 = 2.0 ** -53

GapReference = collections.namedtuple("GapReference", "q tail q_bound e t ftail e_bound t_bound gprime aprime r")


def marginal_factor(Rk, obs):
    """(R_o, P): the upper-triangular factor of P = (Sigma_OO)^-1 for Sigma = (Rk' Rk)^-1, Float64."""
    S = np.linalg.inv(Rk.T @ Rk)
    P = np.linalg.inv(S[np.ix_(obs, obs)])
    P = 0.5 * (P + P.T)
    return np.linalg.cholesky(P).T, P


def reference(X, lab0, m, R, df):
    """X (D, n) Float32 with NaN gaps (every point: 1 <= r <= D - 1 of them, the observed features finite), lab0 (n,) the 0-based clusters;
    m, R, df: `typicality_ref.worker_params`.  Returns a `GapReference` of Float64 arrays: (n,) for q, tail, q_bound, r; (n, D) for the
    rest, NaN on the point's missing features."""
    X = np.asarray(X, np.float32)
    D, n = X.shape
    lab0 = np.asarray(lab0, np.int64)
    m64, R64, df64 = m.astype(np.float64), R.astype(np.float64), df.astype(np.float64)
    gap = np.isnan(X)
    q, tail, qb, rr = (np.zeros(n) for _ in range(4))
    e, t, ft, eb, tb, gp, ap = (np.full((n, D), np.nan) for _ in range(7))
    groups = collections.defaultdict(list)
    for i in range(n):
        groups[(int(lab0[i]), gap[:, i].tobytes())].append(i)
    for (k, _), idx in groups.items():
        idx = np.asarray(idx)
        mis = np.flatnonzero(gap[:, idx[0]])
        obs = np.flatnonzero(~gap[:, idx[0]])
        r, Do = len(mis), len(obs)
        assert 1 <= r <= D - 1
        Rk, dfk = R64[k], df64[k]
        Ro, P = marginal_factor(Rk, obs)
        sub = (m64[k][obs][None], Ro[None], np.array([dfk]))
        zero = np.zeros(len(idx), np.int64)
        Xo = X[np.ix_(obs, idx)]
        qk, _, tk = T.reference(Xo, zero, *sub)
        ex = E.reference(Xo, zero, *sub)
        A = Rk.T @ Rk
        cond = np.linalg.cond(A[np.ix_(mis, mis)])
        z = Xo.astype(np.float64).T - m64[k][obs]                        # (n_g, D_o)
        ai = ((np.abs(z) @ np.abs(Rk[:, obs]).T) ** 2).sum(1)
        f64 = 2 * r * (D + 8 * r + 16) * 2 * U64 * cond
        qbk = (3 * D + 4) * U32 * ai + f64 * ai
        Add, apd = np.diag(A)[obs], np.diag(P)
        g = z @ P
        dg = ((2 * D + 3) * U32 + f64) * np.sqrt(Add[None] * ai[:, None])
        ra = (Add / apd)[None] * (U32 * (1 + 2 * D * np.sqrt(r * cond)) + f64)
        h = dfk + np.maximum(qk[:, None] - g * g / apd, 0.0)
        ebk = dg / apd + np.abs(ex.e) * (ra + U32)
        tbk = (np.sqrt((dfk + Do - 1) / (apd * h)) * dg + np.abs(ex.t) * ra / 2
               + np.abs(ex.t) / (2 * h) * (qbk[:, None] + 2 * np.abs(g) * dg / apd + g * g / apd * ra) + 2 * U32 * np.abs(ex.t))
        q[idx], tail[idx], qb[idx], rr[idx] = qk, tk, qbk, r
        for dst, src in ((e, ex.e), (t, ex.t), (ft, ex.tail), (eb, ebk), (tb, tbk), (gp, g), (ap, np.broadcast_to(apd, g.shape))):
            dst[np.ix_(idx, obs)] = src
    return GapReference(q, tail, qb, e, t, ft, eb, tb, gp, ap, rr)
