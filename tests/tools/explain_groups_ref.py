"""The definitions of include/dpmm_hip_explain_groups.h in numpy Float64, from the Float32 x, m, R, df the worker is given
(tools/typicality_ref.py's `worker_params`).  For a point of cluster k, z = x - m_k, A = R_k' R_k, y = R_k z, q = |y|^2, g = A z, and a
group G of s features, A_GG = L L', W = L^-1, v = W g_G:

  q_G = |v|^2,   f_G = q_G (df + D - s) / (df + max(q - q_G, 0)),   tail_G = I_{nu / (nu + f_G)}(nu / 2, s / 2), nu = df + D - s,

and the quantities the Float32 error bounds are stated in, u = 2^-24, b_c of tools/explain_ref.py:
  dg_c     = (2 D + 3) u b_c
  dv_r     = sum_c |W_rc| dg_c + (s + 2) u sum_c |W_rc| |g_c|
  qg_bound = 2 sum_r |v_r| dv_r + (s + 2) u q_G                        -- the first-order bound; the tests allow twice it
  f_bound  = (df + D - s) / h qg_bound + f_G / h (dq + qg_bound) + 4 u f_G,  dq = (3 D + 4) u a_i, h = df + q - q_G: what the bounds on q_G
             and q leave of f_G, with the four roundings of the Float32 formulas; the tests allow twice it.

The cases of tests/test_gpu_explain_groups.py live here, so that tests/test_explain_groups_cpu.py can check on the CPU that the bound
tells a wrong grouping from the right one on every one of them."""
import collections

import numpy as np

from . import explain_ref as E
from . import sample_ref as SR
from . import typicality_ref as T

U32 = 2.0 ** -24

Reference = collections.namedtuple("Reference", "q qg f tail g qg_bound f_bound")


def stat32(q, qg, df, D, s):
    """f as the kernel forms it, in numpy Float32 from the Float32 q, q_G, df: every operation is correctly rounded, so these are its bits."""
    q, qg, df = (np.asarray(a, np.float32) for a in (q, qg, df))
    h = df + np.maximum(q - qg, np.float32(0))
    return (qg * (df + np.float32(D - s))) / h


def tail_of(f, dof, s):
    """P(F(s, dof) >= f / s) in Float64 by scipy.special.betainc; f, dof, s broadcast."""
    return T.tail_of(f, dof, s)


def reference(X, lab0, m, R, df, groups):
    """X (D, n) the points as the model sees them (Float32), lab0 (n,) their 0-based clusters; m, R, df: `typicality_ref.worker_params`;
    groups: lists of 0-based features.  Returns a `Reference` of Float64 arrays, (n, G) each but q (n,) and g (n, D)."""
    X = np.asarray(X, np.float32).astype(np.float64)
    D, n = X.shape
    G = len(groups)
    lab0 = np.asarray(lab0, np.int64)
    m64, R64, df64 = m.astype(np.float64), R.astype(np.float64), df.astype(np.float64)
    q, ai, _ = T.reference(X, lab0, m, R, df)
    qg, f, tail, qb, fb = (np.zeros((n, G)) for _ in range(5))
    gall = np.zeros((n, D))
    for k in np.unique(lab0):
        idx = np.flatnonzero(lab0 == k)
        Rk, dfk = R64[k], df64[k]
        A = Rk.T @ Rk
        z = X[:, idx].T - m64[k]
        g = (z @ Rk.T) @ Rk
        gall[idx] = g
        dg = (2 * D + 3) * U32 * ((np.abs(z) @ np.abs(Rk).T) @ np.abs(Rk))
        dq = (3 * D + 4) * U32 * ai[idx]
        for j, grp in enumerate(groups):
            Gi = np.asarray(grp, np.int64)
            s = len(Gi)
            W = np.linalg.inv(np.linalg.cholesky(A[np.ix_(Gi, Gi)]))
            v = g[:, Gi] @ W.T
            qj = (v * v).sum(1)
            dv = dg[:, Gi] @ np.abs(W).T + (s + 2) * U32 * (np.abs(g[:, Gi]) @ np.abs(W).T)
            bq = 2 * (np.abs(v) * dv).sum(1) + (s + 2) * U32 * qj
            h = dfk + np.maximum(q[idx] - qj, 0.0)
            fj = qj * (dfk + D - s) / h
            qg[idx, j], f[idx, j], qb[idx, j] = qj, fj, bq
            fb[idx, j] = (dfk + D - s) / h * bq + fj / h * (dq + bq) + 4 * U32 * fj
            tail[idx, j] = tail_of(fj, dfk + D - s, s)
    return Reference(q, qg, f, tail, gall, qb, fb)


def direct_conditional(x, m, R, df, group):
    """(q_G, f_G) of ONE point by the textbook route: Sigma = (R'R)^-1; block G given the rest x_o has conditional mean
    m_G + S_Go S_oo^-1 (x_o - m_o) and scale matrix (df + q_o) / (df + D - s) (S_GG - S_Go S_oo^-1 S_oG), q_o the squared distance of x_o
    under its marginal; f_G is the squared Mahalanobis distance of x_G under that scale, q_G the same under S_GG - S_Go S_oo^-1 S_oG."""
    x, m, R = (np.asarray(v, np.float64) for v in (x, m, R))
    D = len(x)
    S = np.linalg.inv(R.T @ R)
    G = np.asarray(group, np.int64)
    o = np.array([j for j in range(D) if j not in set(group)], np.int64)
    s = len(G)
    if len(o) == 0:
        r, C, qo = x[G] - m[G], S[np.ix_(G, G)], 0.0
    else:
        w = np.linalg.solve(S[np.ix_(o, o)], x[o] - m[o])
        r = x[G] - (m[G] + S[np.ix_(G, o)] @ w)
        C = S[np.ix_(G, G)] - S[np.ix_(G, o)] @ np.linalg.solve(S[np.ix_(o, o)], S[np.ix_(o, G)])
        qo = (x[o] - m[o]) @ w
    qG = r @ np.linalg.solve(C, r)
    return qG, qG * (df + D - s) / (df + qo)


def swapped(groups):
    """`groups` with one feature exchanged between the first two groups (the last of the first, the first of the second): the wrong grouping
    the bound must tell from the right one.  None for a single group: there is nothing to exchange (the identity q_G = q anchors it)."""
    if len(groups) < 2:
        return None
    a, b = list(groups[0]), list(groups[1])
    a[-1], b[0] = b[0], a[-1]
    return [sorted(a), sorted(b)] + [list(g) for g in groups[2:]]


def discriminates(ref, wrong):
    """The right reference and the one of the wrong grouping are further apart than twice the bound on at least one point and group."""
    return bool(np.any(np.abs(ref.qg - wrong.qg) > 2 * ref.qg_bound + 2 * wrong.qg_bound))


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
K_CASE, N_CASE = 3, 300


def _blocks(D, s):
    return [list(range(a, a + s)) for a in range(0, D, s)]


# (D, name, groups).  The issue names {60..64} and {0, 64} at D = 65: they share feature 64 and groups are disjoint, so each gets a case of
# its own, with a second group beside it and one feature left uncovered.
CASES = [
    (5, "1+2+2", [[0], [1, 3], [2, 4]]),
    (64, "64x1", _blocks(64, 1)),
    (64, "4x16", _blocks(64, 16)),
    (64, "all", [list(range(64))]),
    (65, "60..64", [list(range(60, 65)), list(range(1, 60))]),                       # crosses the lane tile; feature 0 uncovered
    (65, "0,64", [[0, 64], [d for d in range(1, 64) if d != 32]]),                   # feature 32 uncovered
    (130, "100+7", [list(range(100)), list(range(100, 107))]),                       # s > 64: two row tiles
    (256, "4x64", _blocks(256, 64)),
    (256, "all", [list(range(256))]),
]
CASE_IDS = [f"D{D}-{name}" for D, name, _ in CASES]


def case_model(D, heavy):
    """(post, m, A, df) of a case: K_CASE clusters, the centres spread so that most points keep the cluster they were drawn from."""
    post, m, A, df = SR.niw_model(D, K_CASE, D + 3.0 if heavy else 1e5, 11 * D + 5 + heavy)
    post["m"] = m = (m * 4.0).astype(np.float32).astype(np.float64)
    return post, m, A, df


def push_out(X, lab0, m, A, groups):
    """The last six points of X (D, n) moved far out along the first group: the centre of their cluster plus 4, 10, 30 conditional-scale
    units along the block's first and last feature.  In place; returns X."""
    n = X.shape[1]
    blk = groups[0]
    for t, (i, d, amount) in enumerate(zip(range(n - 6, n), [blk[0], blk[-1]] * 3, [4.0, 4.0, 10.0, 10.0, 30.0, 30.0])):
        k = lab0[i]
        X[:, i] = m[k]
        X[d, i] = np.float32(m[k][d] + amount * np.abs(A[k][d, d]))
    return X


def case_points_cpu(D, heavy, groups):
    """(X (D, n) Float32, lab0): the reference sampler's draws (tools/sample_ref.py: the law of `Predictor.sample`) and the pushed points."""
    post, m, A, df = case_model(D, heavy)
    lab0 = np.arange(N_CASE) % K_CASE
    X = SR.niw_points(m, A, df, lab0, np.arange(N_CASE), 77 + D).T.astype(np.float32)
    return push_out(X, lab0, m, A, groups), lab0
