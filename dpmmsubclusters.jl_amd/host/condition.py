"""Conditioning a fitted NIW mixture on a fixed set of features, in Float64 on the host (include/dpmm_hip_regress.h serves the result).

Two facts carry everything here.

  * CLOSURE.  The marginal of an NIW posterior over a subset O of the features is an NIW posterior again.  With Psi = U U' (= nu psi, as
    host/priors.py keeps it), D_o = |O|:
        kappa' = kappa,   m' = m[O],   nu' = nu - (D - D_o),   Psi' = Psi[O, O] = U' U''  (U' upper triangular),
        logdet_psi' = log det(Psi[O, O]) - D_o log nu'         (what `posterior()` calls logdet_psi: that of psi = Psi / nu).
    Its Student-t predictive has nu' - D_o + 1 = nu - D + 1 degrees of freedom: the same as the full model's.  `niw_marginal` is that rule;
    a Predictor made from its result scores, samples, absorbs and grows like any other.

  * REGRESSION.  Cluster k's predictive is t_df(m, Sigma), Sigma^-1 = A = R'R.  Split into the targets M and the given features O:
        E[x_M | x_O, k]   = m_M - (A_MM)^-1 A_MO (x_O - m_O)                      = c_k + B_k x_O
        Cov[x_M | x_O, k] = (df + q) / (df + D_o - 2) (A_MM)^-1,   q = (x_O - m_O)' Sigma_OO^-1 (x_O - m_O)
    (a conditional of a multivariate t is a multivariate t with df + D_o degrees of freedom).  `regression_tables` forms B, c, the
    diagonal V of (A_MM)^-1 and the constant h of the marginal model's table entry, per cluster, by Cholesky of A_MM.
"""
import numpy as np
from scipy.special import gammaln


def check_features(features, D, what="features"):
    """`features` as a list of distinct 0-based indices below D, 1 <= len <= D - 1; ValueError otherwise."""
    try:
        idx = [int(f) for f in features]
        same = all(i == f for i, f in zip(idx, features))
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a list of feature indices") from None
    if not same:
        raise ValueError(f"{what} must be a list of integer feature indices")
    if not 1 <= len(idx) <= D - 1:
        raise ValueError(f"{what} must name between 1 and D - 1 = {D - 1} features")
    if min(idx) < 0 or max(idx) >= D:
        raise ValueError(f"{what} must lie in 0..{D - 1}")
    if len(set(idx)) != len(idx):
        raise ValueError(f"{what} must not repeat a feature")
    return idx


def upper_factor(A):
    """Upper-triangular U with U U' = A for a batch of SPD matrices (n, d, d): the Cholesky factor of A with rows and columns reversed,
    reversed back."""
    A = np.asarray(A, np.float64)
    L = np.linalg.cholesky(A[..., ::-1, ::-1])
    return L[..., ::-1, ::-1]


def niw_marginal(post, features):
    """The NIW posterior arrays (kappa, nu, m, U, logdet_psi; any number of rows) of the features `features`, in that order."""
    O = np.asarray(features, np.int64)
    U = np.asarray(post["U"], np.float64)
    D, Do = U.shape[-1], len(O)
    Psi = np.einsum("nij,nkj->nik", U, U)[:, O[:, None], O[None, :]]
    Uo = upper_factor(Psi)
    nu = np.asarray(post["nu"], np.float64) - (D - Do)
    logdet = 2.0 * np.log(np.einsum("nii->ni", Uo)).sum(1) - Do * np.log(nu)
    return dict(kappa=np.array(post["kappa"], np.float64), nu=nu, m=np.asarray(post["m"], np.float64)[:, O].copy(), U=Uo, logdet_psi=logdet)


def hyper_marginal(hyper, features):
    """The hyper-parameters kappa, m, nu, psi (psi mean-like: the scale is nu psi) of the same features, by the same rule."""
    O = np.asarray(features, np.int64)
    psi = np.asarray(hyper["psi"], np.float64)
    D, Do = psi.shape[0], len(O)
    nu = float(hyper["nu"])
    nu_o = nu - (D - Do)
    return dict(kappa=np.float64(hyper["kappa"]), m=np.asarray(hyper["m"], np.float64).ravel()[O].copy(), nu=np.float64(nu_o),
                psi=psi[O[:, None], O[None, :]] * (nu / nu_o))


def table_constant(logdet, df, w, D):
    """h_k = lgamma((df + D) / 2) - lgamma(df / 2) - D / 2 log(df pi) - logdet / 2 + log w: the x-independent part of the table entry
    parr_ik = h_k - (df_k + D) / 2 log1p(q_ik / df_k) of a D-dimensional Student-t predictive."""
    logdet, df, w = (np.asarray(a, np.float64) for a in (logdet, df, w))
    return gammaln(0.5 * (df + D)) - gammaln(0.5 * df) - 0.5 * D * np.log(df * np.pi) - 0.5 * logdet + np.log(w)


def regression_tables(m, R, given, targets, factor=False):
    """(B (K, D_t, D_o), c (K, D_t), V (K, D_t)) in Float64 from the predictive parameters m (K, D), R (K, D, D) or (K, D D) upper triangular
    with Sigma^-1 = R'R, over the features of one model: `given` and `targets` index it, disjoint.  Features in neither are marginalised
    away first -- the precision of the sub-model over given + targets is the inverse of that block of Sigma -- then, with A that precision,
        B = -(A_MM)^-1 A_MO,   c = m_M - B m_O,   V = diag((A_MM)^-1)
    by Cholesky of A_MM = L L'.  factor=True: (B, c, V, W) with W = (L^-1)' (K, D_t, D_t), upper triangular, W W' = (A_MM)^-1 -- what a
    draw from the conditional law multiplies its normals with (include/dpmm_hip_regress_draw.h):
        x_M = c + B x_O + sqrt((df + q) / g) W n,   n ~ N(0, I),  g ~ chi^2(df + D_o)."""
    m = np.asarray(m, np.float64)
    K, D = m.shape
    R = np.asarray(R, np.float64).reshape(K, D, D)
    O, M = np.asarray(given, np.int64), np.asarray(targets, np.int64)
    S = np.concatenate([O, M])
    Do, Dt = len(O), len(M)
    if len(S) == D:
        A = np.einsum("kji,kjl->kil", R, R)[:, S[:, None], S[None, :]]
    else:      # Sigma = R^-1 R^-T; its block over S, inverted
        Ri = np.linalg.inv(R)
        Sig = np.einsum("kij,klj->kil", Ri, Ri)[:, S[:, None], S[None, :]]
        A = np.linalg.inv(Sig)
        A = 0.5 * (A + A.transpose(0, 2, 1))
    Amm, Amo = A[:, Do:, Do:], A[:, Do:, :Do]
    L = np.linalg.cholesky(Amm)
    Li = np.linalg.inv(L)                                   # lower triangular: (A_MM)^-1 = Li' Li
    Ainv = np.einsum("kji,kjl->kil", Li, Li)
    B = -np.einsum("kij,kjl->kil", Ainv, Amo)
    c = m[:, M] - np.einsum("kij,kj->ki", B, m[:, O])
    V = np.einsum("kii->ki", Ainv).copy()
    assert B.shape == (K, Dt, Do)
    if factor:
        return B, c, V, np.ascontiguousarray(Li.transpose(0, 2, 1))
    return B, c, V


def check_groups(groups, D, most):
    """`groups` of `Predictor.explain_groups` -- a sequence of index sequences, or a dict name -> indices -- as (names or None, list of
    sorted lists of distinct 0-based indices below D): 1 .. `most` groups, none empty, pairwise disjoint; ValueError otherwise."""
    names = None
    if isinstance(groups, dict):
        names, groups = tuple(groups.keys()), list(groups.values())
    try:
        groups = [list(g) for g in groups]
    except TypeError:
        raise ValueError("groups must be a sequence of sequences of feature indices, or a dict name -> indices") from None
    if not 1 <= len(groups) <= most:
        raise ValueError(f"groups must hold between 1 and {most} groups")
    out, seen = [], set()
    for j, g in enumerate(groups):
        what = f"group {names[j]!r}" if names is not None else f"group {j}"
        try:
            idx = [int(f) for f in g]
            same = all(i == f for i, f in zip(idx, g))
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a sequence of integer feature indices") from None
        if not same:
            raise ValueError(f"{what} must be a sequence of integer feature indices")
        if not idx:
            raise ValueError(f"{what} is empty")
        if min(idx) < 0 or max(idx) >= D:
            raise ValueError(f"{what} must lie in 0..{D - 1}")
        if len(set(idx)) != len(idx):
            raise ValueError(f"{what} repeats a feature")
        if seen & set(idx):
            raise ValueError(f"{what} overlaps an earlier group in {sorted(seen & set(idx))}")
        seen |= set(idx)
        out.append(sorted(idx))
    return names, out


def group_factors(R, groups, packed=True):
    """The tables of include/dpmm_hip_explain_groups.h in Float64 from the predictive factors R (K, D, D) or (K, D D), upper triangular
    with Sigma^-1 = A = R'R -- the Float32 values the worker holds, widened: the exact A is defined from these.  For every cluster and every
    group G (a sorted list of feature indices) A_GG = L L' by Cholesky and W = L^-1, lower triangular, so that q_G = |W g_G|^2.
    packed=True: (K, T) -- per cluster group after group, per group the rows of the lower triangle, row r holding columns 0 .. r.
    packed=False: a list of (K, s, s) arrays, one per group."""
    R = np.asarray(R)
    K = R.shape[0]
    D = int(round(np.sqrt(R.size // K)))
    R = np.triu(R.astype(np.float32).astype(np.float64).reshape(K, D, D))
    A = np.einsum("kji,kjl->kil", R, R)
    Ws = []
    for g in groups:
        G = np.asarray(g, np.int64)
        L = np.linalg.cholesky(A[:, G[:, None], G[None, :]])
        Ws.append(np.tril(np.linalg.inv(L)))
    if not packed:
        return Ws
    return np.concatenate([W[:, np.tril_indices(W.shape[1])[0], np.tril_indices(W.shape[1])[1]] for W in Ws], axis=1)


# ---- the quantiles of a Student-t (include/dpmm_hip_regress_cdf.h: the table z of dpmm_set_regression_levels), in the library's own
# arithmetic: the incomplete beta function by the continued fraction csrc/typicality_math.h evaluates, a safeguarded Newton solve on it
def _beta_cf(a, b, x):
    """The continued fraction of I_x(a, b) (modified Lentz), elementwise in Float64."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 - qab * x / qap
    d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
    h = d.copy()
    live = np.ones(x.shape, bool)
    for m in range(1, 20001):
        m2 = 2.0 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
            c = 1.0 + aa / c
            c = np.where(np.abs(c) < tiny, tiny, c)
            delta = d * c
            h = np.where(live, h * delta, h)
        live = live & (np.abs(delta - 1.0) >= 2.5e-16)
        if not live.any():
            break
    return h


def _log_beta(a, b):
    """log B(a, b) as csrc/typicality_math.h forms it: for a >= 32 the two large terms are never formed -- lgamma(a + b) - lgamma(a) comes
    from the Stirling series of the difference -- so that nu = 1e7 costs no digits."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    tail = lambda z: (1.0 / z) * (1.0 / 12.0 - (1.0 / z) ** 2 * (1.0 / 360.0 - (1.0 / z) ** 2 * (1.0 / 1260.0 - (1.0 / z) ** 2 * (1.0 / 1680.0))))      # noqa: E731
    big = a >= 32.0
    ab = np.where(big, a, 32.0)
    d = (ab - 0.5) * np.log1p(b / ab) + b * np.log(ab + b) - b + (tail(ab + b) - tail(ab))
    return np.where(big, gammaln(b) - d, gammaln(a) + gammaln(b) - gammaln(a + b))


def student_t_tail(t, nu):
    """P(|T| > |t|) for T ~ t_nu = I_{nu / (nu + t^2)}(nu / 2, 1 / 2), elementwise in Float64 (t, nu broadcast), evaluated on the side
    of the incomplete beta function whose continued fraction converges fast."""
    t, nu = np.broadcast_arrays(np.asarray(t, np.float64), np.asarray(nu, np.float64))
    q = t * t
    a, b = 0.5 * nu, np.full(nu.shape, 0.5)
    out = np.ones(q.shape)
    pos = (q > 0) & np.isfinite(q)
    out[np.isinf(q)] = 0.0
    if pos.any():
        qq, aa, bb, nn = q[pos], a[pos], b[pos], nu[pos]
        x, xc = nn / (nn + qq), qq / (nn + qq)
        lpre = aa * -np.log1p(qq / nn) + bb * (np.log(qq) - np.log(nn + qq)) - _log_beta(aa, bb)
        low = x < (aa + 1.0) / (aa + bb + 2.0)
        res = np.empty(qq.shape)
        if low.any():
            res[low] = np.exp(lpre[low]) * _beta_cf(aa[low], bb[low], x[low]) / aa[low]
        if (~low).any():
            res[~low] = np.maximum(0.0, 1.0 - np.exp(lpre[~low]) * _beta_cf(bb[~low], aa[~low], xc[~low]) / bb[~low])
        out[pos] = res
    return out


def student_t_pdf(t, nu):
    """The density of t_nu at t, elementwise in Float64."""
    t, nu = np.asarray(t, np.float64), np.asarray(nu, np.float64)
    return np.exp(-_log_beta(0.5 * nu, 0.5) - 0.5 * np.log(nu) - 0.5 * (nu + 1) * np.log1p(t * t / nu))


def student_t_ppf(levels, nu):
    """z (K, L) Float64: z[k, q] the quantile of t_{nu_k} at levels[q], 0 < level < 1.  Exactly 0 at level 1 / 2 and antisymmetric:
    the quantile at a level above 1 / 2 is minus the one at 1 - level.  Solved on the lower tail, where tail / 2 = level does not cancel:
    Newton on the half tail from inside a bracket found by doubling, the midpoint whenever a step leaves the bracket."""
    levels = np.atleast_1d(np.asarray(levels, np.float64))
    nu = np.atleast_1d(np.asarray(nu, np.float64))
    if levels.ndim != 1 or nu.ndim != 1 or not np.all((levels > 0) & (levels < 1)) or not np.all(nu > 0):
        raise ValueError("student_t_ppf: levels inside (0, 1) and nu > 0 are needed")
    upper = levels > 0.5
    nu_all = nu
    nu, where = np.unique(nu_all, return_inverse=True)      # (clusters share a handful of df: each is solved once)
    p = np.broadcast_to(np.where(upper, 1.0 - levels, levels)[None, :], (len(nu), len(levels))).copy()      # <= 1 / 2: the lower tail's mass
    n2 = np.broadcast_to(nu[:, None], p.shape).copy()
    half = lambda t: 0.5 * student_t_tail(t, n2)      # noqa: E731  (P(T < -t), decreasing in t >= 0)
    lo, hi = np.zeros(p.shape), np.ones(p.shape)
    for _ in range(1100):
        far = half(hi) > p
        if not far.any():
            break
        lo, hi = np.where(far, hi, lo), np.where(far, 2.0 * hi, hi)
    t = 0.5 * (lo + hi)
    for _ in range(80):                                     # Newton doubles the digits; the tail itself is good to about 1e-15
        f = half(t) - p
        lo, hi = np.where(f > 0, t, lo), np.where(f > 0, hi, t)
        with np.errstate(all="ignore"):
            step = t + f / student_t_pdf(t, n2)
        nxt = np.where((step > lo) & (step < hi), step, 0.5 * (lo + hi))
        done = np.abs(nxt - t) <= 1e-14 * np.abs(t)
        t = nxt
        if done.all():
            break
    t = t[where.reshape(-1)]
    z = np.where(upper[None, :], t, -t)
    z[:, levels == 0.5] = 0.0
    return z
