"""Float64 reference of mixture regression (include/dpmm_hip_regress.h, csrc/regress.hip): a direct evaluation of mean and std from
(p, tables, x), the header's bound from Float64 quantities alone, a second, independent form (the conditional law of every component from
the dense covariance, mixed), the mistakes the bound has to catch, and the inputs of tests/test_gpu_regress.py.  Pure numpy: nothing here
imports the package or needs a GPU.

    mu_ikd = c_kd + sum_e B_kde x_ie              mean_id = sum_k p_ik mu_ikd
    s_ik   = (df_k + q_ik) / (df_k + D_o - 2)     var_id  = sum_k p_ik (s_ik V_kd + mu_ikd^2) - mean_id^2,   std = sqrt(max(0, var))
with p the Float32 probabilities the GPU returned, q_ik = |R_k (x_i - m_k)|^2 of the marginal model in Float64.  The bound is the header's:
    a_ikd = |c_kd| + sum_e |B_kde| |x_ie|,   |mean - exact| <= (D_o + 4) u sum_k p_ik a_ikd,   u = 2^-24
    d_ik = (D_o + 3) u a_ikd,   t_ik a bound on the error of the table entry (predictive_ref.error_bound)
    |var - exact| <= sum_k p_ik [s_ik V_kd (expm1(2 t_ik / (df_k + D_o)) + 3 u) + 2 d_ik |mu_ikd - mean| + d_ik^2] + (sum_k p_ik d_ik)^2
                     + (K + 4) 2^-52 (sum_k p_ik (s_ik V_kd + mu_ikd^2) + mean^2)
    |std - exact| <= min(sqrt(dv), dv / exact std) + 2 u exact std
"""
import types

import numpy as np

U24 = 2.0 ** -24
MUTATIONS = ("sign_of_B", "m_O_not_subtracted", "s_with_D", "no_between_term", "given_order_ignored")


def quad(x, m, R):
    """q (n, K) = |R_k (x_i - m_k)|^2 in Float64; x (n, D_o), m (K, D_o), R (K, D_o, D_o)."""
    z = x[:, None, :] - m[None, :, :]
    y = np.einsum("kij,nkj->nki", R, z)
    return (y * y).sum(-1)


def reference(p, B, c, V, df, q, x, t=None, mutation=None, D_full=None, m_O=None):
    """dict(mean, std (n, D_t), mean_bound, var_bound, std_bound) from p (n, K), the Float64 tables, df (K,), q (n, K), x (n, D_o).
    t (n, K): bounds on the table entries' errors (None: 0).  mutation: one of MUTATIONS, applied to the evaluation (not to the bound)."""
    p, B, c, V, df, q, x = (np.asarray(a, np.float64) for a in (p, B, c, V, df, q, x))
    n, K = p.shape
    Do = x.shape[1]
    Bm, cm, xm = B, c, x
    if mutation == "sign_of_B":
        Bm = -B
    if mutation == "m_O_not_subtracted":          # c = m_M - B m_O: without the subtraction c = m_M, i.e. the mean is m_M + B x
        cm = c + np.einsum("kde,ke->kd", B, np.asarray(m_O, np.float64))
    if mutation == "given_order_ignored":
        xm = np.sort(x, axis=1)
    Ds = D_full if mutation == "s_with_D" else Do
    with np.errstate(all="ignore"):
        mu = cm[None, :, :] + np.einsum("kde,ne->nkd", Bm, xm)                       # (n, K, D_t)
        s = (df[None, :] + q) / (df[None, :] + Ds - 2.0)
        pk = p[:, :, None]
        live = pk != 0
        mean = np.where(live, pk * mu, 0.0).sum(1)
        within = np.where(live, pk * s[:, :, None] * V[None, :, :], 0.0).sum(1)
        e2 = within + np.where(live, pk * mu * mu, 0.0).sum(1)
        var = within if mutation == "no_between_term" else e2 - mean * mean
        std = np.sqrt(np.maximum(var, 0.0))
        # ---- the bound, from the unmutated Float64 quantities
        mu0 = c[None, :, :] + np.einsum("kde,ne->nkd", B, x)
        a = np.abs(c)[None, :, :] + np.einsum("kde,ne->nkd", np.abs(B), np.abs(x))
        pa = np.where(live, pk * a, 0.0).sum(1)
        mean_bound = (Do + 4) * U24 * pa
        d = (Do + 3) * U24 * a
        tt = np.zeros_like(q) if t is None else np.asarray(t, np.float64)
        rel = np.expm1(2.0 * tt / (df[None, :] + Do))[:, :, None] + 3 * U24
        s0 = ((df[None, :] + q) / (df[None, :] + Do - 2.0))[:, :, None]
        mean0 = np.where(live, pk * mu0, 0.0).sum(1)
        per = s0 * V[None, :, :] * rel + 2 * d * np.abs(mu0 - mean0[:, None, :]) + d * d
        e20 = np.where(live, pk * (s0 * V[None, :, :] + mu0 * mu0), 0.0).sum(1)
        var_bound = (np.where(live, pk * per, 0.0).sum(1) + np.where(live, pk * d, 0.0).sum(1) ** 2
                     + (K + 4) * 2.0 ** -52 * (e20 + mean0 * mean0))
        std0 = np.sqrt(np.maximum(e20 - mean0 * mean0, 0.0))
        std_bound = np.minimum(np.sqrt(var_bound), var_bound / np.maximum(std0, 1e-300)) + 2 * U24 * std0
    return dict(mean=mean, std=std, var=var, mean_bound=mean_bound, var_bound=var_bound, std_bound=std_bound)


def weights(counts, alpha=10.0):
    w = np.asarray(counts, np.float64) + alpha
    return w / w.sum()


def marginal_logdens(post, w, given, x):
    """(n, K): log w_k + the log-density of x (n, D_o) under the marginal over `given` of cluster k's Student-t predictive
    t_df(m, c Psi), c = (kappa + 1) / (kappa df), df = nu - D + 1, from the dense scale matrix -- the closed form, no closure rule."""
    from scipy.special import gammaln
    O = np.asarray(given)
    x = np.asarray(x, np.float64)
    K, D = post["m"].shape
    Do = len(O)
    out = np.empty((len(x), K))
    for k in range(K):
        df = post["nu"][k] - D + 1
        S = ((post["kappa"][k] + 1) / (post["kappa"][k] * df)) * (post["U"][k] @ post["U"][k].T)
        Soo = S[np.ix_(O, O)]
        z = x - post["m"][k, O]
        q = np.einsum("ne,ef,nf->n", z, np.linalg.inv(Soo), z)
        out[:, k] = (gammaln(0.5 * (df + Do)) - gammaln(0.5 * df) - 0.5 * Do * np.log(df * np.pi) - 0.5 * np.linalg.slogdet(Soo)[1]
                     - 0.5 * (df + Do) * np.log1p(q / df) + np.log(w[k]))
    return out


def dense_form(p, m, R, df, given, targets, x):
    """The second form: per component the conditional mean m_M + S_MO S_OO^-1 (x - m_O) and the conditional variance
    (df + q) / (df + D_o - 2) diag(S_MM - S_MO S_OO^-1 S_OM) from the dense scale matrix S = (R'R)^-1 of the joint model (m (K, D),
    R (K, D, D) over all D features), mixed with p.  (mean, std)."""
    p, m, R, df, x = (np.asarray(a, np.float64) for a in (p, m, R, df, x))
    O, M = np.asarray(given), np.asarray(targets)
    n, K = p.shape
    mean = np.zeros((n, len(M)))
    e2 = np.zeros((n, len(M)))
    for k in range(K):
        S = np.linalg.inv(R[k].T @ R[k])
        Soo, Smo, Smm = S[np.ix_(O, O)], S[np.ix_(M, O)], S[np.ix_(M, M)]
        G = Smo @ np.linalg.inv(Soo)
        z = x - m[k, O]
        q = np.einsum("ne,ef,nf->n", z, np.linalg.inv(Soo), z)
        mu = m[k, M] + z @ G.T
        v = ((df[k] + q) / (df[k] + len(O) - 2.0))[:, None] * np.diag(Smm - G @ Smo.T)[None, :]
        mean += p[:, k:k + 1] * mu
        e2 += p[:, k:k + 1] * (v + mu * mu)
    return mean, np.sqrt(np.maximum(e2 - mean * mean, 0.0))


# ------------------------------------------------------------------------------------------------ inputs
TILE = 32                      # points per workgroup of regress.hip
SHAPES = ((1, 1), (3, 2), (16, 17), (33, 31), (64, 64), (65, 63), (100, 156), (255, 1), (1, 255))
# K = 1 and 3 everywhere; 24 clusters where the walk over the clusters is the point (a small, a middle and a wide shape)
CASES = tuple((do, dt, k) for do, dt in SHAPES for k in (1, 3)) + ((3, 2, 24), (33, 31, 24), (64, 64, 24))


def make_posterior(D, K, seed):
    """A hand-made NIW posterior over D features: clusters 40 standard deviations apart along a random direction each, the last one
    1e4 standard deviations from the origin in every coordinate (K >= 2)."""
    rng = np.random.default_rng(seed)
    kappa = rng.uniform(5.0, 50.0, K)
    df = np.array([5.25, 5.25, 300.0, 30.0])[np.arange(K) % 4]
    nu = df + D - 1
    s = rng.uniform(0.7, 1.6, K)
    s[:2] = s[0]        # clusters 0 and 1 are alike but for their means: at the point between them where their entries are equal the two
                        # conditional laws have about the same spread, and the mixture's exceeds it by the distance of their means
    off = 0.05 if D <= 64 else 0.02
    U = (np.eye(D) + off * np.triu(rng.standard_normal((K, D, D)), 1)) * (s * np.sqrt(df))[:, None, None]      # Psi about df s^2 I: Sigma about s^2 I
    m = rng.standard_normal((K, D)) + 40.0 * np.arange(K)[:, None] * s.max() * np.sign(rng.standard_normal((K, D)))
    if K >= 2:
        m[K - 1] = 1e4 * s[K - 1] * np.sign(rng.standard_normal(D))
    m = m.astype(np.float32).astype(np.float64)
    post = dict(kappa=kappa, nu=nu, m=m, U=U, logdet_psi=2 * np.log(np.einsum("kii->ki", U)).sum(1) - D * np.log(nu))
    return post, s


def dummy_model(post, K, D, counts=None, hyper=True):
    """What a Predictor reads of a fitted model: rows 3k of the sampler's posterior arrays."""
    rows = {k: np.repeat(np.asarray(v), 3, axis=0) for k, v in post.items()}
    prior = types.SimpleNamespace(kind=0, dim=D)
    if hyper:
        prior.kappa, prior.m, prior.nu, prior.psi = 1.0, np.zeros(D), D + 3.0, np.eye(D)
    s = types.SimpleNamespace(K=K, prior=prior, post=rows, alpha=10.0, points_count=np.asarray(counts if counts is not None else 10 + 5 * np.arange(K)),
                              wk=types.SimpleNamespace(device=0))
    return types.SimpleNamespace(sampler=s)


def make_case(Do, Dt, K, scramble=True):
    """One case: the posterior over D = D_o + D_t features, `given` and `targets` in scrambled order, n = 2 tiles + 5 points of the given
    features (n, D_o) Float32 drawn from the clusters, with the planted points: cluster means at the first and the last position and on
    both sides of the tile boundary, the point between clusters 0 and 1 where their entries are equal (K >= 2), a point at cluster 0's mean -- 40 standard deviations
    from every other cluster, whose probabilities underflow to 0 -- and points of the cluster 1e4 standard deviations out."""
    D = Do + Dt
    post, s = make_posterior(D, K, 1009 * Do + 31 * Dt + K)
    rng = np.random.default_rng(7 * Do + Dt + 100 * K)
    perm = rng.permutation(D) if scramble else np.arange(D)
    given, targets = [int(f) for f in perm[:Do]], [int(f) for f in perm[Do:]]
    n = 2 * TILE + 5
    lab = rng.integers(0, K, n)
    lab[[0, TILE - 1, TILE, n - 1]] = [0, K - 1, 0, K - 1]
    X = post["m"][lab][:, given] + s[lab][:, None] * rng.standard_normal((n, Do))
    planted = dict(mean=[0, TILE - 1, TILE, n - 1], alone=3, far=[TILE - 1, n - 1] if K >= 2 else [])
    for i in planted["mean"] + [planted["alone"]]:
        X[i] = post["m"][lab[i] if i != planted["alone"] else 0][given]
    lab[planted["alone"]] = 0
    if K >= 2:
        planted["mid"] = 5
        w = weights(10 + 5 * np.arange(K))
        a, b = post["m"][0][given], post["m"][1][given]
        lo, hi = 0.0, 1.0
        for _ in range(60):      # the point of the segment where the two entries are equal: both probabilities about a half
            mid = 0.5 * (lo + hi)
            l = marginal_logdens(post, w, given, (a + mid * (b - a))[None, :])[0]
            lo, hi = (mid, hi) if l[0] > l[1] else (lo, mid)
        X[5] = a + lo * (b - a)
    return dict(Do=Do, Dt=Dt, D=D, K=K, n=n, post=post, given=given, targets=targets, X=X.astype(np.float32), lab=lab, planted=planted, s=s)
