"""Float64 reference of the draws of the targets (include/dpmm_hip_regress_draw.h, csrc/regress_draw.hip) from the SAME random words, computed
two independent ways, the derived bound on what a correct kernel may differ from it by, the law check and the inputs that
tests/test_regress_draws_cpu.py and tests/test_gpu_regress_draws.py share.  Pure numpy / scipy on top of tests/tools/regress_ref.py,
tests/tools/sample_ref.py (Philox, the uniforms) and tests/tools/impute_draw_ref.py (chi2, the component pick); nothing here imports the
package.

Draw j of point i (global index idx): u, n, g from the blocks 64 j + b of the streams 46, 47, 48;
  component        impute_draw_ref.pick: the first k with u < c_k, c_k the Float64 cumulative sums of p_k over the clusters with p_k > 0
  both sides start from the FULL Sigma_k = (R_k'R_k)^-1 of the joint model over given + targets (O the first D_o features, M the rest):
  precision side   A = Sigma^-1, A_MM = L L', W = (L^-1)';  mu = m_M - A_MM^-1 A_MO (x - m_O)
  covariance side  S = Sigma_MM - Sigma_MO Sigma_OO^-1 Sigma_OM and its own factorisation S = W W', W upper triangular (the Cholesky factor
                   of S with rows and columns reversed, reversed back: the upper factor with a positive diagonal is unique, and
                   S = A_MM^-1 is the block-inverse identity);  mu = m_M + Sigma_MO Sigma_OO^-1 (x - m_O)
  then             q = (x - m_O)' Sigma_OO^-1 (x - m_O),  s = sqrt((df + q) / g),  g ~ chi^2(df + D_o),  x_M = mu + s W n.
MUTATIONS are deliberately WRONG variants the tests must reject.

The bound of a drawn value x_a = mu_a + s (W n)_a, from Float64 quantities alone (u = 2^-24):
  (D_o + D_t + 4) u (|c_a| + sum_e |B_ae| |x_e| + s sum_b |W_ab| |n_b|)
                        the Float32 chain: the roundings of c, B, W (one u), its at most D_o + D_t steps (one u each), the product s n_b (one
                        u) and room for the rounding of s itself; every term is bounded by the sum of the absolute values of the chain's terms
  s 2e-3 sum_b |W_ab| (1 + |n_b|)
                        the Float32 Box-Muller normals, |dn_b| < 1e-3 with room (the fast log / sin / cos; impute_draw_ref takes the same)
  s |(W n)_a| expm1(2 t_ik / (df + D_o)) / 2
                        the scale: q is recovered from the table entry, whose error is at most t_ik (predictive_ref.error_bound);
                        dq / dparr = -2 (df + q) / (df + D_o), so df + q moves by the factor expm1(2 t / (df + D_o)) at most and its root by half
  2^-23 |x_a| + 1e-37   the last rounding.

The component.  The GPU's table is Float32: its probabilities differ from the reference's by the relative rel_i = expm1(2 max_k t_ik) +
2^-23 (K + 16), so a cumulative edge c_k lies within rel c_k + 2^-50 of the reference's.  A draw whose u is that close to an edge may fall
either way and is EXCUSED (impute_draw_ref.excused); a test may excuse at most 1 % of its draws (MAX_EXCUSED).
"""
import numpy as np
from scipy import stats

from tools import impute_draw_ref as idr
from tools import regress_ref as rr
from tools import sample_ref as sr

STREAM_COMP, STREAM_NORMAL, STREAM_CHI = 46, 47, 48
BLOCKS = 64
U24 = 2.0 ** -24
MAX_EXCUSED = 0.01
MUTATIONS = ("no_q", "chi_df", "Li_not_transposed", "draw_ignored", "stream_44", "sign_of_B")
KS_LAMBDA = 1.95                            # the asymptotic 0.1 % critical value of sqrt(n) D_n


# ------------------------------------------------------------------------------------------------ the random words
def uniform(idx, j, seed):
    w = sr.philox(seed, np.asarray(idx, np.uint64), BLOCKS * j, STREAM_COMP)
    return sr._u53(w[0], w[1])


def normals(idx, j, Dt, seed, stream=STREAM_NORMAL):
    """(len(idx), D_t) Float64: block 64 j + b -> coordinates 4b .. 4b + 3, the Box-Muller of sample_ref.normals."""
    idx = np.asarray(idx, np.uint64)
    nb4 = (Dt + 3) // 4
    w = sr.philox(seed, idx[:, None], (BLOCKS * j + np.arange(nb4, dtype=np.uint64))[None, :], stream).astype(np.float64)
    u = (w + 0.5) / 4294967296.0
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    t0, t1 = 2 * np.pi * u[1], 2 * np.pi * u[3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=2).reshape(len(idx), 4 * nb4)[:, :Dt]


# ------------------------------------------------------------------------------------------------ the two sides
def tables(m, R, Do, side="precision"):
    """dict(B (K, D_t, D_o), c (K, D_t), W (K, D_t, D_t) upper triangular, Soo_inv (K, D_o, D_o), S (K, D_t, D_t) = W W') from the joint
    model m (K, D), R (K, D, D) with Sigma^-1 = R'R, the given features first."""
    m = np.asarray(m, np.float64)
    K, D = m.shape
    R = np.asarray(R, np.float64).reshape(K, D, D)
    Sigma = np.linalg.inv(np.einsum("kji,kjl->kil", R, R))
    Sigma = 0.5 * (Sigma + Sigma.transpose(0, 2, 1))
    Soo, Smo, Smm = Sigma[:, :Do, :Do], Sigma[:, Do:, :Do], Sigma[:, Do:, Do:]
    Soo_inv = np.linalg.inv(Soo)
    if side == "precision":
        A = np.linalg.inv(Sigma)
        A = 0.5 * (A + A.transpose(0, 2, 1))
        L = np.linalg.cholesky(A[:, Do:, Do:])
        Li = np.linalg.inv(L)
        W = Li.transpose(0, 2, 1)
        B = -np.einsum("kij,kjl->kil", np.einsum("kij,kjl->kil", W, Li), A[:, Do:, :Do])
        S = np.einsum("kij,klj->kil", W, W)
    elif side == "covariance":
        B = np.einsum("kij,kjl->kil", Smo, Soo_inv)
        S = Smm - np.einsum("kij,klj->kil", B, Smo)
        S = 0.5 * (S + S.transpose(0, 2, 1))
        W = np.linalg.cholesky(S[:, ::-1, ::-1])[:, ::-1, ::-1]
    else:
        raise ValueError(side)
    c = m[:, Do:] - np.einsum("kij,kj->ki", B, m[:, :Do])
    return dict(B=B, c=c, W=np.ascontiguousarray(W), Soo_inv=Soo_inv, S=S, m_O=m[:, :Do])


def draw(X, m, R, df, want, idx, ndraws, seed, draw0=0, comp=None, t=None, side="precision", mutate=None, q=None):
    """The draws draw0 .. draw0 + ndraws - 1.  X (n, D_o) the given features (Float32 values), m, R the joint model (given features first),
    df (K,), want (K, n) the Float64 marginal table, idx the global index of every point, comp (ndraws, n): take these components (the
    GPU's) in place of the reference's own, t (n, K) the bounds of the table entries' errors (None: 0), q (n, K): the quadratic forms of the
    MARGINAL model the table was made from (None: those of the joint model's Sigma_OO -- the same until `marginal.absorb` moves the marginal
    model, after which probabilities, h, df and q follow it while c + B x and W stay the joint model's).  Points whose column of `want`
    has a NaN or no finite entry, or with a feature that is not finite, take no part.  Returns dict(x, bound (ndraws, n, D_t) -- NaN off
    the points that take part --, own, comp (ndraws, n) int32, u (ndraws, n), p (n, K), part (n,), q (n, K), s (ndraws, n))."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(mutate)
    X = np.asarray(X, np.float32).astype(np.float64)
    n, Do = X.shape
    tb = tables(m, R, Do, side)
    K, Dt = tb["c"].shape
    df = np.asarray(df, np.float64)
    idx = np.asarray(idx, np.uint64)
    with np.errstate(all="ignore"):
        part = np.isfinite(X).all(1) & ~np.isnan(want).any(0) & np.isfinite(want).any(0) & ~np.isposinf(want).any(0)
    p = idr.probabilities(want)
    tt = np.zeros((n, K)) if t is None else np.asarray(t, np.float64)
    B = -tb["B"] if mutate == "sign_of_B" else tb["B"]
    W = tb["W"].transpose(0, 2, 1) if mutate == "Li_not_transposed" else tb["W"]
    with np.errstate(all="ignore"):
        z = X[:, None, :] - tb["m_O"][None, :, :]
        q = np.einsum("nke,kef,nkf->nk", z, tb["Soo_inv"], z) if q is None else np.asarray(q, np.float64)
        mu = tb["c"][None] + np.einsum("kde,ne->nkd", B, X)                          # (n, K, D_t)
        amu = np.abs(tb["c"])[None] + np.einsum("kde,ne->nkd", np.abs(tb["B"]), np.abs(X))
    x = np.full((ndraws, n, Dt), np.nan)
    bound = np.full((ndraws, n, Dt), np.nan)
    own = np.full((ndraws, n), -1, np.int32)
    us = np.empty((ndraws, n))
    ss = np.full((ndraws, n), np.nan)
    P = np.flatnonzero(part)
    for jd in range(ndraws):
        j = draw0 + (0 if mutate == "draw_ignored" else jd)
        us[jd] = uniform(idx, j, seed)
        own[jd, P] = idr.pick(p[P], us[jd, P])[0]
        use = own[jd] if comp is None else np.asarray(comp[jd])
        k = np.maximum(use[P], 0)
        nv = normals(idx[P], j, Dt, seed, stream=44 if mutate == "stream_44" else STREAM_NORMAL)
        g = idr.chi2(df[k] + (0.0 if mutate == "chi_df" else Do), idx[P], seed, stream=STREAM_CHI, block0=BLOCKS * j)
        qk = q[P, k]
        s = np.sqrt((df[k] + (0.0 if mutate == "no_q" else qk)) / g)
        wn = np.einsum("pab,pb->pa", W[k], nv)
        x[jd, P] = mu[P, k] + s[:, None] * wn
        ss[jd, P] = s
        aW = np.abs(tb["W"][k])
        bound[jd, P] = ((Do + Dt + 4) * U24 * (amu[P, k] + s[:, None] * np.einsum("pab,pb->pa", aW, np.abs(nv)))
                        + s[:, None] * 2e-3 * np.einsum("pab,pb->pa", aW, 1 + np.abs(nv))
                        + s[:, None] * np.abs(wn) * (np.expm1(2 * tt[P, k] / (df[k] + Do)) / 2)[:, None]
                        + 2.0 ** -23 * np.abs(x[jd, P]) + 1e-37)
    used = own if comp is None else np.asarray(comp, np.int32)
    return dict(x=x, bound=bound, own=own, comp=used, u=us, p=p, part=part, q=q, s=ss, tables=tb)


def relative_table_error(t, K):
    """rel_i of the docstring from t (n, K)."""
    return np.expm1(2 * np.asarray(t, np.float64).max(1)) + 2.0 ** -23 * (K + 16)


def compare(got, got_comp, ref, rel):
    """The comparison the GPU test makes: got (ndraws, n, D_t) values and got_comp (ndraws, n) components against `ref` = draw(..., comp=
    got_comp) whose `own` are the reference's components.  Returns (worst |got - x| / bound over the points that take part, the fraction of
    the draws excused, the number of component mismatches that are NOT excused); NaN exactly where a point takes no part is part of it."""
    part = ref["part"]
    got = np.asarray(got, np.float64)
    assert np.isnan(got[:, ~part]).all() and (np.asarray(got_comp)[:, ~part] == -1).all(), "a point that takes no part was drawn for"
    if not part.any():
        return 0.0, 0.0, 0
    assert np.isfinite(got[:, part]).all(), "a point that takes part has a value that is not finite"
    ratio = float((np.abs(got[:, part] - ref["x"][:, part]) / ref["bound"][:, part]).max())
    exc = np.stack([idr.excused(ref["p"][part], ref["u"][jd, part], np.asarray(rel)[part]) for jd in range(got.shape[0])])
    wrong = (np.asarray(got_comp)[:, part] != ref["own"][:, part]) & ~exc
    return ratio, float(exc.mean()), int(wrong.sum())


# ------------------------------------------------------------------------------------------------ the law
def law_statistic(x, mu, S, df, q, Do):
    """r' A_MM r (df + D_o) / ((df + q) D_t) of every (draw, point) of a one-cluster model: x (ndraws, n, D_t), mu (n, D_t), S = (A_MM)^-1
    (D_t, D_t), q (n,).  Under the law it is F(D_t, df + D_o)."""
    r = np.asarray(x, np.float64) - mu[None]
    Dt = r.shape[-1]
    quad = np.einsum("jna,ab,jnb->jn", r, np.linalg.inv(S), r)
    return quad * (df + Do) / ((df + q)[None, :] * Dt)


def check_law(stat, Dt, dfo):
    """Kolmogorov distance of the statistic against F(D_t, df + D_o) below 1.95 / sqrt(N).  Returns (distance, limit)."""
    s = np.asarray(stat, np.float64).ravel()
    d = sr.ks_distance(s, stats.f(Dt, dfo).cdf)
    lim = KS_LAMBDA / np.sqrt(len(s))
    assert d < lim, f"r'A r (df + D_o) / ((df + q) D_t) against F({Dt}, {dfo}): KS distance {d:.5f} >= {lim:.5f}"
    return d, lim


# ------------------------------------------------------------------------------------------------ inputs
TILE = 32
N = 2 * TILE + 5
CASES = rr.CASES
LAW_SHAPES = ((3, 2), (33, 31))
LAW_POINTS, LAW_DRAWS = 256, 64
LAW_SEED = {(3, 2): 1, (33, 31): 1}          # seeds for which the reference itself passes check_law (tests/test_regress_draws_cpu.py checks)
SEED = 2024                                  # the seed of the comparison tests: the reference alone excuses below 1 % with it (checked there)
# ... but for the cases whose table error is large against the width of a cluster's share of [0, 1) (rel = 0.02 at D_o = 255, 24 edges at
# K = 24): the first seed from 2024 on for which the reference alone stays within 1 %
CASE_SEED = {(255, 1, 1): 2032, (255, 1, 3): 2032, (64, 64, 24): 2027}


def case_seed(Do, Dt, K):
    return CASE_SEED.get((Do, Dt, K), SEED)


def make_posterior(D, K, seed):
    """A hand-made NIW posterior over D features with OVERLAPPING clusters: the means about 1.5 standard deviations apart in all, so that
    every point gives several clusters a real probability whatever D_o is and a tile of 32 points holds several components."""
    rng = np.random.default_rng(seed)
    kappa = rng.uniform(5.0, 50.0, K)
    df = np.array([5.25, 300.0, 30.0, 8.0])[np.arange(K) % 4]
    nu = df + D - 1
    s = rng.uniform(0.8, 1.3, K)
    off = 0.05 if D <= 64 else 0.02
    U = (np.eye(D) + off * np.triu(rng.standard_normal((K, D, D)), 1)) * (s * np.sqrt(df))[:, None, None]
    m = rng.standard_normal(D)[None, :] + 1.5 / np.sqrt(D) * rng.standard_normal((K, D))
    m = m.astype(np.float32).astype(np.float64)
    return dict(kappa=kappa, nu=nu, m=m, U=U, logdet_psi=2 * np.log(np.einsum("kii->ki", U)).sum(1) - D * np.log(nu)), s


def make_case(Do, Dt, K, n=N, scramble=True):
    """One case: the posterior over D = D_o + D_t features, `given` and `targets` in scrambled order, n points of the given features
    (n, D_o) Float32 drawn from the clusters."""
    D = Do + Dt
    post, s = make_posterior(D, K, 977 * Do + 29 * Dt + K)
    rng = np.random.default_rng(5 * Do + Dt + 100 * K)
    perm = rng.permutation(D) if scramble else np.arange(D)
    given, targets = [int(f) for f in perm[:Do]], [int(f) for f in perm[Do:]]
    lab = rng.integers(0, K, n)
    X = post["m"][lab][:, given] + s[lab][:, None] * rng.standard_normal((n, Do))
    return dict(Do=Do, Dt=Dt, D=D, K=K, n=n, post=post, given=given, targets=targets, X=X.astype(np.float32), lab=lab, s=s)
