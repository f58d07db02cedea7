"""Float64 reference of the imputation draws (include/dpmm_hip_impute.h, miss_draw_kernel of csrc/missing.hip) from the SAME random words,
computed two independent ways, the derived bound on what a correct kernel may differ from it by, the law checks and the inputs that
tests/test_impute_draws_cpu.py and tests/test_gpu_impute_draws.py share.  Pure numpy / scipy on top of tests/tools/missing_ref.py (the
marginal table, the bounds of y, t and q_o) and tests/tools/sample_ref.py (Philox, the uniforms, check_whitened); nothing here imports the
package.

Draw j of point i (global index idx):  u, n, g from the blocks 64 j + b of the streams 43, 44, 45;
  component        the first k with u < c_k, c_k the cumulative sums of p_k = exp(want_k - logsumexp) over the clusters with p_k > 0 (NaN -> 0);
                   none: the last such cluster; no cluster with p_k > 0: cluster 0
  precision side   C = R_k[:, M], A = C'C = L L', t = A^-1 C'y, q_o = |y - C t|^2;  x_M = (m_M - t) + sqrt((df + q_o) / g) L'^-1 n
  covariance side  Sigma = (R'R)^-1 explicitly, S = Sigma_MM - Sigma_MO Sigma_OO^-1 Sigma_OM, mean = m_M + Sigma_MO Sigma_OO^-1 z_O,
                   q_o = z_O' Sigma_OO^-1 z_O, and L the Cholesky factor of S^-1 (A = S^-1 is the block-inverse identity; the factor of an
                   SPD matrix is unique, so both sides form the same function of n)
with g ~ chi^2(df + D_o).  MUTATIONS are deliberately WRONG variants the tests must reject.

The bound of a drawn value x_a = c_a + s w_a (c = m_M - t, s = sqrt((df + q_o) / g), w = L'^-1 n), from Float64 quantities alone:
  |dc_a|  <= dcm_a                                        missing_ref.point_bounds: the Float32 error of y through t = A^-1 C'y
  |dw_a|  <= 2e-3 sum_b |(L'^-1)_ab| (1 + |n_b|)           the Float32 Box-Muller normals, |dn_b| < 1e-3 with room (tests/test_gpu_sample.py's
                                                          derivation: the fast log / sin / cos), pushed through the linear solve
  |ds|    <= s dq / (2 (df + q_o))                        dq as missing_ref.point_bounds forms it: 2 sum |res_i| e_i + sum e_i^2 + 2^-36 (q_o + |y|^2)
  2^-36 s sum_b |(L'^-1)_ab| |n_b|                        the Float64 steps (factor, back-substitution, g): 2^-53 cond(A), cond(A) thousands
  2^-23 |x_a|                                             the one rounding to Float32
bound_a = dcm_a + s (2e-3 sum_b |(L'^-1)_ab| (1 + |n_b|) + |w_a| dq / (2 (df + q_o)) + 2^-36 sum_b |(L'^-1)_ab| |n_b|) + 2^-23 |x_a| + 1e-37.

The component.  The GPU's table is Float32: its probabilities differ from the reference's by the relative `rel` of missing_ref.derived
(expm1(2 max_k bound_k) + 2^-23 (K + 16)), so its cumulative edge c_k lies within rel c_k + 2^-50 of the reference's.  A draw whose u is
that close to an edge may fall either way and is EXCUSED from the comparison of components; excused(...) counts them.
"""
import numpy as np
from scipy import stats
from scipy.linalg import solve_triangular
from scipy.special import logsumexp

from tools import missing_ref as mr
from tools import sample_ref as sr

STREAM_COMP, STREAM_NORMAL, STREAM_CHI = 43, 44, 45
BLOCKS = 64                                 # Philox blocks of a draw index
MUTATIONS = ("no_qo", "chi_df", "L_n", "plus_t", "draw_ignored", "unpatched")
FREQ_P = 1e-9                               # error probability of the component-frequency bound (check_frequencies)


# ------------------------------------------------------------------------------------------------ the random words
def uniform(idx, j, seed):
    w = sr.philox(seed, idx, BLOCKS * j, STREAM_COMP)
    return sr._u53(w[0], w[1])


def normals(idx, j, seed):
    """(len(idx), 16) Float64: block 64 j + b -> coordinates 4b .. 4b + 3, the Box-Muller of sample_ref.normals."""
    idx = np.asarray(idx, np.uint64)
    w = sr.philox(seed, idx[:, None], (BLOCKS * j + np.arange(4, dtype=np.uint64))[None, :], STREAM_NORMAL).astype(np.float64)
    u = (w + 0.5) / 4294967296.0
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    t0, t1 = 2 * np.pi * u[1], 2 * np.pi * u[3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=2).reshape(len(idx), 16)


def chi2(df, idx, seed, stream=STREAM_CHI, block0=0, rounds=8):
    """sample_ref.chi2 with the stream and the first block as parameters (stream 41, block 0: its bits -- the CPU test compares)."""
    idx = np.asarray(idx, np.uint64)
    a = 0.5 * np.asarray(df, np.float64) * np.ones(len(idx))
    boost = np.ones(len(idx))
    low = a < 1.0
    if low.any():
        ru = sr.philox(seed, idx, block0 + 63, stream)
        boost = np.where(low, sr._u53(ru[0], ru[1]) ** (1.0 / a), 1.0)
        a = np.where(low, a + 1.0, a)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    last, done = d.copy(), np.zeros(len(idx), bool)
    for t in range(rounds):
        rn, ru = sr.philox(seed, idx, block0 + 2 * t, stream), sr.philox(seed, idx, block0 + 2 * t + 1, stream)
        x = np.sqrt(-2.0 * np.log(sr._u53(rn[0], rn[1]))) * np.cos(2 * np.pi * sr._u53(rn[2], rn[3]))
        u = sr._u53(ru[0], ru[1])
        v = 1.0 + c * x
        pos = (v > 0.0) & ~done
        v = np.where(v > 0.0, v, 1.0) ** 3
        last = np.where(pos, d * v, last)
        acc = (u < 1.0 - 0.0331 * x ** 4) | (np.log(u) < 0.5 * x * x + d * (1.0 - v + np.log(v)))
        done |= pos & acc
    return 2.0 * last * boost


# ------------------------------------------------------------------------------------------------ the component
def probabilities(want):
    """(n, K) Float64 p_k of the columns of a (K, n) table, NaN entries -> 0 (a column without a finite entry: all 0)."""
    with np.errstate(all="ignore"):
        a = np.where(np.isnan(want), -np.inf, want)
        p = np.exp(a - logsumexp(a, axis=0)[None, :]).T
    return np.where(np.isfinite(p), p, 0.0)


def pick(p, u):
    """Inverse of the cumulative sums in cluster order over the clusters of positive probability: (component (n,), edges (n, K))."""
    c = np.cumsum(p, axis=1)
    pos = p > 0
    hit = pos & (u[:, None] < c)
    first = hit.argmax(1)
    last = np.where(pos.any(1), p.shape[1] - 1 - pos[:, ::-1].argmax(1), 0)
    return np.where(hit.any(1), first, last).astype(np.int32), c


def excused(p, u, rel):
    """(n,) bool: u within rel c_k + 2^-50 of a cumulative edge c_k of a cluster with p_k > 0."""
    c = np.cumsum(p, axis=1)
    return ((p > 0) & (np.abs(u[:, None] - c) <= rel[:, None] * c + 2.0 ** -50)).any(1)


# ------------------------------------------------------------------------------------------------ the draw
def _covariance_parts(x, miss, m, Sigma, k):
    M, O = np.flatnonzero(miss), np.flatnonzero(~miss)
    S, zO = Sigma[k], x[O] - m[k, O]
    Soo_inv_z = np.linalg.solve(S[np.ix_(O, O)], zO)
    Sc = S[np.ix_(M, M)] - S[np.ix_(M, O)] @ np.linalg.solve(S[np.ix_(O, O)], S[np.ix_(O, M)])
    return m[k, M] + S[np.ix_(M, O)] @ Soo_inv_z, np.linalg.cholesky(np.linalg.inv(Sc)), float(zO @ Soo_inv_z)


def draw(c, ref, idx, ndraws, seed, draw0=0, comp=None, mutate=None, side="precision", points=None, bounds=False, cache=None):
    """The draws draw0 .. draw0 + ndraws - 1 of the case `c` (missing_ref's keys) with its reference `ref` (missing_ref.reference).
    idx: the global index of every point.  comp (ndraws, n): take these components (the GPU's) in place of the reference's own.
    points: the positions to draw for (default: every marginalised point).  cache: a dict that keeps missing_ref.point_precision's parts
    of every point between calls on the same case.  Returns a dict:
      comp (ndraws, n) int32, -1 off the marginalised points;  u (ndraws, n);  p (n, K)
      x, bound {i: (ndraws, r)} (bound only with bounds=True);  parts {i: {k: (c (r,), L (r, r), q_o)}} of the clusters drawn."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(mutate)
    X64 = np.asarray(c["X"], np.float32).astype(np.float64)
    m64, df64 = (np.asarray(c[k], np.float32).astype(np.float64) for k in ("m", "df"))
    K, D = m64.shape
    R64 = np.asarray(c["R"], np.float32).astype(np.float64).reshape(K, D, D)
    ld64, w64 = (np.asarray(c[k], np.float32).astype(np.float64) for k in ("logdet", "w"))
    n = X64.shape[0]
    idx = np.asarray(idx, np.uint64)
    listed = np.flatnonzero(ref["listed"]) if points is None else np.asarray(points)
    want = np.full_like(ref["want"], np.nan) if mutate == "unpatched" else ref["want"]
    p = probabilities(want)
    js = [draw0 + (0 if mutate == "draw_ignored" else j) for j in range(ndraws)]
    u = np.stack([uniform(idx, j, seed) for j in js])
    own = np.full((ndraws, n), -1, np.int32)
    for jd in range(ndraws):
        own[jd, listed] = pick(p[listed], u[jd, listed])[0]
    use = own if comp is None else np.asarray(comp)
    nrm = np.stack([normals(idx[listed], j, seed) for j in js])                    # (ndraws, len(listed), 16)
    Do_l = D - ref["r"][listed]
    G = np.stack([chi2(df64[np.maximum(use[jd, listed], 0)] + (0.0 if mutate == "chi_df" else Do_l), idx[listed], seed, block0=BLOCKS * js[jd])
                  for jd in range(ndraws)])                                        # (ndraws, len(listed)): g ~ chi^2(df + D_o)
    Sigma = np.linalg.inv(np.einsum("kji,kjl->kil", R64, R64)) if side == "covariance" else None
    xs, bnd, parts = {}, {}, {}
    with np.errstate(all="ignore"):
        for li, i in enumerate(listed):
            i = int(i)
            miss = ref["miss"][i]
            M = np.flatnonzero(miss)
            r = len(M)
            pp = None
            if side == "precision":
                pp = cache.get(i) if cache is not None else None
                if pp is None:
                    pp = mr.point_precision(X64[i], miss, m64, R64, ld64, df64, w64)
                    if cache is not None:
                        cache[i] = pp
            if bounds:
                _, dcm = mr.point_bounds(pp, m64, R64, df64, D)
                e = (D + 2) * mr.U24 * np.einsum("kij,kj->ki", np.abs(R64), np.abs(pp["z"]))
                dq = 2 * (np.abs(pp["res"]) * e).sum(1) + (e * e).sum(1) + 2.0 ** -36 * (pp["q"] + (pp["y"] * pp["y"]).sum(1))
            xs[i], parts[i] = np.empty((ndraws, r)), {}
            bnd[i] = np.empty((ndraws, r))
            for k in np.unique(use[:, i]):
                k = int(k)
                if side == "precision":
                    C = R64[k][:, M]
                    cm, L, q = pp["cm"][k], np.linalg.cholesky(C.T @ C), pp["q"][k]
                    if mutate == "plus_t":
                        cm = m64[k, M] + pp["tsol"][k]
                else:
                    cm, L, q = _covariance_parts(X64[i], miss, m64, Sigma, k)
                parts[i][k] = (cm, L, q)
                sel = np.flatnonzero(use[:, i] == k)
                nv = nrm[sel, li, :r]                                              # (draws of this cluster, r)
                wv = nv @ L.T if mutate == "L_n" else solve_triangular(L.T, nv.T, lower=False).T
                g = G[sel, li]
                s = np.sqrt((df64[k] + (0.0 if mutate == "no_qo" else q)) / g)
                xs[i][sel] = cm[None, :] + s[:, None] * wv
                if bounds:
                    Li = np.abs(solve_triangular(L.T, np.eye(r), lower=False))      # |L'^-1|
                    bnd[i][sel] = (dcm[k][None, :] + s[:, None] * (2e-3 * (1 + np.abs(nv)) @ Li.T + np.abs(wv) * dq[k] / (2 * (df64[k] + q))
                                                                    + 2.0 ** -36 * np.abs(nv) @ Li.T) + mr.EPS * np.abs(xs[i][sel]) + 1e-37)
    return dict(comp=use.astype(np.int32), own=own, u=u, p=p, x=xs, bound=bnd, parts=parts)


# ------------------------------------------------------------------------------------------------ the law
def standardise(x, parts, comp, df, D):
    """u = L'(x_M - c) sqrt((df + D_o) / (df + q_o)) of one point: x (ndraws, r), comp (ndraws,), parts {k: (c, L, q_o)} -> (ndraws, r)."""
    out = np.empty_like(x, dtype=np.float64)
    r = x.shape[1]
    for k, (cm, L, q) in parts.items():
        sel = comp == k
        out[sel] = (np.asarray(x, np.float64)[sel] - cm[None, :]) @ L * np.sqrt((df[k] + D - r) / (df[k] + q))
    return out


def check_law(u, comp, dfc, min_pairs=1000):
    """u (points, ndraws, r) standardised draws, comp (points, ndraws) their clusters, dfc (K,) = df + D_o.  Raises AssertionError.
      * per cluster with at least min_pairs (point, draw) pairs: sample_ref.check_whitened(u, dfc[k]) -- under the law u = sqrt(dfc / g) n.
      * the draws of a point are independent: the sample correlation of coordinate a between draw j and draw j + 1 over the N points (both of
        the dominant cluster) is N(0, (dfc - 2) / ((dfc - 4) N)) as check_whitened derives for two coordinates; bound 6 / sqrt(N), 4e-9 each.
    Returns the clusters checked."""
    P, nd, r = u.shape
    checked = []
    for k in np.unique(comp):
        sel = comp == k
        if sel.sum() >= min_pairs:
            sr.check_whitened(u[sel], float(dfc[k]))
            checked.append(int(k))
    assert checked, "no cluster with enough draws"
    dom = np.bincount(comp.ravel()).argmax()
    for j in range(nd - 1):
        both = (comp[:, j] == dom) & (comp[:, j + 1] == dom)
        N = int(both.sum())
        for a in range(r):
            cc = np.corrcoef(u[both, j, a], u[both, j + 1, a])[0, 1]
            assert abs(cc) < 6.0 / np.sqrt(N), f"draws {j} and {j + 1}, coordinate {a}: correlation {cc:.4f} >= {6.0 / np.sqrt(N):.4f}"
    return checked


def check_frequencies(comp, p):
    """comp (points, ndraws) against p (points, K): O_k = the draws of cluster k, E_k = ndraws sum_i p_ik.  X^2 = sum_k (O_k - E_k)^2 / E_k over the
    clusters with E_k > 0 is, for draws from ONE probability vector, asymptotically chi^2(K' - 1); with the points' own vectors the
    variances p (1 - p) sum to less than the pooled one, so X^2 is stochastically smaller.  Bound: the 1 - FREQ_P quantile (FREQ_P = 1e-9)."""
    nd = comp.shape[1]
    E = nd * p.sum(0)
    live = E > 0
    O = np.bincount(comp.ravel(), minlength=p.shape[1]).astype(np.float64)
    assert O[~live].sum() == 0, "a cluster of probability 0 was drawn"
    x2 = float(((O[live] - E[live]) ** 2 / E[live]).sum())
    lim = float(stats.chi2(max(1, int(live.sum()) - 1)).isf(FREQ_P))
    assert x2 < lim, f"component frequencies: X^2 = {x2:.1f} >= {lim:.1f} (observed {O.tolist()}, expected {np.round(E, 1).tolist()})"
    return x2, lim


# ------------------------------------------------------------------------------------------------ inputs
LAW_CASES = ((64, 4, 60.0), (130, 3, 60.0), (17, 16, 60.0))      # (D, r, df): see law_case
LAW_POINTS, LAW_DRAWS = 2000, 10


def law_case(D, r, df, n=LAW_POINTS):
    """One dominant cluster and two near copies of it (the means moved a little: every point gives all three a real probability, about
    0.80 / 0.15 / 0.05), n points drawn from the dominant cluster's predictive, each with the same number r of gaps at random features.
    (64, 4) and (130, 3) have D_o >= df = 60: forgetting q_o or D_o in the scale about halves / doubles the variance of the standardised
    draws.  (17, 16) is r at the cap with D_o = 1: no df keeps D_o >= df and check_whitened's df + D_o >= 50 at once, so it keeps df = 60
    and stands for the 16 x 16 system, not for the scale (the CPU test shows which mutations each case rejects).  missing_ref's keys."""
    K = 3
    _, m, A, dfs = sr.niw_model(D, K, df, seed=1000 * D + r)
    rng = np.random.default_rng(77 * D + r)
    A[1:] = A[0]
    m[1:] = m[0] + 0.05 * rng.standard_normal((2, D)).astype(np.float32)
    # the predictive is t_df(m, A A'): R'R = (A A')^-1 with R upper triangular is R = inverse of the LOWER factor of A A', transposed twice:
    Sig = A[0] @ A[0].T
    R0 = np.linalg.cholesky(np.linalg.inv(Sig)).T                                   # upper, R'R = Sigma^-1
    R = np.repeat(R0[None], K, 0).astype(np.float32)
    logdet = (-2 * np.log(np.abs(np.einsum("kii->ki", R.astype(np.float64)))).sum(1)).astype(np.float32)
    w = np.array([0.80, 0.15, 0.05], np.float32)
    g = rng.chisquare(df, n)
    z = rng.standard_normal((n, D)) * np.sqrt(df / g)[:, None]
    X = (m[0][None, :] + np.linalg.solve(R0, z.T).T).astype(np.float32)
    gaps = {}
    for i in range(n):
        gaps[i] = sorted(int(j) for j in rng.choice(D, r, replace=False))
        X[i, gaps[i]] = np.nan
    return dict(D=D, K=K, n=n, X=X, m=m.astype(np.float32), R=R, logdet=logdet, df=np.full(K, df, np.float32), w=w, gaps=gaps)


def structure_case():
    """D = 5, K = 4 with one EMPTY cluster (weight 0: probability 0, never drawn), n = 133 = two 64-point tiles + 5, the gaps of
    missing_ref.make_case among its first 133 points (position 0: the first feature; 50: r = cap = 4; 52: every feature = cap + 1, over the
    cap; 53: NaN with +Inf; 60) and planted here: the last feature at position n - 1, two features each on both sides of the boundary
    between the 64-point trips of the list kernel (63, 64), 1 .. 3 gaps in every fifth point from 66 on."""
    c = mr.make_case(5, 4)
    n = 133
    X = c["X"][:n].copy()
    X[n - 1, 4] = np.nan
    X[63, [2, 3]] = np.nan
    X[64, [0, 4]] = np.nan
    rng = np.random.default_rng(133)
    for i in range(66, 131, 5):                                                    # thirteen more points with 1 .. 3 gaps, in every slab of 40
        X[i, rng.choice(5, int(rng.integers(1, 4)), replace=False)] = np.nan
    w = c["w"].astype(np.float64).copy()
    w[2] = 0.0
    c.update(X=X, n=n, w=(w / w.sum()).astype(np.float32), lab=c["lab"][:n], bulk=c["bulk"][:n], gaps={i: g for i, g in c["gaps"].items() if i < n})
    return c
