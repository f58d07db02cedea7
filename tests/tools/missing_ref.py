"""Float64 reference of scoring and imputing points with MISSING (NaN) features under the Student-t predictive (include/dpmm_hip_missing.h,
csrc/missing.hip), computed two independent ways, a derived bound on what a correct kernel may differ from it by, the inputs of
tests/test_gpu_missing.py and a numpy restatement of the kernel with the mistakes the bound has to catch (tests/test_missing_cpu.py).
Pure numpy / scipy, on top of tests/tools/predictive_ref.py (complete points are its business); nothing here imports the package.

Cluster k's predictive is t_df(m, Sigma), Sigma^-1 = R'R.  A point with missing set M (r = |M| NaN features, observed set O, D_o = D - r):
  precision side   z = x - m on O, 0 on M;  y = R z;  C = R[:, M];  g = C'y;  A = C'C;  t = A^-1 g;  q_o = |y - C t|^2;
                   want = lgamma((df + D_o)/2) - lgamma(df/2) - D_o/2 log(df pi) - (logdet + logdet A)/2 - (df + D_o)/2 log1p(q_o/df) + log w
                   E[x_M | x_O] = m_M - t
  covariance side  Sigma = (R'R)^-1 explicitly: scipy's multivariate_t.logpdf(x_O; m_O, Sigma_OO, df) + log w and m_M + Sigma_MO Sigma_OO^-1 z_O.
(y - C t = P y with P the orthogonal projector onto the complement of span C; |P y|^2 = z_O' (Sigma_OO)^-1 z_O and det Sigma_OO = det Sigma det A
are the block-inverse identities.)

The bound of an entry, from Float64 quantities only (u = 2^-24).  The kernel forms z and y in Float32 and everything behind them in Float64:
  |y_i - fl(y_i)| <= e_i = (D + 2) u sum_j |R_ij| |z_j|                    as predictive_ref: one subtraction, a product and an addition per term
  q_o = |P y|^2:  |P(y + d)|^2 - |P y|^2 = 2 (P y).d + |P d|^2 and |P d| <= |d|, so
      dq = 2 sum_i |(P y)_i| e_i + sum_i e_i^2 + 2^-36 (q_o + |y|^2)       the last term: the Float64 steps (g, A, its factor, t, the residual)
                                                                           err by some 2^-53 cond(A) relative to |y|^2 -- cond(A) <= cond(R)^2,
                                                                           thousands here -- which is why they are Float64: in Float32 this
                                                                           term would be 2^-24 cond(A) |y|^2 and swamp the first two
  bound = hdf_o dq / (df + q_o) + 2^-21 (|cst_o| + hdf_o log1p(q_o / df)) + 1e-6      the roundings of the constant and the log1p term as in
                                                                           predictive_ref (cst_o includes -logdet A / 2)
The bound of a conditional mean c_a = m_a - t_a:  t = B y with B = A^-1 C' (r x D), so |dt_a| <= sum_i |B_ai| e_i + 2^-36 (|t_a| + sum_i |B_ai| |y_i|),
and of an imputed value sum_k p_k c_k (p_k the probabilities, whose logarithms are off by at most 2 max_k bound_k + the finish kernel's
2^-23 (K + 16)):  sum_k p_k dt_k + sum_k p_k (expm1(2 max bound) + 2^-23 (K + 16)) |c_k - v| + 2^-23 |v|, v the Float64 value (the
probabilities sum to 1 on both sides, so only the spread of the c_k about v counts, twice over for the renormalisation).
"""
import numpy as np
from scipy.special import gammaln, logsumexp
from scipy.stats import multivariate_t

from tools import predictive_ref as pref

U24 = 2.0 ** -24
EPS = 2.0 ** -23
MAX_MISSING = 16
# (D, K) of tests/test_gpu_missing.py: every NT = ceil(D / 64) of the patch kernel with its edges, the tile sizes of the sweep, many clusters
CASES = tuple((D, 3) for D in (2, 5, 16, 17, 33, 64, 65, 128, 256)) + ((24, 60),)
MUTATIONS = ("exp_D", "cst_D", "no_logdetA", "logdetA_sign", "z_not_zeroed", "plus_t", "f32_difference")


def cap_of(D):
    return min(MAX_MISSING, D - 1)


def classify(X):
    """(miss (n, D) bool, r (n,), listed (n,) bool: 1 <= r <= cap, over (n,) bool: r > cap)."""
    miss = np.isnan(np.asarray(X))
    r = miss.sum(1)
    cap = cap_of(miss.shape[1])
    return miss, r, (r >= 1) & (r <= cap), r > cap


def _consts(D, Do_exp, Do_cst, df, logdet, logdetA, w, sign=1.0):
    hdf = 0.5 * (df + Do_exp)
    cst = gammaln(0.5 * (df + Do_cst)) - gammaln(0.5 * df) - 0.5 * Do_cst * np.log(df * np.pi) - 0.5 * (logdet + sign * logdetA) + np.log(w)
    return hdf, cst


def point_precision(x, miss, m, R, logdet, df, w):
    """One point against the K clusters, precision side, Float64: dict with want (K,), cm (K, r), and the parts the bounds need."""
    K, D = m.shape
    M = np.flatnonzero(miss)
    Do = D - len(M)
    z = np.where(miss, 0.0, np.where(miss, 0.0, x)[None, :] - m)
    y = np.einsum("kij,kj->ki", R, z)
    C = R[:, :, M]
    g = np.einsum("kir,ki->kr", C, y)
    A = np.einsum("kir,kis->krs", C, C)
    L = np.linalg.cholesky(A)
    logdetA = 2 * np.log(np.einsum("krr->kr", L)).sum(1)
    B = np.linalg.solve(A, C.transpose(0, 2, 1))                 # (K, r, D) = A^-1 C'
    t = np.einsum("kri,ki->kr", B, y)
    res = y - np.einsum("kir,kr->ki", C, t)
    q = (res * res).sum(1)
    hdf, cst = _consts(D, Do, Do, df, logdet, logdetA, w)
    tt = hdf * np.log1p(q / df)
    return dict(want=cst - tt, cm=m[:, M] - t, M=M, z=z, y=y, res=res, q=q, hdf=hdf, cst=cst, t=tt, B=B, tsol=t, g=g)


def point_covariance(x, miss, m, Sigma, df, w):
    """The same two results from the covariance side: scipy's multivariate t on the explicit sub-block, the textbook conditional mean."""
    K, D = m.shape
    M, O = np.flatnonzero(miss), np.flatnonzero(~miss)
    want, cm = np.empty(K), np.empty((K, len(M)))
    for k in range(K):
        Soo = Sigma[k][np.ix_(O, O)]
        want[k] = multivariate_t.logpdf(x[O], loc=m[k, O], shape=Soo, df=df[k]) + np.log(w[k])
        cm[k] = m[k, M] + Sigma[k][np.ix_(M, O)] @ np.linalg.solve(Soo, x[O] - m[k, O])
    return want, cm


def point_bounds(p, m, R, df, D):
    """(bound (K,) of the entries, dcm (K, r) of the conditional means) of one point from point_precision's parts."""
    az = np.einsum("kij,kj->ki", np.abs(R), np.abs(p["z"]))
    e = (D + 2) * U24 * az
    y2 = (p["y"] * p["y"]).sum(1)
    dq = 2 * (np.abs(p["res"]) * e).sum(1) + (e * e).sum(1) + 2.0 ** -36 * (p["q"] + y2)
    bound = p["hdf"] * dq / (df + p["q"]) + 2.0 ** -21 * (np.abs(p["cst"]) + p["t"]) + 1e-6
    aB = np.abs(p["B"])
    dcm = np.einsum("kri,ki->kr", aB, e) + 2.0 ** -36 * (np.abs(p["tsol"]) + np.einsum("kri,ki->kr", aB, np.abs(p["y"])))
    return bound, dcm


def reference(X, m, R, logdet, df, w, exact_logdet=False):
    """Everything the tests compare with, Float64 on the Float32 inputs the library receives.  want, bound (K, n): complete points from
    predictive_ref, marginalised ones from the precision side, over-the-cap ones NaN (bound 0).  cm, dcm: {i: (K, r)}.  exact_logdet: take
    `logdet` as the Float64 numbers they are (the two-sides comparison computes it from R)."""
    Xf = np.asarray(X, np.float32)
    ld = np.asarray(logdet, np.float64) if exact_logdet else np.asarray(logdet, np.float32).astype(np.float64)
    m64, R64, df64, w64 = (np.asarray(a, np.float32).astype(np.float64) for a in (m, R, df, w))
    K, D = m64.shape
    R64 = R64.reshape(K, D, D)
    miss, r, listed, over = classify(Xf)
    want, parts = pref.student_t_table(Xf, m, R, logdet, df, w)
    if exact_logdet:                       # (student_t_table rounds logdet to Float32: put the exact one back)
        want = want + 0.5 * (np.asarray(logdet, np.float32).astype(np.float64) - ld)[:, None]
        parts["cst"] = parts["cst"] + 0.5 * (np.asarray(logdet, np.float32).astype(np.float64) - ld)
    bound = pref.error_bound(Xf, m, R, df, parts)
    want[:, over] = np.nan
    bound[:, over] = 0.0
    cm, dcm = {}, {}
    X64 = Xf.astype(np.float64)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(listed):
            p = point_precision(X64[i], miss[i], m64, R64, ld, df64, w64)
            want[:, i] = p["want"]
            bound[:, i], dcm[int(i)] = point_bounds(p, m64, R64, df64, D)
            cm[int(i)] = p["cm"]
    check = listed & ~np.isinf(Xf).any(1)          # marginalised points with finite observed features: the ones compared with a bound
    return dict(want=want, bound=bound, cm=cm, dcm=dcm, miss=miss, r=r, listed=listed, over=over, check=check, q=parts["q"])


def derived(ref):
    """What the finish kernel makes of the table, in Float64, with tolerances derived from the per-entry bounds: logdens (n,) +- ld_tol,
    probs (n, K) +- p_tol, and for every imputed point i the values fill[i] (r,) +- fill_tol[i]."""
    want, bound = ref["want"], ref["bound"]
    K = want.shape[0]
    with np.errstate(all="ignore"):
        a = np.where(np.isnan(want), -np.inf, want)
        ld = logsumexp(a, axis=0)
        probs = np.exp(a - ld[None, :]).T
        bmax = bound.max(0)
        ld_tol = bmax + EPS * (K + 16) + EPS * np.abs(ld)
        rel = np.expm1(2 * bmax) + EPS * (K + 16)
        p_tol = probs * rel[:, None] + 1e-37
    fill, fill_tol = {}, {}
    for i, c in ref["cm"].items():
        p = probs[i][:, None]
        v = (p * c).sum(0)
        fill[i] = v
        fill_tol[i] = (p * ref["dcm"][i]).sum(0) + (p * rel[i] * np.abs(c - v[None, :])).sum(0) + EPS * np.abs(v) + 1e-37
    return dict(logdens=ld, ld_tol=ld_tol, probs=probs, p_tol=p_tol, fill=fill, fill_tol=fill_tol)


# ------------------------------------------------------------------------------------------------ the kernel in numpy
def emulate(X, m, R, logdet, df, w, mutation=None):
    """csrc/missing.hip restated: z and y in Float32, the small system in Float64, the entry rounded once -- or one of MUTATIONS.
    (table (K, n) Float32 with the listed points' columns filled and NaN elsewhere, cm {i: (K, r) Float64})."""
    f = np.float32
    Xf, m32, R32 = np.asarray(X, f), np.asarray(m, f), np.asarray(R, f)
    K, D = m32.shape
    R32 = R32.reshape(K, D, D)
    R64 = R32.astype(np.float64)
    ld, df64, w64 = (np.asarray(a, f).astype(np.float64) for a in (logdet, df, w))
    miss, r, listed, _ = classify(Xf)
    table = np.full((K, Xf.shape[0]), np.nan, f)
    cm = {}
    for i in np.flatnonzero(listed):
        M = np.flatnonzero(miss[i])
        Do = D - len(M)
        x0 = np.where(miss[i], f(0), Xf[i])
        z = x0[None, :] - m32                                        # Float32
        if mutation != "z_not_zeroed":
            z[:, M] = 0
        y32 = np.einsum("kij,kj->ki", R32, z)
        assert y32.dtype == f
        y = y32.astype(np.float64)
        C = R64[:, :, M]
        g = np.einsum("kir,ki->kr", C, y)
        A = np.einsum("kir,kis->krs", C, C)
        L = np.linalg.cholesky(A)
        logdetA = 2 * np.log(np.einsum("krr->kr", L)).sum(1)
        t = np.linalg.solve(A, g[:, :, None])[:, :, 0]
        if mutation == "f32_difference":
            q = ((y32 * y32).sum(1, dtype=f) - (g.astype(f) * t.astype(f)).sum(1, dtype=f)).astype(np.float64)
        else:
            res = y - np.einsum("kir,kr->ki", C, t)
            q = (res * res).sum(1)
        hdf, cst = _consts(D, D if mutation == "exp_D" else Do, D if mutation == "cst_D" else Do, df64, ld, logdetA, w64,
                           sign=0.0 if mutation == "no_logdetA" else -1.0 if mutation == "logdetA_sign" else 1.0)
        with np.errstate(all="ignore"):
            table[:, i] = (cst - hdf * np.log1p(q / df64)).astype(f)
        cm[int(i)] = m32[:, M].astype(np.float64) + (t if mutation == "plus_t" else -t)
    return table, cm


def worst_ratios(table, cm, ref):
    """(max |table - want| / bound over the entries of the marginalised points with finite features, max |cm - want| / (dcm + 2^-23 |want|) over their conditional means);
    a NaN where the reference is finite counts as infinitely far."""
    lst = np.flatnonzero(ref["check"])
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(table, np.float64)[:, lst] - ref["want"][:, lst]) / ref["bound"][:, lst]
        a = float(np.where(np.isnan(d), np.inf, d).max()) if d.size else 0.0
        b = 0.0
        for i in lst:
            e = np.abs(cm[int(i)] - ref["cm"][int(i)]) / (ref["dcm"][int(i)] + EPS * np.abs(ref["cm"][int(i)]) + 1e-37)
            b = max(b, float(np.where(np.isnan(e), np.inf, e).max()))
    return a, b


# ------------------------------------------------------------------------------------------------ inputs
def make_case(D, K, dense=False):
    """predictive_ref.make_case(D, K) (n = 2 tiles + 5; conditioning as there, which keeps the bound inside test_loglik_table's tolerance
    on the bulk) with gaps planted, c["gaps"] = {position: features}:
      position 0: feature 0; position n - 1: feature D - 1; the last point of tile 0 and the first of tile 1: two adjacent features / the
      two ends (D = 2: one feature each); 50: r = min(16, D - 1); 51: r = 17 where D >= 18 (over the cap); 52: every feature (over the cap);
      53: NaN at feature 0 and +Inf at feature D - 1; 60: the mean of cluster k0 = min(1, K - 1) with feature 1 % D missing;
      predictive_ref's own two NaN points (feature D - 1 at 200, feature 0 at tile + 50); half of the bulk points tile + 60 .. tile + 119
      with 1 .. min(4, cap) random gaps.  No point of 80 .. 119 has a gap: with a capacity of 40 one slab holds none.
    dense: half of ALL remaining bulk points get 1 .. cap random gaps as well (the CPU tests' statistics).
    c["lab"] stays the cluster each bulk point was drawn from."""
    c = pref.make_case(D, K)
    X, n, t = c["X"], c["n"], pref.tile_of(D)
    cap = cap_of(D)
    rng = np.random.default_rng(7919 * D + K)
    gaps = {}

    def put(i, feats):
        feats = sorted(int(j) for j in feats)
        X[i, feats] = np.nan
        gaps[int(i)] = feats

    put(0, [0])
    put(n - 1, [D - 1])
    put(t - 1, [D // 2, D // 2 + 1] if D >= 4 else [1])
    put(t, [0, D - 1] if D >= 3 else [0])
    put(50, rng.choice(D, cap, replace=False))
    if D >= 18:
        put(51, rng.choice(D, 17, replace=False))
    put(52, range(D))
    put(53, [0])
    X[53, D - 1] = np.inf
    k0 = min(1, K - 1)
    X[60] = c["m"][k0]
    put(60, [1 % D])
    for i, j in c["planted"]["nan"]:
        gaps[int(i)] = [int(j)]
    used = set(gaps)
    for i in range(t + 60, t + 120):
        if c["bulk"][i] and i not in used and rng.random() < 0.5:
            put(i, rng.choice(D, int(rng.integers(1, min(4, cap) + 1)), replace=False))
    if dense:
        for i in range(n):
            if c["bulk"][i] and i not in gaps and not 50 <= i <= 60 and rng.random() < 0.5:
                put(i, rng.choice(D, int(rng.integers(1, cap + 1)), replace=False))
    bulk = c["bulk"].copy()
    bulk[[0, n - 1, t - 1, t, 50, 51, 52, 53, 60]] = False
    c.update(gaps=gaps, bulk=bulk, k0=k0, naninf=53, mean_gap=60, free_slab=(80, 120))
    return c


def make_correlated_case(D=4, K=3, rho=0.9999, n=96):
    """Strongly correlated features (equicorrelation rho, cond(Sigma) about D / (1 - rho)): what the observed features say about the missing
    ones is nearly everything, |y|^2 = z_O' Lambda_OO z_O is thousands of times q_o = z_O' Sigma_OO^-1 z_O, and a kernel that forms q_o as
    the difference |y|^2 - g't in Float32 loses it in the rounding of |y|^2 -- the case the explicit residual and the Float64 small system
    are there for.  Every point has 1 .. D - 1 gaps.  Same keys as make_case."""
    rng = np.random.default_rng(31 * D + K)
    scale = np.linspace(0.7, 1.5, K)
    Sigma = scale[:, None, None] ** 2 * ((1 - rho) * np.eye(D) + rho * np.ones((D, D)))[None]
    R = np.linalg.cholesky(np.linalg.inv(Sigma)).transpose(0, 2, 1).astype(np.float32)          # upper, R'R = Sigma^-1
    logdet = (-2 * np.log(np.abs(np.einsum("kii->ki", R.astype(np.float64)))).sum(1)).astype(np.float32)
    m = (0.5 * rng.standard_normal((K, D))).astype(np.float32)
    df = np.array([pref.DFS[k % 3] for k in range(K)], np.float32)
    w = rng.dirichlet(np.full(K, 5.0)).astype(np.float32)
    lab = rng.integers(0, K, n)
    X = (m[lab] + np.linalg.solve(R[lab].astype(np.float64), rng.standard_normal((n, D, 1)))[:, :, 0]).astype(np.float32)
    gaps = {}
    for i in range(n):
        gaps[i] = sorted(int(j) for j in rng.choice(D, int(rng.integers(1, D)), replace=False))
        X[i, gaps[i]] = np.nan
    return dict(D=D, K=K, n=n, X=X, m=m, R=R, logdet=logdet, df=df, w=w, lab=lab, bulk=np.ones(n, bool), gaps=gaps)
