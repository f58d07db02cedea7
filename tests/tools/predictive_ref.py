"""Float64 reference of the Student-t predictive table (the Student-t mode of csrc/niw_sweep.hip behind dpmm_set_predictive_niw), a derived
bound on what a correct Float32 kernel may differ from it by, the inputs of tests/test_gpu_predictive.py, and a numpy Float32 restatement
of the kernel with the mistakes the bound has to catch (tests/test_predictive_reference_cpu.py).  Pure numpy / scipy: nothing here imports
the package or needs a GPU.

The table:   want[k, i] = cst_k - hdf_k log1p(q_ki / df_k),     q_ki = |R_k (x_i - m_k)|^2,     hdf_k = (df_k + D) / 2,
             cst_k = lgamma(hdf_k) - lgamma(df_k / 2) - D/2 log(df_k pi) - logdet_k / 2 + log w_k
evaluated in Float64 on the Float32-rounded parameters and points.

The bound (every quantity from the Float64 evaluation, none from the kernel), u = 2^-24:
  z = x - m is one Float32 subtraction; y = R z is a sum of at most D products accumulated in Float32 in any order, so
      |y_i - fl(y_i)| <= e_i = (D + 2) u sum_j |R_ij| |z_j|            (1 for the subtraction, 1 per product, at most D - 1 additions; rounded up)
  q = sum_i y_i^2:   |q - fl(q)| <= dq = 2 sum_i |y_i| e_i + sum_i e_i^2 + (D + 1) u q            (the squares and their D - 1 additions)
  a = cst - hdf log1p(q / df):   |da/dq| = hdf / (df + q), and the Float32 roundings of cst, of the division, of a few-ulp log1pf, of the
      product and of the subtraction are each relative to |cst| or to hdf log1p(q / df):
  bound = hdf dq / (df + q) + 2^-21 (|cst| + hdf log1p(q / df)) + 1e-6.
"""
import numpy as np
from scipy.special import gammaln

U24 = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
DFS = (1.0, 5.3, 1e6)                    # heavy tail, ordinary, the Gaussian limit
LOGLIK_ATOL, LOGLIK_RTOL = 1e-3, 2e-5    # the tolerance of tests/test_gpu_niw.py::test_loglik_table: what the bound is measured against

# D at K = 3: every instantiation (NB = 1, 2, 4, 8, 16), its padded edge and the first D of the next one
DIMS = (1, 2, 5, 16, 17, 32, 33, 48, 63, 64, 65, 100, 128, 129, 200, 256)
# (D, K): one cluster (the `lone` shortcut must not apply in Student-t mode), more rows than launch_direct's LDS row budget of the NB
# (39, 52 and 79 rows), many clusters on the wide path
K_CASES = ((2, 1), (64, 1), (8, 45), (24, 60), (64, 90), (128, 70))
CASES = tuple((D, 3) for D in DIMS) + K_CASES
POSTERIOR_DIMS = (2, 20, 64, 70, 256)


def tile_of(D):
    return 256 if D <= 64 else 128


def _f64(*a):
    return [np.asarray(v, np.float32).astype(np.float64) for v in a]


def _quad(X, m, R):
    """z (K, n, D), y = R z (K, n, D) and q = |y|^2 (K, n) in Float64."""
    z = X[None, :, :] - m[:, None, :]
    y = np.einsum("kij,knj->kni", R, z)
    return z, y, (y * y).sum(-1)


def student_t_table(X, m, R, logdet, df, w):
    """(want (K, n) Float64, parts): the table of the inputs dpmm_set_predictive_niw receives.  X (n, D), m (K, D), R (K, D, D) or (K, D D)
    upper triangular with Sigma^-1 = R'R, logdet = log det Sigma, df, w (K,).  parts: q (K, n), cst, hdf, df (K,), the Float64 y."""
    X, m, R, logdet, df, w = _f64(X, m, R, logdet, df, w)
    K, D = m.shape
    R = R.reshape(K, D, D)
    with np.errstate(all="ignore"):
        _, y, q = _quad(X, m, R)
        hdf = 0.5 * (df + D)
        cst = gammaln(hdf) - gammaln(0.5 * df) - 0.5 * D * np.log(df * np.pi) - 0.5 * logdet + np.log(w)
        t = hdf[:, None] * np.log1p(q / df[:, None])
    return cst[:, None] - t, dict(q=q, cst=cst, hdf=hdf, df=df, t=t, y=y)


def gaussian_table(parts, logdet, w, D):
    """-D/2 log(2 pi) - logdet/2 - q/2 + log w: what the Student-t table tends to as df grows (within (q^2 + D^2) / df)."""
    logdet, w = _f64(logdet, w)
    return (-0.5 * D * np.log(2 * np.pi) - 0.5 * logdet + np.log(w))[:, None] - 0.5 * parts["q"]


def error_bound(X, m, R, df, want_parts, rounded_R=False):
    """(K, n) bound of the module docstring.  rounded_R: the R the kernel received is the Float32 rounding of the R of the reference
    (a host conversion computed it in Float64), which moves y_i by at most u sum_j |R_ij| |z_j| more."""
    X, m, R, df = _f64(X, m, R, df)
    K, D = m.shape
    R = R.reshape(K, D, D)
    p = want_parts
    with np.errstate(all="ignore"):
        z = X[None, :, :] - m[:, None, :]
        az = np.einsum("kij,knj->kni", np.abs(R), np.abs(z))
        e = (D + 2 + (1 if rounded_R else 0)) * U24 * az
        dq = 2 * (np.abs(p["y"]) * e).sum(-1) + (e * e).sum(-1) + (D + 1) * U24 * p["q"]
        return p["hdf"][:, None] * dq / (df[:, None] + p["q"]) + 2.0 ** -21 * (np.abs(p["cst"])[:, None] + p["t"]) + 1e-6


def bulk_share(bound, want, bulk, lab=None):
    """Share of the bulk points whose bound is within test_loglik_table's tolerance, so that the bound is not vacuous: under the cluster
    the point was drawn from (lab (n,): the entry that carries the point's density), or, without lab, of all (cluster, bulk point) entries."""
    ok = bound <= LOGLIK_ATOL + LOGLIK_RTOL * np.abs(want)
    if lab is not None:
        ok = ok[lab, np.arange(ok.shape[1])][None, :]
    return float(ok[:, bulk].mean())


def check_table(got, want, bound, q):
    """Asserts that `got` is a correct Float32 table and returns max |got - want| / bound over the finite entries.  NaN exactly where the
    reference is NaN (a NaN feature); -Inf exactly where q exceeds the Float32 range (the kernel's q overflows while the Float64 one is
    finite: the documented divergence); every other entry finite and within the bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN entries differ from the reference's"
    over = ~nan & (q > FLT_MAX)
    assert np.all(np.isneginf(got[over])), "an entry whose q is beyond FLT_MAX is not -Inf"
    fin = ~nan & ~over
    assert np.all(np.isfinite(got[fin])), "a non-finite entry where the reference is finite and q is in range"
    ratio = np.abs(got[fin] - want[fin]) / bound[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"max |got - want| / bound = {worst:.3g}"
    return worst


# ------------------------------------------------------------------------------------------------ inputs
def conditioning(D):
    """(size of R's off-diagonal part, largest scale).  Up to D = 64 as plain as can be: 0.05 and scales 0.5 .. 2.  Beyond, the bound's
    first term grows like D^2 u times sum |R_ij| |z_j| / |y_i| against a tolerance of 2e-5 |want|, and with these values it is no longer
    within test_loglik_table's tolerance for 95 % of the bulk (at D = 256: for none of it); bulk_share says which inputs are: a smaller
    off-diagonal part (less cancellation in y) and, above D = 128, scales below 1 (logdet and the log1p term then have the same sign, so
    |want| is not a difference of two large numbers)."""
    return (0.05, 2.0) if D <= 64 else (0.025, 2.0) if D <= 128 else (0.0125, 0.6)


def make_case(D, K):
    """Inputs of one (D, K) case: n = 2 tiles + 5 points, upper-triangular R = scale_k (eye + 0.05 triu(normal)) with scale_k in 0.5 .. 2
    (D > 64: see conditioning), distinct df (1.0, 5.3, 1e6 in turn), unequal weights, bulk points drawn from the clusters' Gaussians (q
    about D under their own cluster) and planted ones: two cluster means, two points 1e3 sd out, a point of +-1e25 features, two points
    with a NaN feature."""
    offd, smax = conditioning(D)
    rng = np.random.default_rng(100003 * D + K)
    n = 2 * tile_of(D) + 5
    m = (0.5 * rng.standard_normal((K, D))).astype(np.float32)
    scale = rng.permutation(np.linspace(0.5, smax, K)) if K > 1 else np.array([1.3])
    R = ((np.eye(D) + offd * np.triu(rng.standard_normal((K, D, D)))) * scale[:, None, None]).astype(np.float32)
    logdet = (-2 * np.log(np.abs(np.einsum("kii->ki", R.astype(np.float64)))).sum(1)).astype(np.float32)
    df = (np.array([DFS[k % 3] for k in range(K)]) if K > 1 else np.array([5.3])).astype(np.float32)
    w = (rng.dirichlet(np.full(K, 5.0)) if K > 1 else np.array([0.7])).astype(np.float32)      # K = 1: not 1, so that log w shows
    lab = rng.integers(0, K, n)
    X = m[lab] + np.linalg.solve(R[lab].astype(np.float64), rng.standard_normal((n, D, 1)))[:, :, 0]
    t = tile_of(D)
    planted = dict(mean=[(1, 0), (n - 2, K - 1)], far=[(7, 0), (t + 3, K - 1)], huge=[100], nan=[(200, D - 1), (t + 50, 0)])
    X = X.astype(np.float32)
    for i, k in planted["mean"]:
        X[i] = m[k]
    for i, k in planted["far"]:
        u = rng.standard_normal(D)
        X[i] = (m[k] + 1e3 * np.linalg.solve(R[k].astype(np.float64), u * np.sqrt(D) / np.linalg.norm(u))).astype(np.float32)      # q = 1e6 D
    for i in planted["huge"]:
        X[i] = np.where(rng.random(D) < 0.5, -1e25, 1e25).astype(np.float32)
    for i, j in planted["nan"]:
        X[i, j] = np.nan
    bulk = np.ones(n, bool)
    bulk[[i for v in planted.values() for i in (e if isinstance(e, int) else e[0] for e in v)]] = False
    return dict(D=D, K=K, n=n, X=X, m=m, R=R, logdet=logdet, df=df, w=w, planted=planted, bulk=bulk, lab=lab)


def make_posterior(D, K=3):
    """A hand-made NIW posterior (kappa, nu, m, upper-triangular U with nu psi = U U'), weights and points.  One nu barely above D - 1
    (df = 1 + 2^-10) and one kappa of 0.01.  m and nu - D + 1 are Float32 values, so that the conversion's only rounding of consequence is
    that of R (error_bound's rounded_R term) -- logdet's is relative to |cst| like the other roundings of the constant."""
    rng = np.random.default_rng(7 * D + 1)
    n = 2 * tile_of(D) + 5
    kappa = np.array([0.01, 3.0, 250.0])[:K]
    df = np.array([1.0 + 2.0 ** -10, 5.25, 300.0])[:K]
    nu = df + D - 1
    m = (0.5 * rng.standard_normal((K, D))).astype(np.float32).astype(np.float64)
    s = np.array([0.7, 1.0, 1.6])[:K] * np.sqrt(nu)                 # psi of about s^2 I
    U = (np.eye(D) + conditioning(D)[0] * np.triu(rng.standard_normal((K, D, D)))) * s[:, None, None]
    w = rng.dirichlet(np.full(K, 5.0)).astype(np.float32)
    c = (kappa + 1) / (kappa * df)
    lab = rng.integers(0, K, n)
    X = (m[lab] + np.sqrt(c[lab])[:, None] * np.einsum("nij,nj->ni", U[lab], rng.standard_normal((n, D)))).astype(np.float32)
    post = dict(kappa=kappa, nu=nu, m=m, U=U)
    return dict(D=D, K=K, n=n, X=X, post=post, w=w, c=c, bulk=np.ones(n, bool), lab=lab)


def posterior_reference(P, conv, logpdf):
    """(want, parts, bound) of a make_posterior problem.  want: logpdf(X, kappa, m, nu, psi) of the posterior itself (the oracle's
    niw_posterior_predictive: scipy's multivariate t) + log w.  The bound is evaluated on conv = (m, R, logdet, df, w), the converted
    Float32 parameters the worker receives, with the rounding of R."""
    post = P["post"]
    want = np.stack([logpdf(P["X"], post["kappa"][k], post["m"][k], post["nu"][k], post["U"][k] @ post["U"][k].T / post["nu"][k])
                     for k in range(P["K"])]) + np.log(P["w"].astype(np.float64))[:, None]
    m, R, logdet, df, w = conv
    _, parts = student_t_table(P["X"], m, R, logdet, df, w)
    return want, parts, error_bound(P["X"], m, R, df, parts, rounded_R=True)


class Capture:
    """Stands in for a worker: keeps what niw_hyperparams.predictive_table hands it."""

    def predict_table_niw(self, m, R, logdet, df, weights, points=False):
        self.args = tuple(np.asarray(a, np.float32) for a in (m, R, logdet, df, weights))


# ------------------------------------------------------------------------------------------------ the kernel in numpy Float32
MUTATIONS = ("hdf_padded", "df_hdf_swapped", "no_log_w", "whole_logdet", "log_for_log1p")


def emulate_f32(X, m, R, logdet, df, w, mutation=None):
    """The kernel's formula with Float32 accumulation (dpmm_set_predictive_niw's constants in Float64, rounded once), or one of MUTATIONS."""
    f = np.float32
    X, m, R, logdet, df, w = (np.asarray(a, f) for a in (X, m, R, logdet, df, w))
    K, D = m.shape
    R = R.reshape(K, D, D)
    v = df.astype(np.float64)
    Dh = 16 * -(-D // 16) if mutation == "hdf_padded" else D
    cst = (gammaln(0.5 * (v + D)) - gammaln(0.5 * v) - 0.5 * D * np.log(v * np.pi)
           - (1.0 if mutation == "whole_logdet" else 0.5) * logdet.astype(np.float64)
           + (0.0 if mutation == "no_log_w" else np.log(w.astype(np.float64)))).astype(f)
    hdf = (0.5 * (v + Dh)).astype(f)
    with np.errstate(all="ignore"):
        z = X[None, :, :] - m[:, None, :]
        y = np.einsum("kij,knj->kni", R, z)
        q = (y * y).sum(-1, dtype=f)
        a, b = (df, hdf) if mutation == "df_hdf_swapped" else (hdf, df)
        r = q / b[:, None]
        lg = np.log(r) if mutation == "log_for_log1p" else np.log1p(r)
        out = cst[:, None] - a[:, None] * lg
    assert out.dtype == f
    return out
