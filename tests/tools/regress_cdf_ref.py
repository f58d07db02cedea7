"""Float64 reference of the conditional CDF and quantiles of the targets (include/dpmm_hip_regress_cdf.h, csrc/regress_cdf.hip) with the
header's bound b_F, the mistakes the bound has to catch, and the inputs tests/test_regress_cdf_cpu.py and tests/test_gpu_regress_cdf.py
share.  numpy and scipy.stats.t -- an evaluation of the Student-t that shares nothing with the library's continued fraction.

    nu_k = df_k + D_o        mu_ikd = c_kd + sum_e B_kde x_ie        sigma_ikd^2 = (df_k + q_ik) / (df_k + D_o) V_kd
    F_id(y) = sum_k p_ik T_nu_k((y - mu_ikd) / sigma_ikd)            f_id(y) = sum_k p_ik g_nu_k(t) / sigma_ikd
    b_F = sum_k p_ik [g_nu_k(max(0, |t| - dt)) dt + 2^-20 h] + ((K + 4) 2^-52 + u) exact + 2^-150,   h = min(T, 1 - T),
    dt = d_ik / sigma + |t| (e / 2) / (1 - e),   d_ik = (D_o + 3) u a_ikd,   e = expm1(2 t_ik / (df_k + D_o)) + 3 u,   u = 2^-24
"""
import numpy as np
from scipy import stats

from tools import regress_ref as rr

U24 = 2.0 ** -24
MUTATIONS = ("variance_with_nu_factor", "df_without_Do", "a_p_dropped")
LEVELS = (1e-4, 0.05, 0.5, 0.95, 1 - 1e-4)
SHAPES = ((1, 1), (5, 31), (32, 33), (33, 130), (7, 249))      # (7 + 249 = 256 = DPMM_MAX_DIM_NIW: the widest joint model there is)
KS = (1, 3, 40)
NS = (1, 31, 33, 229)


def components(B, c, V, df, q, x, Do, mutation=None):
    """mu, sigma (n, K, D_t) and nu (K,) in Float64."""
    B, c, V, df, q, x = (np.asarray(a, np.float64) for a in (B, c, V, df, q, x))
    mu = c[None] + np.einsum("kde,ne->nkd", B, x)
    nu = df + Do
    s = (df[None] + q) / (df[None] + Do)
    if mutation == "variance_with_nu_factor":
        s = (df[None] + q) / (df[None] + Do - 2.0)
    if mutation == "df_without_Do":
        nu = df.copy()
    return mu, np.sqrt(s[:, :, None] * V[None]), nu


def cdf(p, B, c, V, df, q, x, y, t=None, mutation=None):
    """dict(cdf, sf, pdf, b_cdf, b_sf), each (n, D_t): the mixture at y (n, D_t) from p (n, K); t (n, K) bounds the table entries' errors.
    The mutation is applied to the values, never to the bound."""
    p = np.asarray(p, np.float64)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n, K = p.shape
    Do = x.shape[1]
    out = {}
    with np.errstate(all="ignore"):
        for name, mut in (("got", mutation), ("clean", None)):
            mu, sig, nu = components(B, c, V, df, q, x, Do, mut)
            tt = (y[:, None, :] - mu) / sig
            pk = p[:, :, None].copy()
            if mut == "a_p_dropped":
                pk[np.arange(n), np.argmax(p, 1)] = 0.0
            live = pk != 0
            nn = nu[None, :, None]
            out[name] = dict(cdf=np.where(live, pk * stats.t.cdf(tt, nn), 0.0).sum(1), sf=np.where(live, pk * stats.t.sf(tt, nn), 0.0).sum(1),
                             pdf=np.where(live, pk * stats.t.pdf(tt, nn) / sig, 0.0).sum(1), t=tt, live=live, pk=pk, sig=sig, nn=nn)
        cl = out["clean"]
        a = np.abs(np.asarray(c, np.float64))[None] + np.einsum("kde,ne->nkd", np.abs(np.asarray(B, np.float64)), np.abs(x))
        d = (Do + 3) * U24 * a
        te = np.zeros((n, K)) if t is None else np.asarray(t, np.float64)
        e = (np.expm1(2.0 * te / (np.asarray(df, np.float64)[None] + Do)) + 3 * U24)[:, :, None]
        at = np.abs(cl["t"])
        dt = d / cl["sig"] + at * (0.5 * e) / (1.0 - e)
        h = np.minimum(stats.t.cdf(cl["t"], cl["nn"]), stats.t.sf(cl["t"], cl["nn"]))
        per = stats.t.pdf(np.maximum(0.0, at - dt), cl["nn"]) * dt + 2.0 ** -20 * h
        core = np.where(cl["live"], cl["pk"] * per, 0.0).sum(1)
        rel = (K + 4) * 2.0 ** -52 + U24
    g = out["got"]
    under = 2.0 ** -150                                  # the final rounding where Float32 is subnormal: half its smallest step
    return dict(cdf=g["cdf"], sf=g["sf"], pdf=cl["pdf"], b_cdf=core + rel * cl["cdf"] + under, b_sf=core + rel * cl["sf"] + under)


def quantile(p, B, c, V, df, q, x, levels):
    """(L, n, D_t) Float64: the root of F_id = level by bisection from the bracket of the components' own quantiles."""
    p = np.asarray(p, np.float64)
    x = np.asarray(x, np.float64)
    Do = x.shape[1]
    mu, sig, nu = components(B, c, V, df, q, x, Do)
    live = (p != 0)[:, :, None]
    out = []
    for lv in levels:
        yk = mu + sig * stats.t.ppf(lv, nu)[None, :, None]
        lo, hi = np.where(live, yk, np.inf).min(1), np.where(live, yk, -np.inf).max(1)
        for _ in range(120):
            mid = 0.5 * (lo + hi)
            F = np.where(live, p[:, :, None] * stats.t.cdf((mid[:, None, :] - mu) / sig, nu[None, :, None]), 0.0).sum(1)
            lo, hi = np.where(F < lv, mid, lo), np.where(F < lv, hi, mid)
        out.append(0.5 * (lo + hi))
    return np.stack(out)


def ulp32(y):
    """The step up from |y| to the next Float32 value."""
    y = np.abs(np.asarray(y, np.float32))
    return (np.nextafter(y, np.float32(np.inf)) - y).astype(np.float64)


def quantile_contract(p, B, c, V, df, q, x, yq, level, t=None):
    """(|F_exact(y) - level|, its bound) for the returned Float32 yq (n, D_t), the header's: with y- the Float32 predecessor of y,
    max(b_F at y, b_F at y-) + max(f at y, f at y-) (y - y-)."""
    yq = np.asarray(yq, np.float32)
    prev = np.nextafter(yq, np.float32(-np.inf))
    here = cdf(p, B, c, V, df, q, x, yq.astype(np.float64), t=t)
    below = cdf(p, B, c, V, df, q, x, prev.astype(np.float64), t=t)
    bound = np.maximum(here["b_cdf"], below["b_cdf"]) + np.maximum(here["pdf"], below["pdf"]) * (yq.astype(np.float64) - prev.astype(np.float64))
    return np.abs(here["cdf"] - level), bound


# ------------------------------------------------------------------------------------------------ inputs
def make_case(Do, Dt, K, n, overlap=True, low_df=False, seed=0):
    """A posterior over D_o + D_t features (regress_ref.make_posterior) and n points of the given features drawn from its clusters.
    overlap: the cluster means are pulled to about two standard deviations apart, so that several p_ik != 0 for most points; else they stay
    40 apart (one cluster per point, but for the heavy tails at small D_o).  low_df: cluster 0 has df + D_o <= 2 (Do = 1)."""
    D = Do + Dt
    post, s = rr.make_posterior(D, K, 1009 * Do + 31 * Dt + K + seed)
    if overlap:
        post["m"] = (post["m"] / 20.0).astype(np.float32).astype(np.float64)
    if low_df:
        assert Do == 1
        post["nu"][0] = 0.75 + D - 1                   # df = 0.75: no variance, and no mean either
    rng = np.random.default_rng(7 * Do + Dt + 100 * K + n)
    perm = rng.permutation(D)
    given, targets = [int(f) for f in perm[:Do]], [int(f) for f in perm[Do:]]
    lab = rng.integers(0, K, n)
    full = post["m"][lab] + s[lab][:, None] * rng.standard_normal((n, D))
    return dict(Do=Do, Dt=Dt, D=D, K=K, n=n, post=post, given=given, targets=targets, X=full[:, given].astype(np.float32),
                Y=full[:, targets].astype(np.float32), lab=lab, s=s)


# the law test: D = 6, K = 4, overlapping; the reference's PITs of the sample `Predictor.sample(n, seed)` draws pass with room
# (tests/test_regress_cdf_cpu.py checks, on tools/sample_ref's restatement of that sample)
LAW = dict(D=6, K=4, n=20000, given=[0, 2, 5], targets=[1, 3, 4], seed=2, limit=1.63 / np.sqrt(20000.0))


def law_posterior():
    """The law test's model: regress_ref.make_posterior pulled together, the last cluster next to the first."""
    post, _ = rr.make_posterior(LAW["D"], LAW["K"], 77)
    post["m"] = (post["m"] / 20.0).astype(np.float32).astype(np.float64)
    post["m"][LAW["K"] - 1] = post["m"][0] + 1.5
    return post


def kolmogorov(u):
    u = np.sort(np.asarray(u, np.float64).ravel())
    n = len(u)
    return max((np.arange(1, n + 1) / n - u).max(), (u - np.arange(n) / n).max())
