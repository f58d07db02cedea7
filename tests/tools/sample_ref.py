"""A numpy restatement of the sampler (include/dpmm_hip_sample.h) with the same keying, and the statistical checks that the CPU and GPU
tests of Predictor.sample share.

  * philox            Philox4x32-10, key = seed, counter = (i low, i high, block, stream), vectorised over i / block.
  * mult_counts       the alias draw: integers only, so the counts equal the GPU's bit for bit.
  * niw_points        the NIW construction in Float64 from the same random words (53- / 32-bit uniforms, accurate log / cos / sin): the
                      law is exact; the values are those of the GPU up to its Float32 arithmetic.
  * check_whitened    the law checks on whitened points y = A^-1 (x - m), each with its derivation; they raise AssertionError.
"""
import io

import numpy as np
from scipy import stats

STREAM_NORMAL, STREAM_CHI, STREAM_MULT = 40, 41, 42
M32 = np.uint64(0xFFFFFFFF)
SPARSE_CAP = 4096


def philox(seed, idx, block, stream):
    """(4, ...) uint64 array holding the four 32-bit words of every block; idx / block broadcast against each other."""
    idx, block = np.broadcast_arrays(np.asarray(idx, np.uint64), np.asarray(block, np.uint64))
    c0, c1, c2 = idx & M32, idx >> np.uint64(32), block & M32
    c3 = np.full(idx.shape, stream, np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3])


def cluster_sizes(weights64, n, seed):
    return np.random.Generator(np.random.Philox(int(seed))).multinomial(int(n), weights64).astype(np.int64)


def labels_of(n_k):
    """0-based cluster of every sample, grouped."""
    return np.repeat(np.arange(len(n_k)), n_k)


# ------------------------------------------------------------------------------------------------ Multinomial
def mult_counts(thr, alias, lab, idx, seed, trials):
    """(n, D) int64 counts of the samples with global indices `idx` and 0-based clusters `lab`."""
    thr, alias = np.asarray(thr, np.uint64), np.asarray(alias, np.int64)
    K, D = thr.shape
    n = len(idx)
    out = np.zeros((n, D), np.int64)
    if n == 0:
        return out
    nblk = (trials + 1) // 2
    rows = np.arange(n)
    for b0 in range(0, nblk, 512):
        b = np.arange(b0, min(nblk, b0 + 512), dtype=np.uint64)
        w = philox(seed, np.asarray(idx, np.uint64)[:, None], b[None, :], STREAM_MULT)          # (4, n, nb)
        for half in (0, 1):
            r0, r1 = w[2 * half], w[2 * half + 1]
            live = (2 * b.astype(np.int64) + half < trials)[None, :] & np.ones((n, 1), bool)
            j = ((r0 * np.uint64(D)) >> np.uint64(32)).astype(np.int64)
            cat = np.where(r1 < thr[lab[:, None], j], j, alias[lab[:, None], j])
            np.add.at(out, (np.broadcast_to(rows[:, None], cat.shape)[live], cat[live]), 1)
    return out


def alias_probabilities(thr, alias):
    """Category probabilities that (thr, alias) realise with a uniform bucket: Float64, rows of K."""
    thr = np.asarray(thr, np.float64)
    K, D = thr.shape
    p = thr / 2.0 ** 32
    out = np.zeros((K, D))
    for k in range(K):
        full = np.asarray(alias[k]) == np.arange(D)              # its own alias: the threshold decides nothing
        acc = np.where(full, 1.0, p[k])
        out[k] = acc
        np.add.at(out[k], np.asarray(alias[k], np.int64), 1.0 - acc)
    return out / D


# ------------------------------------------------------------------------------------------------ NIW
def _u53(a, b):
    return ((((a << np.uint64(32)) | b) >> np.uint64(11)).astype(np.float64) + 0.5) / 9007199254740992.0


def normals(idx, D, seed):
    """(n, D) Float64: block b -> coordinates 4b .. 4b + 3 (cos, sin of two Box-Muller pairs, 32-bit uniforms (v + 0.5) 2^-32)."""
    nb4 = (D + 3) // 4
    w = philox(seed, np.asarray(idx, np.uint64)[:, None], np.arange(nb4, dtype=np.uint64)[None, :], STREAM_NORMAL).astype(np.float64)
    u = (w + 0.5) / 4294967296.0
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    t0, t1 = 2 * np.pi * u[1], 2 * np.pi * u[3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=2)      # (n, nb4, 4)
    return z.reshape(len(idx), 4 * nb4)[:, :D]


def chi2(df, idx, seed, rounds=8):
    """(n,) Float64: 2 Gamma(df / 2) by Marsaglia-Tsang with the kernel's blocks and its bound of `rounds` rounds."""
    idx = np.asarray(idx, np.uint64)
    a = 0.5 * np.asarray(df, np.float64) * np.ones(len(idx))
    boost = np.ones(len(idx))
    low = a < 1.0
    if low.any():
        ru = philox(seed, idx, 63, STREAM_CHI)
        boost = np.where(low, _u53(ru[0], ru[1]) ** (1.0 / a), 1.0)
        a = np.where(low, a + 1.0, a)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    last, done = d.copy(), np.zeros(len(idx), bool)
    for t in range(rounds):
        rn, ru = philox(seed, idx, 2 * t, STREAM_CHI), philox(seed, idx, 2 * t + 1, STREAM_CHI)
        x = np.sqrt(-2.0 * np.log(_u53(rn[0], rn[1]))) * np.cos(2 * np.pi * _u53(rn[2], rn[3]))
        u = _u53(ru[0], ru[1])
        v = 1.0 + c * x
        pos = (v > 0.0) & ~done
        v = np.where(v > 0.0, v, 1.0) ** 3
        last = np.where(pos, d * v, last)
        acc = (u < 1.0 - 0.0331 * x ** 4) | (np.log(u) < 0.5 * x * x + d * (1.0 - v + np.log(v)))
        done |= pos & acc
    return 2.0 * last * boost


def niw_points(m, A, df, lab, idx, seed, mutate=None):
    """(n, D) Float64 samples x = m_k + sqrt(df_k / g) A_k z.  mutate: None, or one of the deliberately WRONG variants the tests must
    reject: "transpose" (A' for A), "last_column" (the last column of A zeroed: the last normal is missed), "reuse" (z_1 = z_0)."""
    m, A, df = np.asarray(m, np.float64), np.asarray(A, np.float64), np.asarray(df, np.float64)
    D = m.shape[1]
    z = normals(idx, D, seed)
    if mutate == "transpose":
        A = A.transpose(0, 2, 1)
    elif mutate == "last_column":
        A = A.copy()
        A[:, :, -1] = 0.0
    elif mutate == "reuse":
        z[:, 1] = z[:, 0]
    elif mutate is not None:
        raise ValueError(mutate)
    g = chi2(df[lab], idx, seed)
    out = np.empty_like(z)
    for k in np.unique(lab):
        s = lab == k
        out[s] = m[k] + np.sqrt(df[k] / g[s])[:, None] * (z[s] @ A[k].T)
    return out


def whiten(x, m, A):
    """y = A^-1 (x - m) of the points (n, D) of one cluster, in Float64 (A upper triangular)."""
    from scipy.linalg import solve_triangular
    return solve_triangular(np.asarray(A, np.float64), (np.asarray(x, np.float64) - np.asarray(m, np.float64)).T, lower=False).T


# ------------------------------------------------------------------------------------------------ the law checks
KS_LAMBDA = 3.3


def ks_distance(sample, cdf):
    """sup |F_n - F| of a sample against a continuous distribution function."""
    s = np.sort(np.asarray(sample, np.float64))
    n = len(s)
    f = cdf(s)
    return max(np.max(np.arange(1, n + 1) / n - f), np.max(f - np.arange(n) / n))


def tested_coordinates(D):
    """All coordinates for D <= 17; else 16 of them: the first, the last, both sides of multiples of 16 (where a kernel's blocks meet),
    thinned evenly when those are more than 16 and filled up evenly when fewer."""
    if D <= 17:
        return list(range(D))
    must = sorted({0, D - 1} | {c for j in range(16, D, 16) for c in (j - 1, j)})
    if len(must) > 16:
        must = sorted({must[i] for i in np.round(np.linspace(0, len(must) - 1, 16)).astype(int)})
    rest = [c for c in range(D) if c not in must]
    need = 16 - len(must)
    fill = [rest[i] for i in np.round(np.linspace(0, len(rest) - 1, need)).astype(int)] if need else []
    return sorted(must + fill)


def check_whitened(y, df):
    """y (n, D): whitened points of ONE cluster, y = sqrt(df / g) z under the law.  Raises AssertionError on the first check missed.

    KS tests.  For a continuous law, P(sqrt(n) D_n > lambda) -> 2 sum_j (-1)^(j-1) exp(-2 j^2 lambda^2) <= 2 exp(-2 lambda^2); with
    lambda = 3.3 that is 7e-10 per test: some 20 tests in each of 9 cases stay below 2e-7 in all.
      * q = y'y / D = (z'z / D) / (g / df) is a ratio of independent chi^2 / dof: F(D, df).
      * every coordinate y_a = z_a / sqrt(g / df) is Student-t(df).
    Correlations.  E y_a y_b = 0 and, with s = df / g, E y_a^2 y_b^2 = E s^2 = Var(y)^2 (df - 2) / (df - 4) for a != b: the sample
    correlation of n points is asymptotically N(0, (df - 2) / ((df - 4) n)); for df >= 50 its sd is below 1.022 / sqrt(n), so the bound
    6 / sqrt(n) is 5.87 sd: 4e-9 per pair, 1.4e-4 over the 32640 pairs of D = 256.
    Variances.  Var y_a = df / (df - 2), kurtosis 3 (df - 2) / (df - 4): the sample variance has relative variance (kurtosis - 1) / n =
    2 (df - 1) / ((df - 4) n); the bound is 6 of those sd: 2e-9 per coordinate."""
    y = np.asarray(y, np.float64)
    n, D = y.shape
    assert np.isfinite(y).all(), "non-finite whitened points"
    lim = KS_LAMBDA / np.sqrt(n)
    dq = ks_distance((y * y).sum(1) / D, stats.f(D, df).cdf)
    assert dq < lim, f"q = y'y / D against F({D}, {df}): KS distance {dq:.5f} >= {lim:.5f}"
    t = stats.t(df)
    for a in tested_coordinates(D):
        da = ks_distance(y[:, a], t.cdf)
        assert da < lim, f"coordinate {a} against t({df}): KS distance {da:.5f} >= {lim:.5f}"
    var = y.var(0)
    rel = np.abs(var / (df / (df - 2.0)) - 1.0)
    vlim = 6.0 * np.sqrt(2.0 * (df - 1.0) / ((df - 4.0) * n))
    assert rel.max() < vlim, f"variance of coordinate {int(rel.argmax())}: relative deviation {rel.max():.5f} >= {vlim:.5f}"
    if D > 1:
        c = np.corrcoef(y.T)
        np.fill_diagonal(c, 0.0)
        worst = np.abs(c).max()
        assert worst < 6.0 / np.sqrt(n), f"correlation {np.unravel_index(np.abs(c).argmax(), c.shape)}: {worst:.5f} >= {6.0 / np.sqrt(n):.5f}"


# ------------------------------------------------------------------------------------------------ models
def niw_model(D, K, df, seed, offdiag=None):
    """A hand-made NIW posterior: (post dict, m, A, df) with A = sqrt(c) U as the Predictor forms it.  U has a unit-scale diagonal and
    off-diagonal entries of at least half of `offdiag` (default 1 / sqrt(D): A' A then differs from A A' clearly at every D > 1)."""
    rng = np.random.default_rng(seed)
    df = np.broadcast_to(np.asarray(df, np.float64), (K,)).copy()
    kappa = rng.uniform(1.0, 20.0, K)
    nu = df + D - 1
    m = rng.standard_normal((K, D)).astype(np.float32).astype(np.float64)
    off = 1.0 / np.sqrt(D) if offdiag is None else offdiag
    r = rng.standard_normal((K, D, D))
    U = np.triu(off * np.sign(r) * (0.5 + np.abs(r)), 1)           # (no entry near zero: a transposed factor differs at D = 2 as well)
    U[:, np.arange(D), np.arange(D)] = rng.uniform(0.7, 1.4, (K, D))
    U = U * np.sqrt(nu)[:, None, None]
    c = (kappa + 1) / (kappa * df)
    return dict(kappa=kappa, nu=nu, m=m, U=U), m, np.sqrt(c)[:, None, None] * U, df


def predictor_file(kind, D, alpha, points_count, post):
    """An in-memory .npz that Predictor.load reads (the format of Predictor.save)."""
    f = io.BytesIO()
    np.savez(f, kind=np.int64(kind), D=np.int64(D), alpha=np.float64(alpha), points_count=np.asarray(points_count, np.float64),
             **{"post_" + k: v for k, v in post.items()})
    f.seek(0)
    return f
