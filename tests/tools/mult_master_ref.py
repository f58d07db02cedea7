"""A numpy restatement of the Multinomial device master (csrc/mult_master.hip): the Dirichlet draws of all 3K distributions by value, and
their log-marginals.  numpy / scipy only; nothing of the package is imported.

  * log_gamma_variates   log of Gamma(a, 1) variates: Marsaglia-Tsang in Float64 from Philox(seed; (row << 32) + 64 d + {2t, 2t + 1, 63},
                         epoch, stream 35) with 53-bit uniforms; a < 1: Gamma(a + 1) U^(1/a), carried in logs; acceptance forced for t > 28.
  * dirichlet_logp       [3K, D] Float32 log-probabilities (row order: cluster, left, right) from rows [2K, 1 + D] {N, sum x}.
  * log_marginals        N and the log-marginal of the 3K distributions and the pooled log-marginal of cluster pairs.

The draws are a deterministic Float64 function of (seed, epoch, row, d, alpha'): the device and this file round the same Float64
quantity to Float32.  Two conditions on the INPUTS say when that holds to one Float32 ulp; the functions return both measures:
  * margin     the smallest distance of a decisive comparison of the rejection loop from flipping (|1 + c x|, and |m1| where the squeeze
               accepted, |m2| where it did not).  Device and numpy log / cos / sqrt differ by a few Float64 ulp and the device contracts
               a * b + c: a comparison 1e-9 away from its edge falls the same way on both.
  * headroom   log p_d = lg_d - lse is a difference: its Float64 error is a few ulp of max(|lg_d|, |lse|), not of the result.  headroom
               is the smallest spacing(Float32(log p_d)) / (2^-52 max(|lg_d|, |lse|)) over the entries; an entry that is exactly zero
               counts as infinite when the mass of the other entries is below 2^-55 |lse| (it is zero on both sides: lse = max + log(1 + s)
               rounds to max) and as zero otherwise.  With headroom >= 64 a Float64 error of 8 ulp is an eighth of a Float32 ulp.

mutate=: deliberately WRONG variants that the comparisons must reject:
  "no_boost"                    the a < 1 branch is skipped (Marsaglia-Tsang run at a < 1 as it stands)
  "key_d"                       counter 64 d becomes d (neighbouring features share blocks)
  "f64_alpha"                   alpha' = alpha + sum formed in Float64
  "cluster_prior_for_outlier"   cluster 0 keeps the cluster prior under outlier_first
  "pair_prior_second"           a pooled pair takes the prior of its SECOND index
"""
import math

import numpy as np
from scipy.special import gammaln

from .sample_ref import _u53, philox

STREAM_MULT_DIR = 35
FORCED_AFTER = 28
MUTANTS = ("no_boost", "key_d", "f64_alpha", "cluster_prior_for_outlier", "pair_prior_second")


def _check(mutate):
    if mutate is not None and mutate not in MUTANTS:
        raise ValueError(mutate)


def log_gamma_variates(a, seed, row, epoch, mutate=None):
    """(log g, margin): log of a Gamma(a_d, 1) variate for every entry of a [..., D] (row: broadcast against a's leading axes),
    Float64; margin: see the module docstring (one number for the whole call)."""
    _check(mutate)
    a = np.array(a, np.float64, ndmin=1)
    shape = a.shape
    D = shape[-1]
    rows = np.broadcast_to(np.asarray(row, np.uint64)[..., None], shape)
    dd = np.broadcast_to(np.arange(D, dtype=np.uint64), shape)
    base = ((rows << np.uint64(32)) + (dd if mutate == "key_d" else np.uint64(64) * dd)).ravel()
    a = a.ravel().copy()
    boost = np.zeros(a.size)
    low = a < 1.0
    if low.any() and mutate != "no_boost":
        ru = philox(seed, base[low] + np.uint64(63), epoch, STREAM_MULT_DIR)
        boost[low] = np.log(_u53(ru[0], ru[1])) / a[low]
        a[low] += 1.0
    out = np.full(a.size, np.nan)
    margin = np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        d = a - 1.0 / 3.0
        c = 1.0 / np.sqrt(9.0 * d)
        live = np.arange(a.size)
        t = 0
        while live.size:
            assert t < 256, "Marsaglia-Tsang: 1 + c x <= 0 in every round"
            b = base[live]
            rn = philox(seed, b + np.uint64(2 * t), epoch, STREAM_MULT_DIR)
            ru = philox(seed, b + np.uint64(2 * t + 1), epoch, STREAM_MULT_DIR)
            x = np.sqrt(-2.0 * np.log(_u53(rn[0], rn[1]))) * np.cos(6.283185307179586476925 * _u53(rn[2], rn[3]))
            u = _u53(ru[0], ru[1])
            dl = d[live]
            v1 = 1.0 + c[live] * x
            go = ~(v1 <= 0.0)                                  # (a NaN is not <= 0: it goes on to the tests, as on the device)
            v = v1 * v1 * v1
            m1 = 1.0 - 0.0331 * x * x * x * x - u
            m2 = 0.5 * x * x + dl * (1.0 - v + np.log(v)) - np.log(u)
            squeeze = m1 > 0.0
            forced = t > FORCED_AFTER
            acc = go & (squeeze | (m2 > 0.0) | forced)
            near = [np.abs(v1)]
            if not forced:
                near.append(np.where(squeeze, np.abs(m1), np.abs(m2))[go])
            for m in near:
                m = m[np.isfinite(m)]
                if m.size:
                    margin = min(margin, float(m.min()))
            out[live[acc]] = np.log(dl[acc] * v[acc]) + boost[live[acc]]
            live = live[~acc]
            t += 1
    return out.reshape(shape), margin


def posterior_alpha(rows, alpha, alpha_outlier=None, outlier_first=False, mutate=None):
    """(N [3K], alpha' [3K, D] Float64 holding the Float32 values, prior [K, D] Float32) of the distributions cluster, left, right of every
    cluster: alpha' = alpha + Float32(sum x) formed in Float32; N = 0: the prior itself."""
    _check(mutate)
    rows = np.asarray(rows, np.float64)
    K, D = rows.shape[0] // 2, rows.shape[1] - 1
    if outlier_first and alpha_outlier is None:
        raise ValueError("outlier_first without an outlier prior")
    prior = np.broadcast_to(np.asarray(alpha, np.float32), (K, D)).copy()
    if outlier_first and mutate != "cluster_prior_for_outlier":
        prior[0] = np.asarray(alpha_outlier, np.float32)
    l, r = rows[0::2], rows[1::2]
    st = np.stack([l + r, l, r], axis=1)                       # [K, 3, 1 + D]
    if mutate == "f64_alpha":
        ap = prior.astype(np.float64)[:, None, :] + st[:, :, 1:]
    else:
        ap = (prior[:, None, :] + st[:, :, 1:].astype(np.float32)).astype(np.float64)
    ap = np.where(st[:, :, :1] == 0.0, prior.astype(np.float64)[:, None, :], ap)
    return st[:, :, 0].reshape(3 * K), ap.reshape(3 * K, D), prior


def dirichlet_logp(rows, alpha, alpha_outlier, outlier_first, seed, epoch, mutate=None):
    """(logp [3K, D] Float32, margin, headroom): log.(rand(Dirichlet(alpha'))) of all 3K distributions as the device draws them:
    float32(lg - logsumexp(lg)) with lg from log_gamma_variates(alpha'_j, seed, row j, epoch)."""
    _, ap, _ = posterior_alpha(rows, alpha, alpha_outlier, outlier_first, mutate)
    R = ap.shape[0]
    lg, margin = log_gamma_variates(ap, seed, np.arange(R, dtype=np.uint64), epoch, mutate)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = lg.max(axis=1)
        e = np.exp(lg - mx[:, None])
        total = np.array([math.fsum(r) if np.isfinite(r).all() else np.nan for r in e])
        lse = mx + np.log(total)
        r64 = lg - lse[:, None]
        out = r64.astype(np.float32)
        big = np.maximum(np.maximum(np.abs(lg), np.abs(lse)[:, None]), np.finfo(np.float64).tiny)
        ratio = np.spacing(np.abs(out)).astype(np.float64) / (2.0 ** -52 * big)
        others = np.maximum(total - 1.0, 0.0)                                         # (the largest entry contributes exp(0) = 1)
        sure_zero = (r64 == 0.0) & (others <= 2.0 ** -55 * np.abs(lse))[:, None]
        ratio = np.where(r64 == 0.0, np.where(sure_zero, np.inf, 0.0), ratio)
        headroom = float(np.nanmin(ratio)) if np.isfinite(r64).any() else np.nan
    return out, margin, headroom


def _lm(prior64, ap):
    """(log-marginal, scale): lgamma(sum a) - lgamma(sum a') + sum (lgamma(a'_d) - lgamma(a_d)), the four parts summed exactly
    (math.fsum); scale = |lgamma(sum a')| + sum |lgamma(a'_d)|, what the absolute tolerance of a comparison is derived from."""
    gp, ga = gammaln(ap), gammaln(prior64)
    top = float(gammaln(math.fsum(ap)))
    L = math.fsum([float(gammaln(math.fsum(prior64))), -top] + gp.tolist() + (-ga).tolist())
    return L, abs(top) + math.fsum(np.abs(gp))


def log_marginals(rows, alpha, alpha_outlier, outlier_first, pairs=(), mutate=None):
    """(N [3K], L [3K], P [npairs], scale_L [3K], scale_P [npairs]): the log-marginals of the Multinomial master
    (multinomial_prior.jl:34-39) of the 3K distributions and of the POOLED statistics (left + right of both clusters) of every pair
    (i, j), 0-based.  alpha' is formed in Float32 as the draws form it; L = 0 for N = 0 (posterior = prior); a pair takes the prior of
    its first index.  Evaluated with scipy.special.gammaln in Float64 and math.fsum (exact sums) -- tests/test_mult_master_ref_cpu.py
    holds it against mpmath at 50 digits."""
    N, ap, prior = posterior_alpha(rows, alpha, alpha_outlier, outlier_first, mutate)
    rows = np.asarray(rows, np.float64)
    K = rows.shape[0] // 2
    p64 = prior.astype(np.float64)
    L, sL = np.zeros(3 * K), np.zeros(3 * K)
    for j in range(3 * K):
        if N[j] != 0.0:
            L[j], sL[j] = _lm(p64[j // 3], ap[j])
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P, sP = np.zeros(len(pairs)), np.zeros(len(pairs))
    done = {}
    for n, (i, j) in enumerate(pairs.tolist()):
        if (i, j) not in done:
            st = rows[2 * i] + rows[2 * i + 1] + rows[2 * j] + rows[2 * j + 1]
            pr = prior[j if mutate == "pair_prior_second" else i]
            if st[0] == 0.0:
                done[(i, j)] = (0.0, 0.0)
            else:
                a = pr.astype(np.float64) + st[1:] if mutate == "f64_alpha" else (pr + st[1:].astype(np.float32)).astype(np.float64)
                done[(i, j)] = _lm(pr.astype(np.float64), a)
        P[n], sP[n] = done[(i, j)]
    return N, L, P, sL, sP


def ulp_distance(got, want):
    """|got - want| in units of np.spacing(want), Float32 (inf where either is not finite and they differ)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))
