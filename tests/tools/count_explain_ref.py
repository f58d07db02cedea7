"""numpy + mpmath reference of include/dpmm_hip_count_explain.h: the binomial deviance residuals and exact one-sided tails of the features of
a count point under Binomial(t, theta_kd), the header's bounds and a checker of what `Predictor.explain_counts` returns.  Dense, straight.

  theta_of(alpha)                     alpha' / sum(alpha') in Float64
  dense(X)                            (D, n) float64 from a dense array or a scipy sparse matrix
  side_of(x, t, th)                   +1 over, -1 under, 0 where |log(x / (t theta))| <= 2^-40
  deviance(x, t, th)                  g and the size A1 + A2 of what cancels in it, in extended precision (numpy longdouble: 2^-64)
  tail_mp(x, t, th, side)             the exact tail by mpmath.betainc(..., regularized=True) at 50 digits; for integers with t >= 1000, where
                                      that series does not converge, by the finite binomial sum it equals, in the same arithmetic
  tail_fast(x, t, th, side)           the same by scipy.special.betainc / betaincc (the incomplete beta function itself, not 1 - cdf)
  topm(r32, cand, m)                  the definition on given values: a stable sort of -|r| over the candidates
  check(got, X, theta, top, side)     every property the header states, for every point; returns the worst ratios to the two bounds
"""
import mpmath
import numpy as np
import scipy.special as ss

SNAP = 2.0 ** -40
U = 2.0 ** -53
EPS32 = 2.0 ** -24 * (1 + 2.0 ** -20) + 2.0 ** -52      # one Float32 rounding of a Float64 square root
TAIL_REL = 2.0 ** -20
TAIL_FLOOR = 1e-30
SIDES = {"both": None, "over": 1, "under": -1}


def theta_of(alpha):
    a = np.asarray(alpha, np.float64)
    return a / a.sum(1, keepdims=True)


def dense(X):
    return np.asarray(X.toarray() if hasattr(X, "toarray") else X, np.float64)


def side_of(x, t, th):
    """+1 over, -1 under, 0 equal: |log(x / (t th))| <= 2^-40 counts as equal (theta reaches the device as its logarithm; the rounding of
    that difference, a few 2^-53 of the logarithms' size, lies far inside the band).  x == 0 is under for every th > 0."""
    L = np.longdouble
    x, t, th = np.broadcast_arrays(np.asarray(x, L), np.asarray(t, L), np.asarray(th, L))
    with np.errstate(all="ignore"):
        u = np.log(np.where(x > 0, x, 1)) - np.log(t) - np.log(th)
    return np.where(x > 0, np.where(np.abs(u) <= SNAP, 0, np.where(u > 0, 1, -1)), np.where(th > 0, -1, 0)).astype(np.int64)


def deviance(x, t, th):
    """(g, A): g = 2 [x (log x - log t - log th) + (t - x)(log(t - x) - log t - log1p(-th))], a term whose factor is 0 exactly 0, and
    A = x (|log x| + |log t| + |log th|) + (t - x)(|log(t - x)| + |log t| + |log1p(-th)|)."""
    L = np.longdouble
    x, t, th = np.broadcast_arrays(np.asarray(x, L), np.asarray(t, L), np.asarray(th, L))
    y = t - x
    with np.errstate(all="ignore"):
        lx, ly, lt, lth, l1m = np.log(np.where(x > 0, x, 1)), np.log(np.where(y > 0, y, 1)), np.log(t), np.log(th), np.log1p(-th)
        t1 = np.where(x > 0, x * (lx - lt - lth), 0)
        t2 = np.where(y > 0, y * (ly - lt - l1m), 0)
        A = np.where(x > 0, x * (abs(lx) + abs(lt) + abs(lth)), 0) + np.where(y > 0, y * (abs(ly) + abs(lt) + abs(l1m)), 0)
    return np.maximum(2 * (t1 + t2), 0).astype(np.float64), A.astype(np.float64)


def _binomial_sum(x, t, th, step):
    """sum of C(t, j) th^j (1 - th)^(t - j) over j = x, x + step, ... for integers, away from the mean: the terms fall monotonically, the
    sum stops when they fall below 1e-20 of it (the contract is 2^-20)."""
    term = mpmath.exp(mpmath.loggamma(t + 1) - mpmath.loggamma(x + 1) - mpmath.loggamma(t - x + 1) + x * mpmath.log(th) + (t - x) * mpmath.log1p(-th))
    total, j, odds = mpmath.mpf(0), x, th / (1 - th)
    while 0 <= j <= t and term > total * mpmath.mpf(10) ** -20:
        total += term
        term = term * (t - j) / (j + 1) * odds if step > 0 else term * j / (t - j + 1) / odds
        j += step
    return total


def tail_mp(x, t, th, side):
    if side == 0:
        return mpmath.mpf(1)
    with mpmath.workdps(50):
        x, t, th = mpmath.mpf(float(x)), mpmath.mpf(float(t)), mpmath.mpf(float(th))
        if t >= 1000 and x == int(x) and t == int(t) and 0 < x < t:      # (mpmath's series for betainc takes seconds here, then gives up)
            return _binomial_sum(x, t, th, 1 if side > 0 else -1)
        try:
            if side > 0:
                return mpmath.betainc(x, t - x + 1, 0, th, regularized=True) if x < t else th ** t
            return mpmath.betainc(t - x, x + 1, 0, 1 - th, regularized=True) if x > 0 else (1 - th) ** t
        except (ValueError, ZeroDivisionError, mpmath.libmp.NoConvergence):      # mpmath's series gave up (large arguments): for integers the same number is a finite sum
            assert x == int(x) and t == int(t), (x, t, th)
            return _binomial_sum(x, t, th, 1 if side > 0 else -1)


def tail_fast(x, t, th, side):
    x, t, th, side = np.broadcast_arrays(np.asarray(x, np.float64), t, th, side)
    with np.errstate(all="ignore"):
        over = np.where(x < t, ss.betainc(np.maximum(x, 1e-300), t - x + 1, th), np.exp(t * np.log(th)))
        under = np.where(x > 0, ss.betaincc(x + 1, np.maximum(t - x, 1e-300), th), np.exp(t * np.log1p(-th)))
    return np.where(side == 0, 1.0, np.where(side > 0, over, under))


def topm(r32, cand, m):
    """(features (m,) int32, -1 behind the candidates) of one point: |r32| descending, ties to the lower index."""
    idx = np.flatnonzero(cand)
    order = idx[np.argsort(-np.abs(r32[idx]), kind="stable")][:m]
    out = np.full(m, -1, np.int32)
    out[:len(order)] = order
    return out


def explain(X, labels, theta, top, side):
    """The definitions on a dense matrix: (features, count, expected, residual, tail) with Float32 roundings of the extended-precision
    values -- what an exact evaluation returns; the GPU's may differ within the bounds, so `check` compares with intervals, not with this."""
    X = dense(X)
    D, n = X.shape
    want = SIDES[side]
    F = np.full((n, top), -1, np.int32)
    C, E, R, T = (np.full((n, top), np.nan, np.float32) for _ in range(4))
    for i in range(n):
        x, t, th = X[:, i], X[:, i].sum(), theta[labels[i] - 1]
        if not (np.isfinite(x).all() and (x >= 0).all() and t > 0):
            continue
        s = side_of(x, t, th)
        g, _ = deviance(x, t, th)
        r = (s * np.sqrt(np.where(s == 0, 0, g))).astype(np.float32)
        f = topm(r, np.ones(D, bool) if want is None else s == want, top)
        k = f >= 0
        F[i], C[i, k], E[i, k], R[i, k] = f, x[f[k]], (t * th[f[k]]), r[f[k]]
        T[i, k] = tail_fast(x[f[k]], t, th[f[k]], s[f[k]])
    return F, C, E, R, T


def check(got, X, theta, top, side, what="", mp_budget=150, integer=True, skip_rows=None, l1m=None):
    """Asserts the header's statements for every point; got: a CountExplanation of numpy arrays; skip_rows: (n,) bool, the points whose row of
    the table has a NaN or no finite entry (what `predict` marks with NaN probabilities).  Every returned residual against the
    interval the bound on g and the Float32 rounding leave, every tail against scipy's incomplete beta function with a margin of 2^-26
    for its own error and -- the yardstick -- the `mp_budget` smallest, largest and first tails of the case against mpmath at 50 digits.
    A left-out candidate may not rank above the last one returned: by its interval, and for the features the point does not hold, whose
    Float32 residual is known to the bit from `l1m` (default log1p(-theta), what Predictor hands over), by the key itself, ties included.
    Returns (worst residual ratio, worst tail ratio)."""
    X = dense(X)
    D, n = X.shape
    want = SIDES[side]
    l1m = np.log1p(-np.asarray(theta, np.float64)) if l1m is None else np.asarray(l1m, np.float64)      # (the table the worker was handed)
    F, C, E, R, T, lab, tot = (np.asarray(a) for a in (got.features, got.count, got.expected, got.residual, got.feature_tail, got.labels, got.total))
    assert F.shape == C.shape == E.shape == R.shape == T.shape == (n, top) and F.dtype == np.int32 and tot.dtype == np.float64, what
    assert all(a.dtype == np.float32 for a in (C, E, R, T)), what
    worst_r, worst_t, n_sk, n_inc, mp_jobs = 0.0, 0.0, 0, 0, []
    for i in range(n):
        x = X[:, i]
        blank = (F[i] == -1).all() and all(np.isnan(a[i]).all() for a in (C, E, R, T))
        if skip_rows is not None and skip_rows[i]:
            n_sk += 1
            assert blank and np.isnan(tot[i]), (what, i, "a skipped point")
            continue
        t = x.sum() if np.isfinite(x).all() else np.nan
        if not (np.isfinite(x).all() and (x >= 0).all() and t > 0):
            n_inc += 1
            assert blank, (what, i, "an incomplete point")
            continue
        if integer:
            assert tot[i] == t, (what, i, "total")
        t = tot[i]
        th = theta[lab[i] - 1]
        s = side_of(x, t, th)
        g, A = deviance(x, t, th)
        Eg = 16 * U * A
        lo = np.where(s == 0, 0, np.sqrt(np.maximum(g - Eg, 0)) * (1 - EPS32))
        hi = np.where(s == 0, 0, np.sqrt(g + Eg) * (1 + EPS32))
        cand = np.ones(D, bool) if want is None else s == want
        nc = min(top, int(cand.sum()))
        assert (F[i, nc:] == -1).all() and all(np.isnan(a[i, nc:]).all() for a in (C, E, R, T)), (what, i, "slots beyond the candidates")
        f, r = F[i, :nc], R[i, :nc]
        assert ((f >= 0) & (f < D)).all() and len(set(f.tolist())) == nc and cand[f].all(), (what, i, "features", f)
        assert np.array_equal(C[i, :nc], x[f].astype(np.float32)), (what, i, "count")
        assert (np.abs(E[i, :nc] - t * th[f]) <= 2.0 ** -22 * t * th[f]).all(), (what, i, "expected")
        a = np.abs(r).astype(np.float64)
        assert (np.sign(r) == s[f]).all() or (a[np.sign(r) != s[f]] == 0).all(), (what, i, "the sign of the residual", r, s[f])
        assert ((a >= lo[f]) & (a <= hi[f])).all(), (what, i, "residual is outside the bound", a, lo[f], hi[f])
        rs = np.sqrt(g[f])
        with np.errstate(all="ignore"):
            ratio = np.where(a >= rs, (a - rs) / (hi[f] - rs), (rs - a) / (rs - lo[f]))
        worst_r = max(worst_r, float(np.nanmax(ratio, initial=0.0)))
        bits = a.astype(np.float32).view(np.uint32)
        assert (np.diff(a) <= 0).all(), (what, i, "|residual| increases")
        assert (np.diff(f)[bits[1:] == bits[:-1]] > 0).all(), (what, i, "equal bits, decreasing feature")
        rest = cand.copy()
        rest[f] = False
        # a feature the point does not hold has ONE product and no logarithm: its Float32 residual is known to the bit
        un32 = np.sqrt(2 * (t * (0 - l1m[lab[i] - 1]))).astype(np.float32)
        zero = x[f] == 0
        assert np.array_equal(a.astype(np.float32)[zero], un32[f][zero]), (what, i, "the residual of an unseen feature", a[zero], un32[f][zero])
        if nc and rest.any():
            assert (lo[rest] <= a.min()).all(), (what, i, "a better candidate was left out", np.flatnonzero(rest)[lo[rest] > a.min()])
            last = np.float32(a[-1])
            z = rest & (x == 0)
            beats = z & ((un32 > last) | ((un32 == last) & (np.arange(D) < f[-1])))
            assert not beats.any(), (what, i, "an unseen candidate that ranks above the last one returned was left out", np.flatnonzero(beats), f)
        ref = tail_fast(x[f], t, th[f], s[f])
        tl = T[i, :nc].astype(np.float64)
        big = ref >= TAIL_FLOOR
        assert (np.abs(tl - ref)[big] <= (TAIL_REL - 2.0 ** -26) * ref[big]).all(), (what, i, "tail is outside the contract", tl, ref)
        assert ((tl[~big] >= 0) & (tl[~big] <= TAIL_FLOOR * (1 + TAIL_REL))).all(), (what, i, "a tail below the floor")
        mp_jobs += [(float(ref[j]), i, int(f[j]), float(x[f[j]]), float(t), float(th[f[j]]), int(s[f[j]]), float(tl[j])) for j in range(nc)]
    # the yardstick: mpmath on the smallest, the largest and the first tails of the case
    mp_jobs.sort()
    third = max(1, mp_budget // 3)
    picked = mp_jobs[:third] + mp_jobs[-third:] + sorted(mp_jobs, key=lambda q: q[1:3])[:third] if len(mp_jobs) > mp_budget else mp_jobs
    for _, i, d, x, t, th, s, tl in picked:
        ex = tail_mp(x, t, th, s)
        if ex >= TAIL_FLOOR:
            err = float(abs(mpmath.mpf(tl) - ex) / ex)
            assert err <= TAIL_REL, (what, i, d, "tail against mpmath", tl, ex)
            worst_t = max(worst_t, err / TAIL_REL)
        else:
            assert 0 <= tl <= TAIL_FLOOR * (1 + TAIL_REL), (what, i, d, "a tail below the floor against mpmath", tl, ex)
    assert got.skipped == n_sk and got.incomplete == n_inc, (what, "counters", got.skipped, n_sk, got.incomplete, n_inc)
    return worst_r, worst_t

