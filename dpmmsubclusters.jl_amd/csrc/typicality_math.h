// typicality_math.h -- the Float64 tail of include/dpmm_hip_typicality.h, tail(q) = I_x(a, b) with a = df / 2, b = D / 2, x = df / (df + q):
// the regularised incomplete beta function by its continued fraction (modified Lentz), evaluated on the side where it converges fast.
// Plain C++ without a device call other than the maths library's, so that a host program can check it against another evaluation.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TYP_HD __host__ __device__ __forceinline__
#else
#define TYP_HD inline
#endif

namespace dpmm {

constexpr int TYP_CF_MAX = 20000;          // trips of the continued fraction at most: it needs O(sqrt(max(a, b))) of them, 2.3e3 at df = 1e7
constexpr double TYP_CF_EPS = 2.5e-16;     // it stops when a factor lies this close to 1
constexpr double TYP_CF_TINY = 1e-300;
constexpr double TYP_STIRLING_MIN = 32.0;  // from here on lgamma(a + b) - lgamma(a) is formed from the Stirling series of the difference

// the tail of Stirling's series: lgamma(z) = (z - 1/2) log z - z + log(2 pi) / 2 + typ_stirling(z); the next term is below 1e-3 z^-9
TYP_HD double typ_stirling(double z) {
    const double r = 1.0 / z, r2 = r * r;
    return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
}

// log B(a, b) = lgamma(a) + lgamma(b) - lgamma(a + b).  For large a the two big terms (a log a each, 7e7 at df = 1e7) are never formed:
// lgamma(a + b) - lgamma(a) = (a - 1/2) log1p(b / a) + b log(a + b) - b + the difference of the series' tails, terms of size b log a.
TYP_HD double typ_log_beta(double a, double b) {
    if (a < TYP_STIRLING_MIN) return lgamma(a) + lgamma(b) - lgamma(a + b);
    const double d = (a - 0.5) * log1p(b / a) + b * log(a + b) - b + (typ_stirling(a + b) - typ_stirling(a));
    return lgamma(b) - d;
}

// the continued fraction of I_x(a, b) (Numerical Recipes' betacf, modified Lentz); *trips: the steps it took, TYP_CF_MAX if it ran out
TYP_HD double typ_beta_cf(double a, double b, double x, int *trips) {
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < TYP_CF_TINY) d = TYP_CF_TINY;
    d = 1.0 / d;
    double h = d;
    int m = 1;
    for (; m <= TYP_CF_MAX; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < TYP_CF_TINY) d = TYP_CF_TINY;
        c = 1.0 + aa / c;
        if (fabs(c) < TYP_CF_TINY) c = TYP_CF_TINY;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < TYP_CF_TINY) d = TYP_CF_TINY;
        c = 1.0 + aa / c;
        if (fabs(c) < TYP_CF_TINY) c = TYP_CF_TINY;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < TYP_CF_EPS) break;
    }
    if (trips) *trips = m < TYP_CF_MAX ? m : TYP_CF_MAX;
    return h;
}

// tail(q) for q >= 0 (q == 0: exactly 1; q = +Inf: 0), df > 0, D >= 1.  x and 1 - x are both formed without cancellation, from q and df.
TYP_HD double typ_tail(double q, double df, int D, int *trips) {
    if (trips) *trips = 0;
    if (!(q > 0.0)) return 1.0;
    if (!(q < INFINITY)) return 0.0;
    const double a = 0.5 * df, b = 0.5 * (double)D;
    const double x = df / (df + q), xc = q / (df + q);
    const double lpre = a * -log1p(q / df) + b * (log(q) - log(df + q)) - typ_log_beta(a, b);      // a log x + b log(1 - x) - log B(a, b)
    if (x < (a + 1.0) / (a + b + 2.0)) return exp(lpre) * typ_beta_cf(a, b, x, trips) / a;
    const double t = 1.0 - exp(lpre) * typ_beta_cf(b, a, xc, trips) / b;
    return t < 0.0 ? 0.0 : t;
}

// The general I_x(a, b) for a, b > 0 and 0 < x < 1 (count_explain.hip: the binomial tails of include/dpmm_hip_count_explain.h).  The caller
// hands over x AND xc = 1 - x, each formed without cancellation, and their logarithms lx, lxc -- it has them from its tables; a caller
// without passes log(x), log(xc).  The same two sides as typ_tail: the fraction that converges fast is the one that is evaluated.
TYP_HD double typ_inc_beta(double a, double b, double x, double xc, double lx, double lxc, int *trips) {
    if (trips) *trips = 0;
    const double lpre = a * lx + b * lxc - typ_log_beta(a, b);
    if (x < (a + 1.0) / (a + b + 2.0)) return exp(lpre) * typ_beta_cf(a, b, x, trips) / a;
    const double t = 1.0 - exp(lpre) * typ_beta_cf(b, a, xc, trips) / b;
    return t < 0.0 ? 0.0 : t;
}

}  // namespace dpmm
