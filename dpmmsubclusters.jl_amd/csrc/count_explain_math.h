// count_explain_math.h -- the Float64 arithmetic of include/dpmm_hip_count_explain.h for ONE feature of one count point: the binomial
// deviance g_d, the side of the deviation, the residual and the exact one-sided binomial tail.  Plain C++ without a device call other than
// the maths library's (as typicality_math.h, whose functions it uses), so that a host program can check it against another evaluation.
// One piece of code for the three stores: the bits of a feature depend on (x, t, log theta, log1p(-theta)) alone.
#pragma once
#include "typicality_math.h"

namespace dpmm {

constexpr double CE_SNAP = 0x1p-40;      // x and t theta are taken as EQUAL when |log(x / (t theta))| is at most this (see ce_side_of)
constexpr double CE_LOG_HALF = -0.6931471805599453;

// theta and 1 - theta from their logarithms, each on the side where the exponential loses nothing: exp of the logarithm that is small,
// -expm1 of it for the other one.  (Only the tail kernel needs them: the ranking works on the logarithms alone.)
TYP_HD void ce_theta(double lth, double l1m, double &th, double &thc) {
    if (lth > CE_LOG_HALF) { th = exp(lth); thc = -expm1(lth); }
    else { thc = exp(l1m); th = -expm1(l1m); }
}

// g = 2 [x (log x - log t - log theta) + (t - x)(log(t - x) - log t - log1p(-theta))], lt = log(t); a term whose factor is 0 is exactly 0.
// Two logarithms, three subtractions and one product per term, one sum: the operations the header's bound counts.  For x == 0 the first
// term is 0 and log(t - x) - lt is 0 exactly, so g = 2 (t (-l1m)): the bits of ce_deviance_unseen.  Rounding can leave g a little below
// 0 next to x = t theta: 0 then.
TYP_HD double ce_deviance(double x, double t, double lt, double lth, double l1m) {
    const double y = t - x;
    const double t1 = x > 0. ? x * ((log(x) - lt) - lth) : 0.;
    const double t2 = y > 0. ? y * ((log(y) - lt) - l1m) : 0.;
    const double g = 2. * (t1 + t2);
    return g > 0. ? g : 0.;
}
// ... of a feature the point does not hold: one product, no logarithm
TYP_HD double ce_deviance_unseen(double t, double l1m) {
    const double g = 2. * (t * (0. - l1m));
    return g > 0. ? g : 0.;
}

// +1: x > t theta (over), -1: x < t theta (under), 0: equal -- from u = log x - log t - log theta, the factor of the deviance's first term,
// the same bits.  theta reaches the device as a logarithm, so "equal" is |u| <= CE_SNAP: u carries a rounding error of a few 2^-53 of the
// logarithms' size, far inside the band, and the deviance inside the band is below 2^-79 x, far below its own rounding error.  For x == 0:
// theta > 0 exactly when l1m < 0, nothing else is needed.
TYP_HD int ce_side_of(double x, double lt, double lth, double l1m) {
    if (!(x > 0.)) return l1m < 0. ? -1 : 0;
    const double u = (log(x) - lt) - lth;
    return fabs(u) <= CE_SNAP ? 0 : (u > 0. ? 1 : -1);
}

// |residual| as returned, sqrt(g) rounded to Float32 once, and the side (0: the residual is 0).  x >= 0, t > 0, x <= t.
TYP_HD float ce_score(double x, double t, double lt, double lth, double l1m, int *side) {
    *side = ce_side_of(x, lt, lth, l1m);
    if (*side == 0) return 0.f;
    return (float)sqrt(x > 0. ? ce_deviance(x, t, lt, lth, l1m) : ce_deviance_unseen(t, l1m));
}

// The exact one-sided tail on the side of the deviation: over P(X >= x) = I_theta(x, t - x + 1), under P(X <= x) = I_{1-theta}(t - x, x + 1),
// X ~ Binomial(t, theta); the two ends in closed form (theta^t and (1 - theta)^t); equal: 1.  For values that are no integers the same
// formulas are the continuous extension, no probability statement.
TYP_HD double ce_tail(double x, double t, int side, double lth, double l1m, int *trips) {
    if (trips) *trips = 0;
    if (side == 0) return 1.;
    double th, thc;
    ce_theta(lth, l1m, th, thc);
    if (side > 0) return x < t ? typ_inc_beta(x, t - x + 1., th, thc, lth, l1m, trips) : exp(t * lth);
    return x > 0. ? typ_inc_beta(t - x, x + 1., thc, th, l1m, lth, trips) : exp(t * l1m);
}

}  // namespace dpmm
