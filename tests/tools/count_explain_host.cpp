// count_explain_host.cpp -- csrc/count_explain_math.h (and with it the general I_x(a, b) of csrc/typicality_math.h) as a host program, for
// tests/test_count_explain_cpu.py: reads lines "x t theta" from standard input and prints, per line,
//   side  |residual| (Float32)  g  tail  trips  I_theta(x, t - x + 1) by typ_inc_beta from log(theta), log1p(-theta)
// with 17 significant digits.  Build: g++ -O2 -std=c++17 -ffp-contract=off -I dpmmsubclusters.jl_amd/csrc count_explain_host.cpp
#include <cstdio>
#include "count_explain_math.h"

int main() {
    double x, t, th;
    while (std::scanf("%lf %lf %lf", &x, &t, &th) == 3) {
        const double lth = std::log(th), l1m = std::log1p(-th), lt = std::log(t);
        int side = 0, trips = 0;
        const float r = dpmm::ce_score(x, t, lt, lth, l1m, &side);
        const double g = x > 0. ? dpmm::ce_deviance(x, t, lt, lth, l1m) : dpmm::ce_deviance_unseen(t, l1m);
        const double tail = dpmm::ce_tail(x, t, side, lth, l1m, &trips);
        const double ib = (x > 0. && x < t) ? dpmm::typ_inc_beta(x, t - x + 1., th, 1. - th, lth, l1m, nullptr) : -1.;
        std::printf("%d %.9g %.17g %.17g %d %.17g\n", side, (double)r, g, tail, trips, ib);
    }
    return 0;
}
