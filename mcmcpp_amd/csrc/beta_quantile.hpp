// beta_quantile.hpp -- mcmcpp::beta_quantile(p, a, b): the x in (0, 1) with I_x(a, b) = p, the quantile function of the Beta
// distribution, which mcmcpp_hip_posterior_summary needs for the Monte Carlo standard error of a quantile.  Host only, <cmath>
// only, deterministic: no random start, no table, the same sequence of operations for the same arguments.
//
// Specified to an ACCURACY, not to bits: it calls the host libm (lgamma, log, log1p, exp, sqrt), whose last bits differ between
// libraries.  For a, b in [1, 2^31 + 2] and p in (0, 1) the relative error of the result is below 1e-10
// (tests/test_beta_quantile.py, against a 50-digit inverse).  Larger a and b (an effective sample size may exceed the number of
// draws) take the same path; the caps below then bound the work, not the accuracy, up to a + b of about 10^11.
//
// Algorithm
//   I_x(a, b)   for x <= (a + 1) / (a + b + 2):  front(a, b, x) cf(a, b, x) / a, otherwise 1 - front(b, a, 1 - x) cf(b, a, 1 - x) / b,
//               with cf the continued fraction of Numerical Recipes' betacf evaluated by the modified Lentz method: at most
//               kBetaCfCap = 1 000 000 terms (it needs about sqrt(max(a, b)) of them), until a factor differs from 1 by less
//               than 3e-16.
//   front       x^a (1 - x)^b / B(a, b) without the cancellation of lgamma(a + b) - lgamma(a) - lgamma(b):
//               a, b >= 16: sqrt(a b / (2 pi (a + b))) exp(-(a r(-l / a) + b r(l / b))) exp(-(d(a) + d(b) - d(a + b))), where
//                           l = a - (a + b) x, r(e) = e - log(1 + e) (by its series in e / (2 + e) for |e| <= 0.3) and d the
//                           Stirling correction 1 / (12 z) - 1 / (360 z^3) + 1 / (1260 z^5) - 1 / (1680 z^7) (DiDonato and Morris 1992)
//               the larger >= 16: lgamma(a + b) - lgamma(larger) from Stirling's formula with the same d
//               both < 16:  lgamma as it is
//   inverse     Newton's method on I_x(a, b) - p from the mean a / (a + b), with derivative front / (x (1 - x)), kept inside a
//               bracket [lo, hi] that every evaluation shrinks; a step that leaves the bracket, or does not halve the last
//               one, is replaced by a bisection.  At most kBetaNewtonCap = 200 evaluations, until the step is below 1e-15 x.
#pragma once

#include <cmath>

namespace mcmcpp
{
constexpr int kBetaCfCap = 1000000;
constexpr int kBetaNewtonCap = 200;

// e - log(1 + e), e > -1
inline double beta_rlog1(double e)
{
    if (e < -0.3 || e > 0.3) return e - std::log1p(e);
    // log(1 + e) = 2 (r + r^3 / 3 + r^5 / 5 + ...) with r = e / (2 + e), and e - 2 r = e r
    const double r = e / (2.0 + e), t = r * r;
    double sum = 0.0;
    for (int k = 14; k >= 1; --k) sum = sum * t + 1.0 / (2.0 * k + 1.0);  // 1/3 + t/5 + t^2/7 + ...
    return r * (e - 2.0 * t * sum);
}

// lgamma(z) - ((z - 0.5) log z - z + 0.5 log(2 pi)), z >= 16
inline double beta_stirling_rest(double z)
{
    const double w = 1.0 / (z * z);
    return (1.0 / 12.0 - w * (1.0 / 360.0 - w * (1.0 / 1260.0 - w * (1.0 / 1680.0)))) / z;
}

// x^a y^b / B(a, b), y = 1 - x
inline double beta_front(double a, double b, double x, double y)
{
    const double kLarge = 16.0;
    if (a >= kLarge && b >= kLarge)
    {
        const double lambda = x <= y ? a - (a + b) * x : (a + b) * y - b;
        const double u = beta_rlog1(-lambda / a), v = beta_rlog1(lambda / b);
        const double rest = beta_stirling_rest(a) + beta_stirling_rest(b) - beta_stirling_rest(a + b);
        return std::sqrt(a * b / (6.283185307179586476925 * (a + b))) * std::exp(-(a * u + b * v)) * std::exp(-rest);
    }
    const double s = a < b ? a : b, l = a < b ? b : a;
    double log_inv_beta;  // log(1 / B(a, b))
    if (l >= kLarge)      // lgamma(s + l) - lgamma(l) = (l - 0.5) log(1 + s / l) + s log(s + l) - s + d(s + l) - d(l)
        log_inv_beta = (l - 0.5) * std::log1p(s / l) + s * std::log(s + l) - s + (beta_stirling_rest(s + l) - beta_stirling_rest(l)) - std::lgamma(s);
    else
        log_inv_beta = std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b);
    return std::exp(a * std::log(x) + b * std::log1p(-x) + log_inv_beta);
}

// the continued fraction of I_x(a, b) (modified Lentz), for x <= (a + 1) / (a + b + 2)
inline double beta_cf(double a, double b, double x)
{
    const double tiny = 1e-300, eps = 3e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= kBetaCfCap; ++m)
    {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return h;
}

// I_x(a, b); *density = x^(a-1) (1 - x)^(b-1) / B(a, b)
inline double beta_cdf(double a, double b, double x, double* density)
{
    const double y = 1.0 - x;
    const double front = beta_front(a, b, x, y);
    *density = front / (x * y);
    if (x <= (a + 1.0) / (a + b + 2.0)) return front * beta_cf(a, b, x) / a;
    return 1.0 - front * beta_cf(b, a, y) / b;
}

inline double beta_quantile(double p, double a, double b)
{
    double lo = 0.0, hi = 1.0, x = a / (a + b), last = 1.0;
    for (int it = 0; it < kBetaNewtonCap; ++it)
    {
        double density;
        const double f = beta_cdf(a, b, x, &density) - p;
        if (f == 0.0) return x;
        if (f < 0.0)
            lo = x;
        else
            hi = x;
        double step = f / density, next = x - step;
        if (!(density > 0.0) || !(next > lo && next < hi) || std::fabs(step) > 0.5 * last)
        {
            next = lo + 0.5 * (hi - lo);
            step = x - next;
        }
        last = std::fabs(step);
        const bool done = last <= 1e-15 * next || next == x;
        x = next;
        if (done) break;
    }
    return x;
}
}  // namespace mcmcpp
