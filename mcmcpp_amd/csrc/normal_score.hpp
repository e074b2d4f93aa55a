// normal_score.hpp -- z = Phi^-1(p), the normal score of a rank, as a function with one value in bits wherever it is compiled:
// the device (rank.hip), the host, and the numpy restatement of the tests (tests/rank_restatement.py) give the same double.
//
// The algorithm is Wichura's AS 241, routine PPND16 (Applied Statistics 37 (1988) 477-484), the public one that CPython's
// statistics.NormalDist.inv_cdf uses too.  This comment is the definition; every +, -, *, / below is an IEEE double operation
// rounded on its own (no fused multiply-add anywhere: compile with -ffp-contract=off, and under clang the functions say so
// themselves), the square root is the correctly rounded one, and the logarithm is normal_score_log below, not libm's or OCML's.
//
//   q = p - 0.5
//   |q| <= 0.425:   r = 0.180625 - q * q
//                   z = (q * A(r)) / B(r)
//   else:           t = p if q < 0, else 1.0 - p
//                   r = sqrt(-normal_score_log(t))
//                   r <= 5:  r = r - 1.6;  z = C(r) / D(r)
//                   else:    r = r - 5.0;  z = E(r) / F(r)
//                   z = -z if q < 0
//   A .. F are polynomials of degree 7 evaluated by Horner's rule from the highest coefficient down:
//   (((((((k7 * r + k6) * r + k5) * r + k4) * r + k3) * r + k2) * r + k1) * r + k0), with B, D, F's k0 = 1.0.
//
//   normal_score_log(x), x a positive normal number: fast_log.hpp's reduction and coefficients, without its fused operations:
//   x = 2^k m, m in [1, 2) from the bits of x; if m > 1.41421356237309504880: m = m * 0.5, k = k + 1
//   f = m - 1.0;  s = f / (2.0 + f);  z = s * s;  w = z * z
//   t1 = w * ((w * (w * Lg6 + Lg4)) + Lg2)
//   t2 = z * ((w * ((w * (w * Lg7 + Lg5)) + Lg3)) + Lg1)
//   R = t2 + t1;  hfsq = (0.5 * f) * f
//   log = k * ln2_hi + (f - (hfsq - (s * (hfsq + R) + k * ln2_lo)))
//
// p is (r - 0.375) / (S + 0.25) of an average rank r in [1, S], S >= 2: 0 < p < 1, and t is a positive normal number.
//
// Plain C++ (no HIP dependency) so that a CPU test can compile it (tests/test_normal_score.py).
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MCMCPP_NS_HD __host__ __device__ __forceinline__
#else
#define MCMCPP_NS_HD inline
#endif

namespace mcmcpp
{
MCMCPP_NS_HD double normal_score_log(double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
    uint64_t bits;
    memcpy(&bits, &x, 8);
    int k = (int)(bits >> 52) - 1023;
    bits = (bits & 0x000FFFFFFFFFFFFFULL) | 0x3FF0000000000000ULL;  // m in [1, 2)
    double m;
    memcpy(&m, &bits, 8);
    if (m > 1.41421356237309504880)
    {
        m = m * 0.5;
        k += 1;
    }
    const double f = m - 1.0;
    const double dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * ((w * (w * Lg6 + Lg4)) + Lg2);
    const double t2 = z * ((w * ((w * (w * Lg7 + Lg5)) + Lg3)) + Lg1);
    const double R = t2 + t1;
    const double hfsq = (0.5 * f) * f;
    return dk * ln2_hi + (f - (hfsq - (s * (hfsq + R) + dk * ln2_lo)));
}

MCMCPP_NS_HD double normal_score_poly(double r, double k7, double k6, double k5, double k4, double k3, double k2, double k1, double k0)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (((((((k7 * r + k6) * r + k5) * r + k4) * r + k3) * r + k2) * r + k1) * r + k0);
}

MCMCPP_NS_HD double normal_score(double p)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double q = p - 0.5;
    if ((q < 0.0 ? -q : q) <= 0.425)
    {
        const double r = 0.180625 - q * q;
        const double num = q * normal_score_poly(r, 2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                                                 1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0);
        const double den = normal_score_poly(r, 5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                                             5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0);
        return num / den;
    }
    const double t = q < 0.0 ? p : 1.0 - p;
    double r = __builtin_sqrt(-normal_score_log(t));
    double num, den;
    if (r <= 5.0)
    {
        r = r - 1.6;
        num = normal_score_poly(r, 7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
                                3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0);
        den = normal_score_poly(r, 1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                                6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0);
    }
    else
    {
        r = r - 5.0;
        num = normal_score_poly(r, 2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                                2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0);
        den = normal_score_poly(r, 2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                                1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0);
    }
    const double z = num / den;
    return q < 0.0 ? -z : z;
}

// the score of the average rank r = below + (equal + 1) / 2 among S draws: both halves of r are exact in double
MCMCPP_NS_HD double normal_score_of_rank(unsigned below, unsigned equal, unsigned S)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double r = (double)below + ((double)equal + 1.0) / 2.0;
    const double p = (r - 0.375) / ((double)S + 0.25);
    return normal_score(p);
}
}  // namespace mcmcpp
