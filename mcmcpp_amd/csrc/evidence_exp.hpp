// evidence_exp.hpp -- e = exp(x) for x <= 0, the weight of a draw in the evidence ratios (evidence.hip), as a function with one
// value in bits wherever it is compiled: the device, the host, and the numpy restatement of the tests
// (tests/evidence_restatement.py) give the same double.
//
// This comment is the definition; every +, -, *, / below is an IEEE double operation rounded on its own (no fused multiply-add
// anywhere: compile with -ffp-contract=off, and under clang the function says so itself), and nothing of libm or OCML is called.
//
//   x is NaN:                    x
//   x < -708.3964185322:         0.0   (the flush point: -1022 ln 2 = -708.39641853226..., cut off from above, so that every
//                                       result that is not flushed is a normal number; -inf is flushed)
//   else:  t = x * 1.4426950408889634 - 0.5;  k = t truncated towards zero (an integer in [-1022, 0]);  kd = k as a double
//          r = (x - kd * ln2_hi) - kd * ln2_lo          (ln2_hi, ln2_lo: fdlibm's, as in normal_score.hpp; kd * ln2_hi is exact)
//          q = (((((((((((c13 * r + c12) * r + c11) * r + c10) * r + c9) * r + c8) * r + c7) * r + c6) * r + c5) * r + c4) * r + c3) * r + c2)
//          p = 1.0 + (r + (r * r) * q)                   (c_n = 1 / n! rounded to double: the Taylor series, |r| < 0.3472)
//          e = p * 2^k                                   (2^k from its bits: exact; p in [1/sqrt 2, sqrt 2], so e is normal)
//   evidence_exp(0) = evidence_exp(-0.0) = 1 (k = 0, r = +-0, p = 1) and evidence_exp(-inf) = 0, exactly.
//
// The argument is u - max u of a draw: never positive.  (A positive x below 709 is served by the same lines; the function is
// not meant for one.)
//
// Plain C++ (no HIP dependency) so that a CPU test can compile it (tests/test_evidence_exp.py).
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MCMCPP_EE_HD __host__ __device__ __forceinline__
#else
#define MCMCPP_EE_HD inline
#endif

namespace mcmcpp
{
constexpr double kEvidenceExpFlush = -708.3964185322;

MCMCPP_EE_HD double evidence_exp(double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, inv_ln2 = 1.4426950408889634;
    const double c2 = 0.5, c3 = 0.16666666666666666, c4 = 0.041666666666666664, c5 = 0.008333333333333333, c6 = 0.001388888888888889,
                 c7 = 0.0001984126984126984, c8 = 2.48015873015873e-05, c9 = 2.7557319223985893e-06, c10 = 2.755731922398589e-07,
                 c11 = 2.505210838544172e-08, c12 = 2.08767569878681e-09, c13 = 1.6059043836821613e-10;
    if (x != x) return x;
    if (x < kEvidenceExpFlush) return 0.0;
    const double t = x * inv_ln2 - 0.5;
    const int k = (int)t;
    const double kd = (double)k;
    const double r = (x - kd * ln2_hi) - kd * ln2_lo;
    const double q = (((((((((((c13 * r + c12) * r + c11) * r + c10) * r + c9) * r + c8) * r + c7) * r + c6) * r + c5) * r + c4) * r + c3) * r + c2);
    const double p = 1.0 + (r + (r * r) * q);
    const uint64_t bits = (uint64_t)(1023 + k) << 52;
    double scale;
    memcpy(&scale, &bits, 8);
    return p * scale;
}
}  // namespace mcmcpp
