// canonical.hpp -- a raw 64-bit engine output as a uniform variate in [0, 1), as libstdc++ makes it.
//
// Plain C++ (no HIP dependency), like fast_log.hpp, so that a CPU test can compile the very lines the kernels run and feed
// the sampler's own arguments to the logarithm under test (tests/cpp/fast_log_cases.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MCMCPP_HD __host__ __device__ __forceinline__
#else
#define MCMCPP_HD inline
#endif

namespace mcmcpp
{

// libstdc++ generate_canonical<T>(pcg64): T(r) rounded to nearest, divided by 2^64, clamped below 1
// (bits/random.tcc:3345-3380; MultiSampler.h:60,86 through uniform_real / exponential distributions)
MCMCPP_HD double canonical(uint64_t r, double)
{
    // u64 -> f64 round-to-nearest-even: hi*2^32 is exact, lo is exact, one rounded add
    const double hi = (double)(uint32_t)(r >> 32);
    const double lo = (double)(uint32_t)r;
    double u = __builtin_fma(hi, 4294967296.0, lo) * 5.42101086242752217003726400434970855712890625e-20;
    // fma(hi, 2^32, lo) rounds once (the product is exact), as the conversion instruction would
    if (u >= 1.0) u = 0.99999999999999988897769753748434595763683319091796875;
    return u;
}

MCMCPP_HD float canonical(uint64_t r, float)
{
    float u = (float)r * 5.42101086242752217003726400434970855712890625e-20f;
    if (u >= 1.0f) u = 0.999999940395355224609375f;
    return u;
}

}  // namespace mcmcpp
