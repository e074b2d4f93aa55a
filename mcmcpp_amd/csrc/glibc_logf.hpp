// glibc_logf.hpp -- the natural logarithm of a float with the bits of glibc's logf, on the host and on the device.
//
// The reference computes the two logarithms of the accept test (ln z at MCMCpp/Movers/StretchMove.h:110, the exponential
// variate -log(1-u) at :113) with the host's logf.  In fp32 a device logarithm that differs from it in the last place can
// turn a decision inside the near-tie band the other way, after which the chains part; OCML's logf differs from glibc's on
// 49 % of all floats in [2^-24, 4].  This is a restatement of the algorithm of glibc 2.28 - 2.40 (a 16-entry table of
// {1/c, ln c}, a cubic in r = z/c - 1, everything in double and one rounding to float at the end), which returns glibc's
// bits on every float of that range with every operation rounded on its own, as the library and the tests build it
// (tests/test_glibc_logf.py: exhaustive on the host, and on the device against the host's logf); a build that fuses every
// multiply-add returns the same bits (checked exhaustively by hand, not in the suite).  glibc 2.41 replaced logf by a
// correctly rounded one; against such a host the exhaustive tests fail and print the C library's version.
//
// Plain C++ (no HIP dependency, no libm call), like fast_log.hpp, so that a CPU test can compile the very lines the
// kernels run.  Plug-in Calculators get it through mcmcpp_hip_plugin.hpp, host Calculators through
// include/MCMCpp/Device/GlibcLogf.h: an fp32 Calculator that takes a logarithm stays the same function on both sides.
#pragma once

#include <stdint.h>
#include <string.h>

#if !defined(MCMCPP_HD)
#if defined(__HIPCC__)
#define MCMCPP_HD __host__ __device__ __forceinline__
#else
#define MCMCPP_HD inline
#endif
#endif

namespace mcmcpp
{

// x must be a positive normal number (the kernels pass z in [1/2, 2] and 1-u in [2^-24, 1])
MCMCPP_HD float glibc_logf(float x)
{
    // {1/c, ln c} for the 16 subintervals of [0x1.66p-1, 0x1.66p0): c is near the centre of each
    // (on the device a table in constant memory, 16 bytes per lane in one load; see DESIGN.md section 6 for the placements tried)
    static constexpr double tab[16][2] = {
        {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
        {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
        {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
        {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
        {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
        {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
        {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
        {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2},
    };
    const double Ln2 = 0x1.62e42fefa39efp-1;
    const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
    uint32_t ix;
    memcpy(&ix, &x, 4);
    // (glibc returns 0 for x == 1 ahead of the rest; the rest gives +0 there as well -- i = 9, c = 1, r = 0 -- so that no
    // wavefront pays for a branch: the test asks for the bits of +0 at x == 1)
    // x = 2^k z with z in [0x1.66p-1, 0x1.66p0), split into 16 subintervals
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) & 15u);
    const int k = (int32_t)tmp >> 23;  // arithmetic shift
    const uint32_t iz = ix - (tmp & 0xff800000u);
    float zf;
    memcpy(&zf, &iz, 4);
    const double z = (double)zf;
    // ln x = ln(z/c) + ln c + k ln 2
    const double r = z * tab[i][0] - 1.0;
    const double y0 = tab[i][1] + (double)k * Ln2;
    const double r2 = r * r;
    double y = A1 * r + A2;
    y = A0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

}  // namespace mcmcpp
