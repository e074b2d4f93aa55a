// glibc_logf_cases.cpp -- mcmcpp::glibc_logf (mcmcpp_amd/csrc/glibc_logf.hpp) against the platform's logf, on the CPU.
//
// Built by tests/test_glibc_logf.py with g++ and with hipcc's host pass, -ffp-contract=off, and once more with
// -fsanitize=address,undefined.  GLIBC_LOGF_HEADER names the include path under test (the kernels' header by default, the
// public twin include/MCMCpp/Device/GlibcLogf.h where the test says so).
//
//   glibc_logf_cases                     every float in [2^-24, 4] (x = 1 among them): 218 103 809 arguments
//   glibc_logf_cases FIRST LAST          every float whose bits are in [FIRST, LAST] (hexadecimal; positive normal floats only)
//
// Prints `arguments=N mismatches=0` and returns 0, or prints the first mismatch with its bits and returns 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef GLIBC_LOGF_HEADER
#define GLIBC_LOGF_HEADER "glibc_logf.hpp"
#endif
#include GLIBC_LOGF_HEADER

int main(int argc, char** argv)
{
    uint32_t first = 0x33800000u, last = 0x40800000u;  // 2^-24, 4
    if (argc == 3)
    {
        first = (uint32_t)strtoul(argv[1], nullptr, 16);
        last = (uint32_t)strtoul(argv[2], nullptr, 16);
    }
    else if (argc != 1)
    {
        fprintf(stderr, "usage: glibc_logf_cases [FIRST_BITS LAST_BITS]\n");
        return 2;
    }
    if (first < 0x00800000u || last > 0x7f7fffffu || first > last)
    {
        fprintf(stderr, "the range must lie within the positive normal floats\n");
        return 2;
    }
    uint64_t n = 0;
    for (uint64_t b = first; b <= last; ++b)
    {
        const uint32_t bits = (uint32_t)b;
        float x;
        memcpy(&x, &bits, 4);
        // (volatile: the argument is opaque to the compiler, so the call below is the library's logf and not a folded constant)
        volatile float xv = x;
        const float want = logf(xv), got = mcmcpp::glibc_logf(x);
        uint32_t wb, gb;
        memcpy(&wb, &want, 4);
        memcpy(&gb, &got, 4);
        if (wb != gb)
        {
            printf("mismatch at x=%a (bits 0x%08x): logf 0x%08x (%a), glibc_logf 0x%08x (%a)\n", (double)x, bits, wb, (double)want, gb, (double)got);
            return 1;
        }
        ++n;
    }
    uint32_t one_bits;
    const float one = mcmcpp::glibc_logf(1.0f);
    memcpy(&one_bits, &one, 4);
    if (one_bits != 0)
    {
        printf("mismatch at x=1: glibc_logf 0x%08x, want +0\n", one_bits);
        return 1;
    }
    printf("arguments=%llu mismatches=0\n", (unsigned long long)n);
    return 0;
}
