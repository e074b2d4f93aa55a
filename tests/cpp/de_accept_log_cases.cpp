// de_accept_log_cases.cpp -- the accept logarithm of a differential-evolution record on the host, for tests/test_de_planner.py:
// neg_exp = log(1 - canonical(raw)) with the host build of the very headers the device compiles -- fast_log.hpp in fp64,
// glibc_logf.hpp in fp32 -- both pinned to the device's bits by tests/test_accept_logs.py and tests/test_glibc_logf.py.
// Built with the host compiler alone, -ffp-contract=off like the library.
//   de_accept_log_cases IN OUT64 OUT32    IN: raw 64-bit draws; OUT64: the doubles; OUT32: the floats
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "canonical.hpp"
#include "fast_log.hpp"
#include "glibc_logf.hpp"

int main(int argc, char** argv)
{
    if (argc != 4)
    {
        fprintf(stderr, "usage: de_accept_log_cases IN OUT64 OUT32\n");
        return 1;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* f64 = fopen(argv[2], "wb");
    FILE* f32 = fopen(argv[3], "wb");
    if (!fi || !f64 || !f32) return 2;
    std::vector<double> d;
    std::vector<float> f;
    uint64_t r;
    while (fread(&r, 8, 1, fi) == 1)
    {
        d.push_back(mcmcpp::fast_log(1.0 - mcmcpp::canonical(r, double())));
        f.push_back(mcmcpp::glibc_logf(1.0f - mcmcpp::canonical(r, float())));
    }
    if (fwrite(d.data(), 8, d.size(), f64) != d.size() || fwrite(f.data(), 4, f.size(), f32) != f.size()) return 2;
    return fclose(fi) | fclose(f64) | fclose(f32) ? 2 : 0;
}
