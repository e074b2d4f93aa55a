// evidence_exp_cases.cpp -- mcmcpp_amd/csrc/evidence_exp.hpp compiled with the host compiler, for tests/test_evidence_exp.py:
//   evidence_exp_cases exp|libexp < doubles > doubles     (raw little-endian doubles on both sides)
// exp: evidence_exp(x).  libexp: the host libm's exp(x).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mcmcpp_amd/csrc/evidence_exp.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::vector<double> in;
    double buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(double), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
    std::vector<double> out;
    if (!strcmp(argv[1], "exp"))
        for (double x : in) out.push_back(mcmcpp::evidence_exp(x));
    else if (!strcmp(argv[1], "libexp"))
        for (double x : in) out.push_back(std::exp(x));
    else
        return 2;
    return fwrite(out.data(), sizeof(double), out.size(), stdout) == out.size() ? 0 : 1;
}
