// normal_score_cases.cpp -- mcmcpp_amd/csrc/normal_score.hpp compiled with the host compiler, for tests/test_normal_score.py:
//   normal_score_cases score|log|liblog|rank < doubles > doubles     (raw little-endian doubles on both sides)
// score: z = normal_score(p).  log: normal_score_log(x).  liblog: the host libm's log(x).  rank: triples (below, equal, S) as
// doubles -> normal_score_of_rank.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mcmcpp_amd/csrc/normal_score.hpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::vector<double> in;
    double buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(double), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
    std::vector<double> out;
    if (!strcmp(argv[1], "score"))
        for (double p : in) out.push_back(mcmcpp::normal_score(p));
    else if (!strcmp(argv[1], "log"))
        for (double x : in) out.push_back(mcmcpp::normal_score_log(x));
    else if (!strcmp(argv[1], "liblog"))
        for (double x : in) out.push_back(std::log(x));
    else if (!strcmp(argv[1], "rank"))
        for (size_t i = 0; i + 2 < in.size(); i += 3) out.push_back(mcmcpp::normal_score_of_rank((unsigned)in[i], (unsigned)in[i + 1], (unsigned)in[i + 2]));
    else
        return 2;
    return fwrite(out.data(), sizeof(double), out.size(), stdout) == out.size() ? 0 : 1;
}
