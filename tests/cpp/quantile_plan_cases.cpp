// quantile_plan_cases.cpp -- prints the launch plan of the order-statistics kernels (tests/test_quantile_plan.py,
// tests/test_quantiles.py).  Built with the host compiler against mcmcpp_amd/csrc/quantile_plan.hpp (and the hist_plan.hpp it
// includes) alone: that it compiles without HIP is part of the test.
//   quantile_plan_cases plan n=.. P=.. groups=.. key_bits=.. cus=.. lds=..   one selection pass and the rank pass: a line of
//                                                                            key=value fields
//   quantile_plan_cases grid n=a,b P=.. groups=.. key_bits=.. cus=.. lds=..  the same for every combination
//   quantile_plan_cases digits key_bits=.. [digit_bits=..]                   the digit schedule: "shift:bits" per pass
//   quantile_plan_cases chunk chunk_bytes=.. step_bytes=.. W=..              steps per chunk
//   quantile_plan_cases limits                                               the constants the entry points check against
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "quantile_plan.hpp"

using namespace mcmcpp;

static void print_plan(long long n, int P, int groups, int key_bits, int cus, size_t lds)
{
    const QuantPlan p = quantile_plan((unsigned)n, P, groups, key_bits, kQuantDigitBits, cus, lds);
    const QuantRankPlan r = quantile_rank_plan((unsigned)n, P, cus);
    std::printf("n=%lld P=%d groups=%d key_bits=%d cus=%d lds_limit=%zu digit_bits=%d cells=%d lds=%d tile=%d ptiles=%d slices=%u per=%u blocks=%u lds_bytes=%zu "
                "counters=%zu rank_tile=%d rank_ptiles=%d rank_slices=%u rank_per=%u rank_blocks=%u query_tile=%d\n",
                n, P, groups, key_bits, cus, lds, p.digit_bits, p.cells, p.lds, p.tile, p.ptiles, p.slices, p.per, p.blocks, p.lds_bytes, p.counters, r.tile, r.ptiles,
                r.slices, r.per, r.blocks, r.query_tile);
}

static std::vector<long long> list_of(const std::string& s)
{
    std::vector<long long> v;
    for (size_t at = 0; at < s.size();)
    {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        v.push_back(std::atoll(s.substr(at, end - at).c_str()));
        at = end + 1;
    }
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    std::map<std::string, std::string> a;
    for (int i = 2; i < argc; ++i)
    {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        a[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    auto get = [&](const char* key, long long fallback) { return a.count(key) ? std::atoll(a[key].c_str()) : fallback; };

    if (what == "plan")
    {
        print_plan(get("n", 1), (int)get("P", 1), (int)get("groups", 1), (int)get("key_bits", 64), (int)get("cus", 256), (size_t)get("lds", 65536));
        return 0;
    }
    if (what == "grid")
    {
        for (long long n : list_of(a["n"]))
            for (long long P : list_of(a["P"]))
                for (long long groups : list_of(a["groups"]))
                    for (long long key_bits : list_of(a["key_bits"]))
                        for (long long cus : list_of(a["cus"])) print_plan(n, (int)P, (int)groups, (int)key_bits, (int)cus, (size_t)get("lds", 65536));
        return 0;
    }
    if (what == "digits")
    {
        const int key_bits = (int)get("key_bits", 64), digit_bits = (int)get("digit_bits", kQuantDigitBits);
        for (int pass = 0; pass < quantile_passes(key_bits, digit_bits); ++pass)
        {
            const QuantDigit d = quantile_digit(key_bits, pass, digit_bits);
            std::printf("%s%d:%d", pass ? " " : "", d.shift, d.bits);
        }
        std::printf("\n");
        return 0;
    }
    if (what == "chunk")
    {
        std::printf("%lld\n", quantile_steps_per_chunk((size_t)get("chunk_bytes", 0), (size_t)get("step_bytes", 1), (int)get("W", 1)));
        return 0;
    }
    if (what == "limits")
    {
        std::printf("threads=%d digit_bits=%d max_ranks=%d max_params=%d min_tile=%d query_tile=%d grid_x=%lld grid_y=%lld grid_z=%lld\n", kQuantPlanThreads,
                    kQuantDigitBits, kQuantMaxRanks, kQuantMaxParams, kQuantMinTile, kQuantQueryTile, kQuantGridXMax, kQuantGridYMax, kQuantGridZMax);
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
