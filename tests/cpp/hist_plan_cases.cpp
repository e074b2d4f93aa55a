// hist_plan_cases.cpp -- prints the launch plan of the histogram kernels (tests/test_hist_plan.py, tests/test_histograms.py).
// Built with the host compiler against mcmcpp_amd/csrc/hist_plan.hpp alone: that it compiles without HIP is part of the test.
//   hist_plan_cases plan n=.. P=.. bins=.. pairs=0|1 cus=.. lds=..       one plan: a line of key=value fields, then a line
//                                                                        "launches=t0:now:q0,..." of the pair launches
//   hist_plan_cases grid                                                 the same for the grid named in the test; the values
//                                                                        of n, P, bins and cus come on the command line as
//                                                                        n=a,b,c P=... bins=... cus=... lds=...
//   hist_plan_cases chunk chunk_bytes=.. step_bytes=.. W=..              steps per chunk
//   hist_plan_cases lds shared=..                                        the LDS limit for a device's sharedMemPerBlock
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "hist_plan.hpp"

using namespace mcmcpp;

static void print_plan(long long n, int P, int bins, int pairs, int cus, size_t lds)
{
    const HistPlan p = hist_plan((unsigned)n, P, bins, pairs != 0, cus, lds);
    std::printf("n=%lld P=%d bins=%d pairs=%d cus=%d lds=%zu idx_bytes=%d col=%zu bounds_blocks=%u bounds_per=%u bin_blocks=%u single_lds=%d single_slices=%u "
                "single_per=%u single_blocks=%u single_lds_bytes=%zu npairs=%lld pair_lds=%d tile=%d tiles=%lld last_count=%d pair_slices=%u pair_per=%u "
                "pair_blocks=%u pair_lds_bytes=%zu pair_launches=%lld\n",
                n, P, bins, pairs, cus, lds, p.idx_bytes, p.col, p.bounds_blocks, p.bounds_per, p.bin_blocks, p.single_lds, p.single_slices, p.single_per,
                p.single_blocks, p.single_lds_bytes, p.npairs, p.pair_lds, p.tile, p.tiles, p.last_count, p.pair_slices, p.pair_per, p.pair_blocks,
                p.pair_lds_bytes, p.pair_launches);
    std::printf("launches=");
    for (long long i = 0; i < p.pair_launches; ++i)
    {
        const HistPairLaunch l = p.pair_launch(i);
        std::printf("%s%lld:%lld:%lld", i ? "," : "", l.t0, l.now, l.q0);
    }
    std::printf("\n");
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
        print_plan(get("n", 0), (int)get("P", 1), (int)get("bins", 2), (int)get("pairs", 1), (int)get("cus", 256), (size_t)get("lds", 65536));
        return 0;
    }
    if (what == "grid")
    {
        for (long long n : list_of(a["n"]))
            for (long long P : list_of(a["P"]))
                for (long long bins : list_of(a["bins"]))
                    for (long long cus : list_of(a["cus"]))
                        for (int pairs = 0; pairs < 2; ++pairs) print_plan(n, (int)P, (int)bins, pairs, (int)cus, (size_t)get("lds", 65536));
        return 0;
    }
    if (what == "chunk")
    {
        std::printf("%lld\n", hist_steps_per_chunk((size_t)get("chunk_bytes", 0), (size_t)get("step_bytes", 1), (int)get("W", 1)));
        return 0;
    }
    if (what == "lds")
    {
        std::printf("%zu\n", hist_lds_limit((size_t)get("shared", 0)));
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
