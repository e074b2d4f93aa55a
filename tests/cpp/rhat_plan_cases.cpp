// rhat_plan_cases.cpp -- prints what mcmcpp_amd/csrc/rhat_plan.hpp plans for the Gelman-Rubin kernels (tests/test_rhat_plan.py,
// tests/test_rhat.py).  Built with the host compiler against rhat_plan.hpp (and the step_chunks.hpp it includes) alone: that
// it compiles without HIP is part of the test.
//   rhat_plan_cases slices N=a,b,..                              "N slice_len slices" per line
//   rhat_plan_cases shape K=.. n=.. W=.. split=..                H, L, M and the first step of each half
//   rhat_plan_cases plan E=.. elem_bytes=.. base=.. L=.. zs=.. cus=..   the series kernel's launch: a line of key=value fields
//   rhat_plan_cases grid E=a,b L=.. zs=.. cus=.. elem_bytes=.. base=..  the same for every combination
//   rhat_plan_cases walk n=.. split=.. per=.. own=..            every (half, chunk, block y, slice) a launch sequence walks:
//                                                                "h g0 g1 y t s f fresh closes" per line (chunks by
//                                                                for_each_step_chunk, as the host code takes them)
//   rhat_plan_cases sum N=.. P=.. G=..                           the combine's launch
//   rhat_plan_cases chunk chunk_bytes=.. step_bytes=..           steps per chunk
//   rhat_plan_cases limits                                       the constants the entry points check against
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "rhat_plan.hpp"

using namespace mcmcpp;

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

static void print_plan(long long E, int elem_bytes, long long base, long long L, int zs, int cus)
{
    const int vec = rhat_vector_width((size_t)elem_bytes, E, (uintptr_t)base);
    const RhatSeriesPlan p = rhat_series_plan(E, vec, L, zs, cus);
    std::printf("E=%lld elem_bytes=%d base=%lld L=%lld zs=%d cus=%d vec=%d lanes=%lld waves=%lld etiles=%u own=%d slices=%d slots=%d slen=%lld slice_blocks=%u grid_z=%u\n", E,
                elem_bytes, base, L, zs, cus, p.vec, p.lanes, p.waves, p.etiles, p.own, p.slices, p.slots, p.slen, p.slice_blocks, p.zs);
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

    if (what == "slices")
    {
        for (long long N : list_of(a["N"])) std::printf("%lld %lld %d\n", N, rhat_slice_len(N), rhat_slices(N));
        return 0;
    }
    if (what == "shape")
    {
        const long long n = get("n", 4);
        const RhatShape s = rhat_shape((int)get("K", 1), n, (int)get("W", 1), (int)get("split", 1));
        std::printf("H=%d L=%lld M=%lld begin0=%lld begin1=%lld last=%lld\n", s.H, s.L, s.M, rhat_half_begin(n, s.L, 0), rhat_half_begin(n, s.L, s.H - 1),
                    rhat_sequence((int)get("K", 1) - 1, s.H - 1, get("W", 1) - 1, s.H, get("W", 1)));
        return 0;
    }
    if (what == "plan")
    {
        print_plan(get("E", 1), (int)get("elem_bytes", 8), get("base", 0), get("L", 2), (int)get("zs", 1), (int)get("cus", 256));
        return 0;
    }
    if (what == "grid")
    {
        for (long long E : list_of(a["E"]))
            for (long long L : list_of(a["L"]))
                for (long long zs : list_of(a["zs"]))
                    for (long long cus : list_of(a["cus"]))
                        for (long long eb : list_of(a["elem_bytes"]))
                            for (long long base : list_of(a["base"])) print_plan(E, (int)eb, base, L, (int)zs, (int)cus);
        return 0;
    }
    if (what == "walk")
    {
        const long long n = get("n", 4), per = get("per", n);
        const int own = (int)get("own", 1);
        const RhatShape s = rhat_shape(1, n, 1, (int)get("split", 1));
        const long long slen = rhat_slice_len(s.L);
        const int slices = rhat_slices(s.L);
        return for_each_step_chunk(n, per, [&](long long g0, long long now) -> int {
            for (int h = 0; h < s.H; ++h)
                for (int y = 0; y < (own ? 1 : slices); ++y)
                {
                    int t0, t1;
                    rhat_block_slices(own, slices, y, &t0, &t1);
                    for (int t = t0; t < t1; ++t)
                    {
                        const RhatWalk w = rhat_slice_walk(rhat_half_begin(n, s.L, h), s.L, slen, t, g0, g0 + now);
                        if (w.s < w.f) std::printf("%d %lld %lld %d %d %lld %lld %d %d\n", h, g0, g0 + now, y, t, w.s, w.f, w.fresh, w.closes);
                    }
                }
            return 0;
        });
    }
    if (what == "sum")
    {
        const RhatSumPlan p = rhat_sum_plan(get("N", 2), (int)get("P", 1), (int)get("G", 1));
        std::printf("slen=%lld slices=%d blocks=%u segments=%u\n", p.slen, p.slices, p.blocks, p.segments);
        return 0;
    }
    if (what == "chunk")
    {
        std::printf("%lld\n", rhat_steps_per_chunk((size_t)get("chunk_bytes", 0), (size_t)get("step_bytes", 1)));
        return 0;
    }
    if (what == "limits")
    {
        std::printf("threads=%d rows_in_flight=%d max_chains=%d max_params=%d min_slice=%lld max_slices=%d own_waves_per_cu=%d vector_bytes=%d grid_x=%lld "
                    "grid_y=%lld grid_z=%lld\n",
                    kRhatPlanThreads, kRhatRowsInFlight, kRhatMaxChains, kRhatMaxParams, kRhatMinSlice, kRhatMaxSlices, kRhatOwnWavesPerCu, kRhatVectorBytes,
                    kRhatGridXMax, kRhatGridYMax, kRhatGridZMax);
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
