// exchange_plan_cases.cpp -- prints what mcmcpp_amd/csrc/exchange_plan.hpp gives (tests/test_exchange_kernels.py).
// Built with the host compiler against that header alone: that it compiles without HIP is part of the test.
//   exchange_plan_cases rows                     every D in 1..1024, both element sizes: "elem D vec pieces lpr rows_per_block"
//   exchange_plan_cases blocks cap=a,b,c         the same points times every cap: "elem D cap idx logp rows bytes grid_x"
//   exchange_plan_cases scatter_y cap=a,b,c      ranks 2..8: "ranks y", after checking that y is the same at every point
//   exchange_plan_cases pack walkers=N           1..N walkers (colours x slice): "walkers blocks"
//   exchange_plan_cases sync shard=N             1..N walkers per colour: "shard blocks"
//   exchange_plan_cases constants                the launch constants, "name=value" fields on one line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "exchange_plan.hpp"

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
    const size_t elems[2] = {8, 4};
    const int max_dims = 1024;

    if (what == "rows")
    {
        for (size_t e : elems)
            for (int D = 1; D <= max_dims; ++D)
            {
                const XRowPieces r = exchange_row_pieces(D, e);
                const int lpr = exchange_lanes_per_row(r.pieces);
                std::printf("%zu %d %d %d %d %d\n", e, D, r.vec ? 1 : 0, r.pieces, lpr, exchange_scatter_rows_per_block(lpr));
            }
        return 0;
    }
    if (what == "blocks")
    {
        for (size_t e : elems)
            for (int D = 1; D <= max_dims; ++D)
                for (long long cap : list_of(a["cap"]))
                    std::printf("%zu %d %lld %zu %zu %zu %zu %u\n", e, D, cap, xblock_idx_offset(), xblock_logp_offset((uint32_t)cap), xblock_rows_offset((uint32_t)cap, e),
                                xblock_bytes((uint32_t)cap, D, e), exchange_scatter_grid((uint32_t)cap, D, e, 2).x);
        return 0;
    }
    if (what == "scatter_y")
    {
        for (int ranks = 2; ranks <= 8; ++ranks)
        {
            const unsigned y = exchange_scatter_grid(1, 1, 8, ranks).y;
            for (size_t e : elems)
                for (int D = 1; D <= max_dims; ++D)
                    for (long long cap : list_of(a["cap"]))
                    {
                        const XScatterGrid g = exchange_scatter_grid((uint32_t)cap, D, e, ranks);
                        if (g.y != y || g.x != exchange_scatter_grid((uint32_t)cap, D, e, 2).x)
                        {
                            std::fprintf(stderr, "the scatter grid of elem %zu D %d cap %lld depends on the ranks in more than y\n", e, D, cap);
                            return 1;
                        }
                    }
            std::printf("%d %u\n", ranks, y);
        }
        return 0;
    }
    if (what == "pack")
    {
        for (int w = 1; w <= std::atoi(a["walkers"].c_str()); ++w) std::printf("%d %u\n", w, exchange_pack_blocks(w));
        return 0;
    }
    if (what == "sync")
    {
        for (int s = 1; s <= std::atoi(a["shard"].c_str()); ++s) std::printf("%d %u\n", s, exchange_sync_seen_blocks(s));
        return 0;
    }
    if (what == "constants")
    {
        std::printf("header=%zu walkers_per_wave=%d waves_per_block=%d pack_threads=%d scatter_threads=%d sync_threads=%d max_lpr=%d\n", kXBlockHeaderBytes,
                    kPackWalkersPerWave, kPackWavesPerBlock, kPackThreads, kScatterThreads, kSyncSeenThreads, kExchangeMaxLanesPerRow);
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
