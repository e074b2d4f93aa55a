// rank_plan_cases.cpp -- mcmcpp_amd/csrc/rank_plan.hpp compiled with the host compiler alone, for tests/test_rank_plan.py:
//   rank_plan_cases plan S=.. P=.. bits=.. work_mb=..     one line of key=value: the sort of a tile
//   rank_plan_cases spans S=..                            "first count" of every block of a pass
//   rank_plan_cases digits bits=..                        the shift of every pass
//   rank_plan_cases quantile S=.. q=..                    h (as bits), lo, hi
//   rank_plan_cases grids S=.. P=..                       blocks of the kernels with a thread per (draw, parameter); 1 if every grid fits
//   rank_plan_cases env                                   the work bytes the environment gives
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "rank_plan.hpp"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::map<std::string, std::string> a;
    for (int i = 2; i < argc; ++i)
    {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        a[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    const auto num = [&](const char* k) { return a.count(k) ? atoll(a[k].c_str()) : 0LL; };
    const std::string what = argv[1];
    if (what == "plan")
    {
        const long long S = num("S");
        const int P = (int)num("P"), bits = (int)num("bits");
        const size_t work = (size_t)num("work_mb") << 20;
        const int tile = mcmcpp::rank_param_tile(S, P, bits, work);
        const mcmcpp::RankLayout l = mcmcpp::rank_layout(S, bits, tile), one = mcmcpp::rank_layout(S, bits, 1);
        printf("tile=%d tiles=%d bytes=%zu one=%zu keys_a=%zu keys_b=%zu idx_a=%zu idx_b=%zu table=%zu totals=%zu blocks=%lld draw_blocks=%lld items=%lld passes=%d "
               "threads=%d rounds=%d digits=%d xmax=%lld ymax=%lld maxdraws=%lld default_mb=%zu align=%zu\n",
               tile, mcmcpp::rank_tiles(P, tile), l.bytes, one.bytes, l.keys_a, l.keys_b, l.idx_a, l.idx_b, l.table, l.totals, mcmcpp::rank_blocks(S), mcmcpp::rank_draw_blocks(S),
               mcmcpp::rank_items_per_block(), mcmcpp::rank_passes(bits), mcmcpp::kRankThreads, mcmcpp::kRankItemsPerThread, mcmcpp::kRankDigits, mcmcpp::kRankGridXMax,
               mcmcpp::kRankGridYMax, mcmcpp::kRankMaxDraws, mcmcpp::kRankDefaultWorkMb, mcmcpp::kRankAlign);
        return 0;
    }
    if (what == "spans")
    {
        const long long S = num("S");
        for (long long b = 0; b < mcmcpp::rank_blocks(S); ++b)
        {
            long long first, count;
            mcmcpp::rank_block_span(S, b, &first, &count);
            printf("%lld %lld\n", first, count);
        }
        return 0;
    }
    if (what == "digits")
    {
        for (int pass = 0; pass < mcmcpp::rank_passes((int)num("bits")); ++pass) printf("%d\n", mcmcpp::rank_digit_shift(pass));
        return 0;
    }
    if (what == "quantile")
    {
        const mcmcpp::RankQuantile r = mcmcpp::rank_quantile(atof(a["q"].c_str()), num("S"));
        uint64_t bits;
        memcpy(&bits, &r.h, 8);
        printf("%" PRIu64 " %lld %lld\n", bits, r.lo, r.hi);
        return 0;
    }
    if (what == "grids")
    {
        printf("%lld %d\n", mcmcpp::rank_element_blocks(num("S"), (int)num("P")), mcmcpp::rank_grids_fit(num("S"), (int)num("P")) ? 1 : 0);
        return 0;
    }
    if (what == "env")
    {
        printf("%zu %d %d\n", mcmcpp::rank_work_bytes_from_env(), mcmcpp::rank_key_bits(true, false), mcmcpp::rank_key_bits(true, true) + mcmcpp::rank_key_bits(false, false));
        return 0;
    }
    return 2;
}
