// Prints the compaction plan of mcmcpp_amd/csrc/chain_compact_plan.hpp for tests/test_device_facade.py.  Compiled with the host
// compiler against that header alone: that it compiles without a HIP include path is an assertion.
//
//   chain_compact_plan_cases <max_n> <max_interval>
// one line per (n, burn <= n, interval): "n burn interval kept | first:count first:count ..."
#include <cstdio>
#include <cstdlib>

#include "chain_compact_plan.hpp"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const long long maxN = std::atoll(argv[1]), maxInterval = std::atoll(argv[2]);
    for (long long n = 0; n <= maxN; ++n)
        for (long long burn = 0; burn <= n; ++burn)
            for (long long interval = 1; interval <= maxInterval; ++interval)
            {
                const long long kept = mcmcpp::chain_compact_kept(n, burn, interval);
                std::printf("%lld %lld %lld %lld |", n, burn, interval, kept);
                mcmcpp::ChainCompactWave w;
                for (std::int64_t done = 0; mcmcpp::chain_compact_wave(done, kept, burn, interval, &w); done = w.first + w.count)
                    std::printf(" %lld:%lld", static_cast<long long>(w.first), static_cast<long long>(w.count));
                std::printf("\n");
            }
    return 0;
}
