// bridge_plan_cases.cpp -- prints what mcmcpp_amd/csrc/bridge_plan.hpp plans for the bridge estimate
// (tests/test_bridge_plan.py).  Built with the host compiler against bridge_plan.hpp (and the headers it includes) alone: that
// it compiles without HIP is part of the test.  Doubles are printed as the 16 hex digits of their bits.
//   bridge_plan_cases plan N=..        tiles, slices, grid, doubles of tile and slice sums, fits; then "t first count" per slice
//   bridge_plan_cases buffers K=..     the buffers in flight, then "d p buffer" per pair and direction
//   bridge_plan_cases sum file=..      sum_tree of the doubles of the file
//   bridge_plan_cases sigma file=..    sigma of every double of the file, one per line
//   bridge_plan_cases solve file=..    the file holds u0 then u1 (N each): the solver with a host pass; c*, passes, converged, then
//                                      S_0 S_1 Q_0 Q_1 H_0 H_1 of the final pass
//   bridge_plan_cases limits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "bridge_plan.hpp"

using namespace mcmcpp;

static std::vector<double> read_doubles(const std::string& path)
{
    std::vector<double> v;
    if (std::FILE* f = std::fopen(path.c_str(), "rb"))
    {
        double buf[1024];
        size_t got;
        while ((got = std::fread(buf, 8, 1024, f)) > 0) v.insert(v.end(), buf, buf + got);
        std::fclose(f);
    }
    return v;
}
static unsigned long long bits(double x)
{
    unsigned long long b;
    std::memcpy(&b, &x, 8);
    return b;
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
        const long long N = get("N", 1);
        const BridgePlan p = bridge_plan(N);
        std::printf("tiles=%lld slices=%d grid_x=%u grid_y=%u tile_sums=%zu slice_sums=%zu fits=%d\n", p.tiles, p.slices, p.grid_x, p.grid_y, p.tile_sum_doubles,
                    p.slice_sum_doubles, (int)bridge_grid_fits(N));
        for (int t = 0; t < p.slices; ++t)
        {
            long long first, count;
            bridge_slice_span(p.tiles, t, &first, &count);
            std::printf("%d %lld %lld\n", t, first, count);
        }
        return 0;
    }
    if (what == "buffers")
    {
        const int K = (int)get("K", 2);
        std::printf("%d\n", bridge_buffers(K));
        for (int p = 0; p < evidence_pairs(K); ++p)
            for (int d = 0; d < 2; ++d) std::printf("%d %d %d\n", d, p, bridge_buffer_of(d, p));
        return 0;
    }
    if (what == "sum")
    {
        const std::vector<double> v = read_doubles(a["file"]);
        std::printf("%016llx\n", bits(bridge_sum_tree(v.data(), (long long)v.size())));
        return 0;
    }
    if (what == "sigma")
    {
        for (double x : read_doubles(a["file"])) std::printf("%016llx\n", bits(bridge_sigma(x)));
        return 0;
    }
    if (what == "solve")
    {
        const std::vector<double> v = read_doubles(a["file"]);
        const long long N = (long long)v.size() / 2;
        std::vector<double> h(3 * (size_t)N);
        const auto eval = [&](double c, bool final, BridgeSums* s) -> int {
            for (int d = 0; d < 2; ++d)
            {
                for (long long i = 0; i < N; ++i)
                {
                    const double u = v[(size_t)(d * N + i)], x = bridge_sigma(d ? u + c : u - c);
                    h[(size_t)i] = x, h[(size_t)(N + i)] = x * (1.0 - x), h[(size_t)(2 * N + i)] = x * x;
                }
                s->S[d] = bridge_sum_tree(h.data(), N), s->Q[d] = bridge_sum_tree(h.data() + N, N);
                s->H[d] = final ? bridge_sum_tree(h.data() + 2 * N, N) : 0.0;
            }
            return 0;
        };
        BridgeRoot r;
        if (bridge_solve(eval, &r)) return 3;
        std::printf("%016llx %lld %d\n", bits(r.c), r.passes, r.converged);
        std::printf("%016llx %016llx %016llx %016llx %016llx %016llx\n", bits(r.at.S[0]), bits(r.at.S[1]), bits(r.at.Q[0]), bits(r.at.Q[1]), bits(r.at.H[0]), bits(r.at.H[1]));
        return 0;
    }
    if (what == "limits")
    {
        std::printf("threads=%d tile=%d slice_tiles=%d bracket=%d newton=%d tolerance=%016llx\n", kBridgeThreads, kBridgeTile, kBridgeSliceTiles, kBridgeBracketPasses,
                    kBridgeNewtonPasses, bits(kBridgeTolerance));
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
