// ess_plan_cases.cpp -- prints what mcmcpp_amd/csrc/ess_plan.hpp plans for the effective-sample-size kernels and what its host
// part computes (tests/test_ess_plan.py, tests/test_ess.py).  Built with the host compiler against ess_plan.hpp (and the
// rhat_plan.hpp and step_chunks.hpp it includes) alone: that it compiles without HIP is part of the test.  Doubles travel as
// hexadecimal floats.
//   ess_plan_cases window L=.. max_lag=.. n_functions=..       cap, kmax, function lags, lags needed, blocks
//   ess_plan_cases walk L=.. t0=a,b,..                         "t0 lead_end full_end" per line: the steps a lag block walks
//   ess_plan_cases rounds L=.. max_lag=.. n_functions=.. series=.. E=.. zs=.. decided=..   (knobs from the environment)
//                                                              "first lags blocks gx gy gz" per round, as the host loop takes
//                                                              them when every window is decided once `decided` lags are known
//   ess_plan_cases capacity work_bytes=.. series=..            lags of a round that fit the work buffer
//   ess_plan_cases window_walk kmax=.. have=.. rho=a,b,..      "state pairs total" by the window rule
//   ess_plan_cases tau total=.. N=..                           tau and ess
//   ess_plan_cases rho S=.. M=.. L=.. within=.. between=.. t=..   gamma, varplus and rho
//   ess_plan_cases limits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ess_plan.hpp"

using namespace mcmcpp;

static std::vector<std::string> split_list(const std::string& s)
{
    std::vector<std::string> v;
    for (size_t at = 0; at < s.size();)
    {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        v.push_back(s.substr(at, end - at));
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
    auto real = [&](const char* key) { return std::strtod(a[key].c_str(), nullptr); };

    if (what == "window")
    {
        const long long cap = ess_cap(get("L", 2), get("max_lag", 0)), nf = get("n_functions", 0);
        std::printf("cap=%lld kmax=%lld function_lags=%lld needed=%lld blocks=%lld\n", cap, ess_kmax(cap), ess_function_lags(nf, cap), ess_lags_needed(cap, nf),
                    ess_blocks(ess_lags_needed(cap, nf)));
        return 0;
    }
    if (what == "walk")
    {
        for (const std::string& t : split_list(a["t0"]))
        {
            const EssWalk w = ess_block_walk(get("L", 2), std::atoll(t.c_str()));
            std::printf("%s %lld %lld\n", t.c_str(), w.lead_end, w.full_end);
        }
        return 0;
    }
    if (what == "rounds")
    {
        const long long L = get("L", 2), nf = get("n_functions", 0), series = get("series", 1), E = get("E", 1), decided = get("decided", 0);
        const long long cap = ess_cap(L, get("max_lag", 0)), F = ess_function_lags(nf, cap);
        const EssKnobs knobs = ess_knobs_from_env();
        long long done = 0, previous = 0;
        for (bool more = true; more;)
        {
            const long long lags = ess_round_lags(done, previous, knobs, series, cap, nf);
            if (lags < kEssLagBlock) return 3;
            const EssGrid g = ess_lag_grid(E, lags / kEssLagBlock, (int)get("zs", 1));
            std::printf("%lld %lld %lld %u %u %u\n", done, lags, lags / kEssLagBlock, g.x, g.y, g.z);
            done += lags;
            previous = lags;
            more = done < F || (done < decided && done < ess_blocks(ess_lags_needed(cap, nf)) * kEssLagBlock);  // (a window is decided at its cap)
        }
        return 0;
    }
    if (what == "capacity")
    {
        std::printf("%lld\n", ess_round_capacity((size_t)get("work_bytes", 0), get("series", 1)));
        return 0;
    }
    if (what == "window_walk")
    {
        std::vector<double> rho;
        for (const std::string& t : split_list(a["rho"])) rho.push_back(std::strtod(t.c_str(), nullptr));
        const EssWindow w = ess_walk_window([&](long long t) { return rho[(size_t)t]; }, get("have", (long long)rho.size()), get("kmax", 0));
        std::printf("%d %lld %a\n", w.state, w.pairs, w.total);
        return 0;
    }
    if (what == "tau")
    {
        const double tau = ess_tau(real("total"), real("N"));
        std::printf("%a %a\n", tau, real("N") / tau);
        return 0;
    }
    if (what == "rho")
    {
        const double gamma = ess_gamma(real("S"), real("M"), real("L")), varplus = ess_varplus(real("within"), real("between"), real("L"));
        std::printf("%a %a %a\n", gamma, varplus, ess_rho(get("t", 1), gamma, real("within"), varplus));
        return 0;
    }
    if (what == "limits")
    {
        std::printf("lag_block=%d rows_in_flight=%d vector=%d wave=%d blocks_per_group=%d threads=%d first_lags=%lld work_mb=%zu max_round_blocks=%lld grid_y=%lld\n",
                    kEssLagBlock, kEssRowsInFlight, kEssVector, kEssWave, kEssBlocksPerGroup, kEssThreads, kEssDefaultFirstLags, kEssDefaultWorkMb, kEssMaxRoundBlocks,
                    kRhatGridYMax);
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
