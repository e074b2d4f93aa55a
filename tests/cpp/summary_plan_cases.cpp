// summary_plan_cases.cpp -- mcmcpp_amd/csrc/summary_plan.hpp and beta_quantile.hpp compiled with the host compiler alone, for
// tests/test_summary_plan.py (which also builds this file with the address and undefined-behaviour sanitizers and runs it):
//   summary_plan_cases limits                              the constants, one line of key=value
//   summary_plan_cases hdi windows=..                      blocks, then a check of every span: "ok <blocks> <covered>" or the
//                                                          first block whose span does not follow its predecessor's
//   summary_plan_cases spans windows=..                    "first count" of every block of the reduction
//   summary_plan_cases check S=.. hdi=.. probs=a,b,..      the refusal of the probabilities, then of hdi_prob ("-" = none), and m
//   summary_plan_cases ranks ess=.. prob=.. S=..           rank_lower rank_upper
//   summary_plan_cases pooled L=.. M=.. within=.. between=.. over=..      the pooled variance, as bits
//   summary_plan_cases beta p=.. a=.. b=..                 beta_quantile, %.17g
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "summary_plan.hpp"

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
    const auto real = [&](const char* k) { return a.count(k) ? strtod(a[k].c_str(), nullptr) : 0.0; };
    const std::string what = argv[1];
    if (what == "limits")
    {
        printf("max_probs=%d threads=%d span=%lld xmax=%lld ymax=%lld cf_cap=%d newton_cap=%d lower=%.17g upper=%.17g\n", mcmcpp::kSummaryMaxProbs, mcmcpp::kSummaryThreads,
               mcmcpp::kSummaryHdiSpan, mcmcpp::kRankGridXMax, mcmcpp::kRankGridYMax, mcmcpp::kBetaCfCap, mcmcpp::kBetaNewtonCap, mcmcpp::kSummaryLowerTail,
               mcmcpp::kSummaryUpperTail);
        return 0;
    }
    if (what == "hdi" || what == "spans")
    {
        const long long windows = num("windows"), blocks = mcmcpp::summary_hdi_blocks(windows);
        long long next = 0;
        for (long long b = 0; b < blocks; ++b)
        {
            long long first, count;
            mcmcpp::summary_hdi_block_span(windows, b, &first, &count);
            if (what == "spans") printf("%lld %lld\n", first, count);
            if (first != next || count < 1 || count > mcmcpp::kSummaryHdiSpan)
            {
                printf("bad %lld %lld %lld\n", b, first, count);
                return 1;
            }
            next = first + count;
        }
        long long first, count;  // a block past the last takes nothing
        mcmcpp::summary_hdi_block_span(windows, blocks, &first, &count);
        if (what == "hdi") printf("ok %lld %lld %lld %d\n", blocks, next, count, mcmcpp::summary_grids_fit(windows, (int)num("tile")) ? 1 : 0);
        return 0;
    }
    if (what == "check")
    {
        std::vector<double> probs;
        const std::string list = a["probs"];
        for (size_t at = 0; at < list.size();)
        {
            const size_t comma = list.find(',', at);
            probs.push_back(strtod(list.substr(at, comma == std::string::npos ? std::string::npos : comma - at).c_str(), nullptr));
            if (comma == std::string::npos) break;
            at = comma + 1;
        }
        const int n = a.count("n_probs") ? (int)num("n_probs") : (int)probs.size();
        const std::string p = mcmcpp::summary_check_probs(a.count("null") ? nullptr : probs.data(), n);
        const std::string h = mcmcpp::summary_check_hdi(real("hdi"), num("S"));
        printf("%s\n%s\n%lld\n", p.empty() ? "-" : p.c_str(), h.empty() ? "-" : h.c_str(), mcmcpp::summary_hdi_m(real("hdi"), num("S")));
        return 0;
    }
    if (what == "ranks")
    {
        const mcmcpp::SummaryMcseRanks r = mcmcpp::summary_mcse_ranks(real("ess"), real("prob"), num("S"));
        printf("%lld %lld\n", r.lower, r.upper);
        return 0;
    }
    if (what == "pooled")
    {
        const double v = mcmcpp::summary_pooled(num("L"), num("M"), real("within"), real("between"), num("over"));
        uint64_t bits;
        memcpy(&bits, &v, 8);
        printf("%" PRIu64 "\n", bits);
        return 0;
    }
    if (what == "beta")
    {
        printf("%.17g\n", mcmcpp::beta_quantile(real("p"), real("a"), real("b")));
        return 0;
    }
    return 2;
}
