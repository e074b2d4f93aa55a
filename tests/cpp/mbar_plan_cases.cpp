// mbar_plan_cases.cpp -- prints what mcmcpp_amd/csrc/mbar_plan.hpp plans for the multistate Bennett acceptance ratio
// (tests/test_mbar_plan.py).  Built with the host compiler against mbar_plan.hpp (and the headers it includes) alone: that it
// compiles without HIP is part of the test.  Doubles are printed as the 16 hex digits of their bits.
//   mbar_plan_cases plan K=.. N=..      Q, the joint and the rung tree, the buffers' doubles, fits
//   mbar_plan_cases index K=..          "k l index" per sum P_kl, k <= l, in the order of the groups
//   mbar_plan_cases sum file=..         sum_tree of the doubles of the file
//   mbar_plan_cases chol file=..        the file holds M, then A [M][M], then b [M]: "1" and x = solve(A, b), or "0"
//   mbar_plan_cases solve file=.. ess=..  the file holds K, N, then l [K][K N]; the ess file holds ess [K]: the solver with a host
//                                       pass: "passes converged failed", zeta, the joint sums, the rungs' sums, the series
//                                       w_r of every rung's own draws, then cov, log_ratio, mcse and the two totals
//   mbar_plan_cases limits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mbar_plan.hpp"

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
static void print_row(const double* v, size_t count)
{
    for (size_t i = 0; i < count; ++i) std::printf("%s%016llx", i ? " " : "", bits(v[i]));
    std::printf("\n");
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
        const int K = (int)get("K", 2);
        const long long N = get("N", 1);
        const MbarPlan p = mbar_plan(K, N);
        std::printf("Q=%d joint_terms=%lld joint_tiles=%lld joint_slices=%d rung_terms=%lld rung_tiles=%lld rung_slices=%d l=%zu series=%zu tile_sums=%zu slice_sums=%zu totals=%zu fits=%d\n",
                    p.Q, p.joint.terms, p.joint.tiles, p.joint.slices, p.rung.terms, p.rung.tiles, p.rung.slices, p.l_doubles, p.series_doubles, p.tile_sum_doubles,
                    p.slice_sum_doubles, p.total_doubles, (int)mbar_grid_fits(K, N));
        return 0;
    }
    if (what == "index")
    {
        const int K = (int)get("K", 2);
        for (int k = 0; k < K; ++k)
        {
            std::printf("group %d %d\n", k, mbar_group_quantities(K, k));
            for (int l = k; l < K; ++l) std::printf("%d %d %d\n", k, l, mbar_index_p(K, k, l));
        }
        return 0;
    }
    if (what == "sum")
    {
        const std::vector<double> v = read_doubles(a["file"]);
        std::printf("%016llx\n", bits(bridge_sum_tree(v.data(), (long long)v.size())));
        return 0;
    }
    if (what == "chol")
    {
        const std::vector<double> v = read_doubles(a["file"]);
        const int M = (int)v[0];
        std::vector<double> L((size_t)M * (size_t)M, 0.0), x((size_t)M);
        if (!mbar_factor(M, v.data() + 1, L.data()))
        {
            std::printf("0\n");
            return 0;
        }
        mbar_substitute(M, L.data(), v.data() + 1 + (size_t)M * (size_t)M, x.data());
        std::printf("1\n");
        print_row(x.data(), (size_t)M);
        return 0;
    }
    if (what == "solve")
    {
        const std::vector<double> v = read_doubles(a["file"]), ess = read_doubles(a["ess"]);
        const int K = (int)v[0], Q = mbar_quantities(K);
        const long long N = (long long)v[1];
        const size_t KN = (size_t)K * (size_t)N;
        const double* l = v.data() + 2;
        std::vector<double> series(KN);
        const auto eval = [&](const double* zeta, bool final, MbarSums* s) -> int {
            s->joint.assign((size_t)Q, 0.0);
            mbar_host_sums(K, l, KN, 0, (long long)KN, zeta, s->joint.data(), nullptr, 0);
            if (final)
            {
                s->rung.assign((size_t)K * (size_t)Q, 0.0);
                for (int r = 0; r < K; ++r) mbar_host_sums(K, l, KN, (long long)r * N, N, zeta, s->rung.data() + (size_t)r * (size_t)Q, series.data() + (size_t)r * (size_t)N, r);
            }
            return 0;
        };
        MbarRoot r;
        if (mbar_solve(K, N, eval, &r)) return 3;
        std::printf("%lld %d %d\n", r.passes, r.converged, (int)r.failed);
        print_row(r.zeta.data(), (size_t)K);
        if (r.failed) return 0;
        print_row(r.at.joint.data(), (size_t)Q);
        print_row(r.at.rung.data(), (size_t)K * (size_t)Q);
        print_row(series.data(), KN);
        std::vector<double> cov((size_t)K * (size_t)K), log_ratio((size_t)(K - 1)), mcse((size_t)(K - 1));
        double totals[2];
        mbar_covariance(K, N, r.L.data(), r.at.rung.data(), ess.data(), cov.data());
        mbar_figures(K, r.zeta.data(), cov.data(), log_ratio.data(), mcse.data(), &totals[0], &totals[1]);
        print_row(cov.data(), cov.size());
        print_row(log_ratio.data(), log_ratio.size());
        print_row(mcse.data(), mcse.size());
        print_row(totals, 2);
        return 0;
    }
    if (what == "limits")
    {
        std::printf("max_chains=%d batch=%d solver_passes=%d cap=%016llx tolerance=%016llx threads=%d tile=%d slice_tiles=%d\n", kMbarMaxChains, kMbarBatch, kMbarSolverPasses,
                    bits(kMbarStepCap), bits(kMbarTolerance), kBridgeThreads, kBridgeTile, kBridgeSliceTiles);
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
