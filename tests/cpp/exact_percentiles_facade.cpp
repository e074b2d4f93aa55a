// exact_percentiles_facade.cpp -- the facade's Analysis::ExactPercentiles (an extension: include/MCMCpp/Analysis/
// ExactPercentiles.h) on a chain the facade's own sampler produced, written like the analysis section of a reference-style
// program.  The kind of chain memory comes from the environment (MCMCPP_CHAIN_MEMORY=device / pinned / heap, and
// MCMCPP_DEVICE_ANALYSIS=0): tests/test_quantiles.py runs the program under each and checks that every run prints the same
// bytes, and the results against the restatement of the chain it wrote (tests/quantile_restatement.py).
//   usage: exact_percentiles_facade <out.bin>      (needs an MI355X)
// out.bin: int32 W, P, n_steps, slice, K, n_values; double chain[n][W][P]; double percentiles[K]; per parameter p and k < K:
//   getLowerValue, getHigherValue, getValueFromPercentile (double); double values[P][n_values]; per (p, k): getCountBelow,
//   getCountNotAbove (int64), getPercentileFromValue (double); getNumPoints (int64)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "Analysis/ExactPercentiles.h"
#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/StretchMove.h"

static FILE* g_out;
template <class V>
static void put(const V& v)
{
    std::fwrite(&v, sizeof(V), 1, g_out);
}

int main(int argc, char** argv)
{
    if (argc != 2) return 1;
    g_out = std::fopen(argv[1], "wb");
    if (!g_out) return 1;
    typedef MCMC::Device::IsoGaussian<double> Target;
    typedef MCMC::Mover::StretchMove<double, Target> Mover;
    const int W = 64, P = 4, steps = 200, slice = 3;
    Target target(P);
    Mover mover(P, 11, target);
    MCMC::EnsembleSampler<double, Mover> sampler(11, W, P, mover);
    std::vector<double> pos(static_cast<size_t>(W) * P), aux(W);
    unsigned long long s = 4242;
    for (size_t k = 0; k < pos.size(); ++k)
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        pos[k] = ((s >> 11) * (1.0 / 9007199254740992.0)) * 4.0 - 2.0;
    }
    for (int w = 0; w < W; ++w) aux[w] = target.calcLogPostProb(&pos[static_cast<size_t>(w) * P]);
    sampler.setInitialWalkerPos(pos.data(), aux.data());
    sampler.runMCMC(steps);

    const std::vector<double> percentiles = {0.0, 2.5, 16.0, 50.0, 84.0, 97.5, 100.0};
    const int K = static_cast<int>(percentiles.size());
    MCMC::Analysis::ExactPercentiles<double> ep(P, W);
    ep.processChainData(sampler.getStepIttBegin(), sampler.getStepIttEnd(), slice, percentiles);
    // the values asked about: the selected percentiles themselves, and one value below and one above every sample
    const int nv = K + 2;
    std::vector<double> values(static_cast<size_t>(P) * nv);
    for (int p = 0; p < P; ++p)
    {
        for (int k = 0; k < K; ++k) values[static_cast<size_t>(p) * nv + k] = ep.getLowerValue(p, k);
        values[static_cast<size_t>(p) * nv + K] = -1.0e300;
        values[static_cast<size_t>(p) * nv + K + 1] = 1.0e300;
    }
    MCMC::Analysis::ExactPercentiles<double> ranks(P, W);
    ranks.processValues(sampler.getStepIttBegin(), sampler.getStepIttEnd(), slice, values);

    int n = 0;
    for (auto it = sampler.getStepIttBegin(); it != sampler.getStepIttEnd(); ++it) ++n;
    const int32_t head[6] = {W, P, n, slice, K, nv};
    std::fwrite(head, sizeof(int32_t), 6, g_out);
    for (auto it = sampler.getStepIttBegin(); it != sampler.getStepIttEnd(); ++it) std::fwrite(*it, sizeof(double), static_cast<size_t>(W) * P, g_out);
    for (int k = 0; k < K; ++k) put(percentiles[k]);
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < K; ++k)
        {
            put(ep.getLowerValue(p, k));
            put(ep.getHigherValue(p, k));
            put(ep.getValueFromPercentile(p, k));
            std::printf("p%d %g%%: %.17g %.17g %.17g\n", p, percentiles[k], ep.getLowerValue(p, k), ep.getHigherValue(p, k), ep.getValueFromPercentile(p, k));
        }
    for (size_t k = 0; k < values.size(); ++k) put(values[k]);
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < nv; ++k)
        {
            put(static_cast<int64_t>(ranks.getCountBelow(p, k)));
            put(static_cast<int64_t>(ranks.getCountNotAbove(p, k)));
            put(ranks.getPercentileFromValue(p, k));
            std::printf("p%d value %.17g: %lld %lld %.17g\n", p, values[static_cast<size_t>(p) * nv + k], ranks.getCountBelow(p, k), ranks.getCountNotAbove(p, k),
                        ranks.getPercentileFromValue(p, k));
        }
    put(static_cast<int64_t>(ep.getNumPoints()));
    std::fclose(g_out);
    std::printf("exact_percentiles_facade OK\n");
    return 0;
}
