// posterior_summary_facade.cpp -- the facade's Analysis::PosteriorSummary (an extension:
// include/MCMCpp/Analysis/PosteriorSummary.h) on the chains of three of the facade's own samplers with different seeds.  The
// kind of chain memory comes from the environment (MCMCPP_CHAIN_MEMORY=device / heap, and MCMCPP_DEVICE_ANALYSIS=0):
// tests/test_summary.py runs the program under each and checks that every run writes the same bytes, and the results against the
// restatement on the chains it wrote (tests/summary_restatement.py).
//   usage: posterior_summary_facade <out.bin>      (needs an MI355X)
// out.bin: int32 K, W, P, n_steps, slice, Q; double probs[Q], hdi_prob; double chains[K][n][W][P]; double mean[P], sd[P],
//   mcse_mean[P], ess_mean[P], ess_sd[P], mcse_sd[P], quantile[P][Q], ess_quantile[P][Q], mcse_quantile[P][Q]; int64
//   rank_lower[P][Q], rank_upper[P][Q]; double hdi_lower[P], hdi_upper[P]; int64 sequence_length, num_sequences
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <memory>
#include <vector>

#include "Analysis/PosteriorSummary.h"
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
    typedef MCMC::EnsembleSampler<double, Mover> Sampler;
    const int K = 3, W = 64, P = 4, steps = 900, slice = 2;
    Target target(P);
    std::vector<std::unique_ptr<Mover> > movers;
    std::vector<std::unique_ptr<Sampler> > samplers;
    for (int k = 0; k < K; ++k)
    {
        movers.push_back(std::unique_ptr<Mover>(new Mover(P, 11 + k, target)));
        samplers.push_back(std::unique_ptr<Sampler>(new Sampler(11 + k, W, P, *movers[k])));
        std::vector<double> pos(static_cast<size_t>(W) * P), aux(W);
        unsigned long long s = 4242 + 1000 * k;
        for (size_t i = 0; i < pos.size(); ++i)
        {
            s = s * 6364136223846793005ULL + 1442695040888963407ULL;
            pos[i] = ((s >> 11) * (1.0 / 9007199254740992.0)) * 4.0 - 2.0;
        }
        for (int w = 0; w < W; ++w) aux[w] = target.calcLogPostProb(&pos[static_cast<size_t>(w) * P]);
        samplers[k]->setInitialWalkerPos(pos.data(), aux.data());
        samplers[k]->runMCMC(steps);
    }

    const std::vector<double> probs = {0.1, 0.5};
    const double hdiProb = 0.8;
    MCMC::Analysis::PosteriorSummary<double> ps(P, W);
    for (int k = 0; k < K; ++k) ps.addChain(samplers[k]->getStepIttBegin(), samplers[k]->getStepIttEnd(), slice);
    ps.calculate(probs, hdiProb);
    const int Q = ps.getNumQuantiles();

    int n = 0;
    for (auto it = samplers[0]->getStepIttBegin(); it != samplers[0]->getStepIttEnd(); ++it) ++n;
    const int32_t head[6] = {K, W, P, n, slice, Q};
    std::fwrite(head, sizeof(int32_t), 6, g_out);
    for (int i = 0; i < Q; ++i) put(ps.getQuantileProb(i));
    put(ps.getHdiProb());
    for (int k = 0; k < K; ++k)
        for (auto it = samplers[k]->getStepIttBegin(); it != samplers[k]->getStepIttEnd(); ++it) std::fwrite(*it, sizeof(double), static_cast<size_t>(W) * P, g_out);
    for (int p = 0; p < P; ++p) put(ps.getMean(p));
    for (int p = 0; p < P; ++p) put(ps.getSd(p));
    for (int p = 0; p < P; ++p) put(ps.getMcseMean(p));
    for (int p = 0; p < P; ++p) put(ps.getEssMean(p));
    for (int p = 0; p < P; ++p) put(ps.getEssSd(p));
    for (int p = 0; p < P; ++p) put(ps.getMcseSd(p));
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < Q; ++i) put(ps.getQuantile(p, i));
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < Q; ++i) put(ps.getEssQuantile(p, i));
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < Q; ++i) put(ps.getMcseQuantile(p, i));
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < Q; ++i) put(static_cast<int64_t>(ps.getMcseRankLower(p, i)));
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < Q; ++i) put(static_cast<int64_t>(ps.getMcseRankUpper(p, i)));
    for (int p = 0; p < P; ++p) put(ps.getHdiLower(p));
    for (int p = 0; p < P; ++p) put(ps.getHdiUpper(p));
    put(static_cast<int64_t>(ps.getSequenceLength()));
    put(static_cast<int64_t>(ps.getNumSequences()));
    std::fclose(g_out);
    ps.writeTable(std::cout);
    std::cout << "posterior_summary_facade OK" << std::endl;
    return 0;
}
