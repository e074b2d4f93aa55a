// effective_sample_size_facade.cpp -- the facade's Analysis::EffectiveSampleSize (an extension:
// include/MCMCpp/Analysis/EffectiveSampleSize.h) on the chains of three of the facade's own samplers with different seeds,
// written like the analysis section of a reference-style program.  The kind of chain memory comes from the environment
// (MCMCPP_CHAIN_MEMORY=device / pinned / heap, and MCMCPP_DEVICE_ANALYSIS=0): tests/test_ess.py runs the program under each and
// checks that every run writes the same bytes, and the results against the restatement of the chains it wrote
// (tests/ess_restatement.py).
//   usage: effective_sample_size_facade <out.bin>      (needs an MI355X)
// out.bin: int32 K, W, P, n_steps, slice, split; double chains[K][n][W][P]; double ess[P], tau[P]; int64 lags_used[P], closed[P];
//   double rhat[P], mean[P], within[P], between[P]; int64 sequence_length, num_sequences
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "Analysis/EffectiveSampleSize.h"
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
    const int K = 3, W = 64, P = 4, steps = 900, slice = 2, split = 1;
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

    MCMC::Analysis::EffectiveSampleSize<double> es(P, W);
    for (int k = 0; k < K; ++k) es.addChain(samplers[k]->getStepIttBegin(), samplers[k]->getStepIttEnd(), slice);
    es.calculate(split != 0);

    int n = 0;
    for (auto it = samplers[0]->getStepIttBegin(); it != samplers[0]->getStepIttEnd(); ++it) ++n;
    const int32_t head[6] = {K, W, P, n, slice, split};
    std::fwrite(head, sizeof(int32_t), 6, g_out);
    for (int k = 0; k < K; ++k)
        for (auto it = samplers[k]->getStepIttBegin(); it != samplers[k]->getStepIttEnd(); ++it) std::fwrite(*it, sizeof(double), static_cast<size_t>(W) * P, g_out);
    for (int p = 0; p < P; ++p) put(es.getEss(p));
    for (int p = 0; p < P; ++p) put(es.getTau(p));
    for (int p = 0; p < P; ++p) put(static_cast<int64_t>(es.getLagsUsed(p)));
    for (int p = 0; p < P; ++p) put(static_cast<int64_t>(es.windowClosed(p) ? 1 : 0));
    for (int p = 0; p < P; ++p) put(es.getRhat(p));
    for (int p = 0; p < P; ++p) put(es.getMean(p));
    for (int p = 0; p < P; ++p) put(es.getWithin(p));
    for (int p = 0; p < P; ++p) put(es.getBetween(p));
    put(static_cast<int64_t>(es.getSequenceLength()));
    put(static_cast<int64_t>(es.getNumSequences()));
    std::fclose(g_out);
    for (int p = 0; p < P; ++p)
        std::printf("p%d: ess %.17g tau %.17g lags %lld closed %d rhat %.17g\n", p, es.getEss(p), es.getTau(p), es.getLagsUsed(p), es.windowClosed(p) ? 1 : 0, es.getRhat(p));
    std::printf("effective_sample_size_facade OK\n");
    return 0;
}
