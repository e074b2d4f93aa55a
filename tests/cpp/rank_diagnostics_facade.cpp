// rank_diagnostics_facade.cpp -- the facade's Analysis::RankDiagnostics (an extension:
// include/MCMCpp/Analysis/RankDiagnostics.h) on the chains of three of the facade's own samplers with different seeds, written
// like the analysis section of a reference-style program.  The kind of chain memory comes from the environment
// (MCMCPP_CHAIN_MEMORY=device / pinned / heap, and MCMCPP_DEVICE_ANALYSIS=0): tests/test_rank_diagnostics_facade.py runs the
// program under each and checks that every run writes the same bytes, and the results against the C ABI and the restatement
// on the chains it wrote (tests/rank_restatement.py).
//   usage: rank_diagnostics_facade <out.bin>      (needs an MI355X)
// out.bin: int32 K, W, P, n_steps, slice, split; double chains[K][n][W][P]; double rhat[P], rhat_rank[P], rhat_folded[P],
//   ess_bulk[P], ess_tail[P], ess_tail_lower[P], ess_tail_upper[P], median[P], q05[P], q95[P]; int64 closed_bulk[P],
//   closed_tail[P]; int64 sequence_length, num_sequences
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "Analysis/RankDiagnostics.h"
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

    MCMC::Analysis::RankDiagnostics<double> rd(P, W);
    for (int k = 0; k < K; ++k) rd.addChain(samplers[k]->getStepIttBegin(), samplers[k]->getStepIttEnd(), slice);
    rd.calculate(split != 0);

    int n = 0;
    for (auto it = samplers[0]->getStepIttBegin(); it != samplers[0]->getStepIttEnd(); ++it) ++n;
    const int32_t head[6] = {K, W, P, n, slice, split};
    std::fwrite(head, sizeof(int32_t), 6, g_out);
    for (int k = 0; k < K; ++k)
        for (auto it = samplers[k]->getStepIttBegin(); it != samplers[k]->getStepIttEnd(); ++it) std::fwrite(*it, sizeof(double), static_cast<size_t>(W) * P, g_out);
    for (int p = 0; p < P; ++p) put(rd.getRhat(p));
    for (int p = 0; p < P; ++p) put(rd.getRhatRank(p));
    for (int p = 0; p < P; ++p) put(rd.getRhatFolded(p));
    for (int p = 0; p < P; ++p) put(rd.getEssBulk(p));
    for (int p = 0; p < P; ++p) put(rd.getEssTail(p));
    for (int p = 0; p < P; ++p) put(rd.getEssTailLower(p));
    for (int p = 0; p < P; ++p) put(rd.getEssTailUpper(p));
    for (int p = 0; p < P; ++p) put(rd.getMedian(p));
    for (int p = 0; p < P; ++p) put(rd.getQ05(p));
    for (int p = 0; p < P; ++p) put(rd.getQ95(p));
    for (int p = 0; p < P; ++p) put(static_cast<int64_t>(rd.bulkWindowClosed(p) ? 1 : 0));
    for (int p = 0; p < P; ++p) put(static_cast<int64_t>(rd.tailWindowsClosed(p) ? 1 : 0));
    put(static_cast<int64_t>(rd.getSequenceLength()));
    put(static_cast<int64_t>(rd.getNumSequences()));
    std::fclose(g_out);
    for (int p = 0; p < P; ++p)
        std::printf("p%d: rhat %.17g bulk %.17g tail %.17g median %.17g\n", p, rd.getRhat(p), rd.getEssBulk(p), rd.getEssTail(p), rd.getMedian(p));
    std::printf("rank_diagnostics_facade OK\n");
    return 0;
}
