// Example: three independent ensembles on the skewed Gaussian of the other examples, with different seeds and starting
// clouds, followed by the rank-normalised convergence figures of both parameters (Analysis::RankDiagnostics, an extension of
// this repository): the rank-normalised split R-hat (the larger of the bulk and the folded variant), the bulk-ESS, and the
// tail-ESS that says how many draws the 5 % / 95 % bounds rest on.  On a skewed target these are the figures to read beside
// the raw-value ones of skewed_gaussian_ess.cpp.  With MCMCPP_CHAIN_MEMORY=device the chains stay in GPU memory.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/skewed_gaussian_rank_diagnostics.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o skewed_rank
//   ./skewed_rank [stored_steps]
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "Analysis/RankDiagnostics.h"
#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/StretchMove.h"

namespace Analysis = MCMC::Analysis;

int main(int argc, char** argv)
{
    typedef MCMC::Device::SkewedGaussian2D<double> Likelihood;
    typedef MCMC::Mover::StretchMove<double, Likelihood> Mover;
    typedef MCMC::EnsembleSampler<double, Mover> Sampler;
    const int numChains = 3, numWalkers = 320, numParams = 2;
    const int numSteps = argc > 1 ? std::atoi(argv[1]) : 2019;

    Likelihood likelihood(0.13);
    std::vector<std::unique_ptr<Mover> > movers;
    std::vector<std::unique_ptr<Sampler> > samplers;
    for (int k = 0; k < numChains; ++k)
    {
        const int runNumber = k;  // (the run number seeds the sampler)
        movers.push_back(std::unique_ptr<Mover>(new Mover(numParams, runNumber, likelihood)));
        samplers.push_back(std::unique_ptr<Sampler>(new Sampler(runNumber, numWalkers, numParams, *movers[k])));
        std::vector<double> initVals(numWalkers * numParams), auxVals(numWalkers);
        std::mt19937_64 engine(53 + k);
        std::normal_distribution<double> spread(0.0, 3.5);
        for (double& v : initVals) v = spread(engine);
        for (int w = 0; w < numWalkers; ++w) auxVals[w] = likelihood.calcLogPostProb(&initVals[w * numParams]);
        samplers[k]->setInitialWalkerPos(initVals.data(), auxVals.data());
        samplers[k]->runMCMC(numSteps);
    }

    // the first fifth of every chain is burn-in
    Analysis::RankDiagnostics<double> rd(numParams, numWalkers);
    for (int k = 0; k < numChains; ++k)
    {
        auto startItt = samplers[k]->getStepIttBegin();
        startItt += numSteps / 5;
        rd.addChain(startItt, samplers[k]->getStepIttEnd(), 1);
    }
    rd.calculate();
    std::printf("%lld sequences of %lld steps\n", rd.getNumSequences(), rd.getSequenceLength());
    std::printf("Parameter: R-hat | rank R-hat | folded R-hat | bulk-ESS | tail-ESS | q05 | median | q95\n");
    for (int p = 0; p < numParams; ++p)
        std::printf("P%d: %.6f | %.6f | %.6f | %.1f | %.1f | %.10g | %.10g | %.10g\n", p, rd.getRhat(p), rd.getRhatRank(p), rd.getRhatFolded(p), rd.getEssBulk(p),
                    rd.getEssTail(p), rd.getQ05(p), rd.getMedian(p), rd.getQ95(p));
    return 0;
}
