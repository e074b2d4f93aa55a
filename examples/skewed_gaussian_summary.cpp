// Example: three independent ensembles on the skewed Gaussian of the other examples, with different seeds and starting
// clouds, followed by the table a user prints (Analysis::PosteriorSummary, an extension of this repository): mean, sd, the
// 5 %, 50 % and 95 % quantiles and the 94 % highest-density interval of both parameters, each with its Monte Carlo standard
// error -- how many digits of the figure are real -- and beside it the rank-normalised R-hat, bulk-ESS and tail-ESS of
// Analysis::RankDiagnostics.  With MCMCPP_CHAIN_MEMORY=device the chains stay in GPU memory.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/skewed_gaussian_summary.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o skewed_summary
//   ./skewed_summary [stored_steps]
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <random>
#include <vector>

#include "Analysis/PosteriorSummary.h"
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
    Analysis::PosteriorSummary<double> ps(numParams, numWalkers);
    Analysis::RankDiagnostics<double> rd(numParams, numWalkers);
    for (int k = 0; k < numChains; ++k)
    {
        auto startItt = samplers[k]->getStepIttBegin();
        startItt += numSteps / 5;
        ps.addChain(startItt, samplers[k]->getStepIttEnd(), 1);
        rd.addChain(startItt, samplers[k]->getStepIttEnd(), 1);
    }
    ps.calculate();
    rd.calculate();
    std::printf("%lld sequences of %lld steps\n", ps.getNumSequences(), ps.getSequenceLength());
    ps.writeTable(std::cout);
    std::printf("Parameter: R-hat | bulk-ESS | tail-ESS\n");
    for (int p = 0; p < numParams; ++p) std::printf("P%d: %.6f | %.1f | %.1f\n", p, rd.getRhat(p), rd.getEssBulk(p), rd.getEssTail(p));
    return 0;
}
