// Example: three independent ensembles on the skewed Gaussian of the other examples, with different seeds and starting
// clouds, followed by the Gelman-Rubin split R-hat of both parameters (Analysis::GelmanRubin, an extension of this repository):
// values near 1 say that the ensembles have converged to the same distribution.  With MCMCPP_CHAIN_MEMORY=device the chains are
// read in GPU memory.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/skewed_gaussian_rhat.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o skewed_rhat
//   ./skewed_rhat [stored_steps]
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "Analysis/GelmanRubin.h"
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
    Analysis::GelmanRubin<double> gr(numParams, numWalkers);
    for (int k = 0; k < numChains; ++k)
    {
        auto startItt = samplers[k]->getStepIttBegin();
        startItt += numSteps / 5;
        gr.addChain(startItt, samplers[k]->getStepIttEnd(), 1);
    }
    gr.calculate();
    std::printf("%lld sequences of %lld steps\n", gr.getNumSequences(), gr.getSequenceLength());
    std::printf("Parameter: R-hat | mean | within | between\n");
    for (int p = 0; p < numParams; ++p) std::printf("P%d: %.6f | %.10g | %.10g | %.10g\n", p, gr.getRhat(p), gr.getMean(p), gr.getWithin(p), gr.getBetween(p));
    std::printf("Chain, parameter: mean | within\n");
    for (int k = 0; k < numChains; ++k)
        for (int p = 0; p < numParams; ++p) std::printf("C%d, P%d: %.10g | %.10g\n", k, p, gr.getChainMean(k, p), gr.getChainWithin(k, p));
    return 0;
}
