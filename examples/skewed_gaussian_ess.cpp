// Example: three independent ensembles on the skewed Gaussian of the other examples, with different seeds and starting
// clouds, followed by the split R-hat and the effective sample size of both parameters (Analysis::EffectiveSampleSize, an
// extension of this repository): R-hat near 1 says that the ensembles have converged to the same distribution, and the
// effective sample size how many independent draws their steps are worth, which sizes the error bar of a posterior mean.  With
// MCMCPP_CHAIN_MEMORY=device the chains stay in GPU memory.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/skewed_gaussian_ess.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o skewed_ess
//   ./skewed_ess [stored_steps]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "Analysis/EffectiveSampleSize.h"
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
    Analysis::EffectiveSampleSize<double> ess(numParams, numWalkers);
    for (int k = 0; k < numChains; ++k)
    {
        auto startItt = samplers[k]->getStepIttBegin();
        startItt += numSteps / 5;
        ess.addChain(startItt, samplers[k]->getStepIttEnd(), 1);
    }
    ess.calculate();
    std::printf("%lld sequences of %lld steps\n", ess.getNumSequences(), ess.getSequenceLength());
    std::printf("Parameter: R-hat | ESS | tau | lags used | window closed | mean | standard error of the mean\n");
    for (int p = 0; p < numParams; ++p)
    {
        const double variance = ess.getWithin(p) * (ess.getSequenceLength() - 1) / ess.getSequenceLength() + ess.getBetween(p);
        std::printf("P%d: %.6f | %.1f | %.3f | %lld | %d | %.10g | %.3g\n", p, ess.getRhat(p), ess.getEss(p), ess.getTau(p), ess.getLagsUsed(p),
                    ess.windowClosed(p) ? 1 : 0, ess.getMean(p), std::sqrt(variance / ess.getEss(p)));
    }
    return 0;
}
