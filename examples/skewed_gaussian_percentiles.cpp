// Example: the skewed-Gaussian run of the other examples, followed by the exact median and 16 / 84 bounds of both parameters
// (Analysis::ExactPercentiles, an extension of this repository), with the figures of the reference's binned
// PercentileAndMaximumFinder beside them.  The two classes answer the same question; the reference's interpolates inside one of
// its 10 000 bins -- and reads parameter 0's cumulative sums for every parameter -- while the exact one selects samples of the
// chain.  With MCMCPP_CHAIN_MEMORY=device both read the chain in GPU memory.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/skewed_gaussian_percentiles.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o skewed_percentiles
//   ./skewed_percentiles [stored_steps]
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "Analysis/ExactPercentiles.h"
#include "Analysis/PercentileAndMaximumFinder.h"
#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/StretchMove.h"

namespace Analysis = MCMC::Analysis;

int main(int argc, char** argv)
{
    typedef MCMC::Device::SkewedGaussian2D<double> Likelihood;
    typedef MCMC::Mover::StretchMove<double, Likelihood> Mover;
    const int runNumber = 0, numWalkers = 320, numParams = 2;
    const int numSteps = argc > 1 ? std::atoi(argv[1]) : 4019;

    Likelihood likelihood(0.13);
    Mover mover(numParams, runNumber, likelihood);
    MCMC::EnsembleSampler<double, Mover> sampler(runNumber, numWalkers, numParams, mover);
    sampler.setSlicingMode(true, 30);
    std::vector<double> initVals(numWalkers * numParams), auxVals(numWalkers);
    std::mt19937_64 engine(53);
    std::normal_distribution<double> spread(0.0, 3.5);
    for (double& v : initVals) v = spread(engine);
    for (int w = 0; w < numWalkers; ++w) auxVals[w] = likelihood.calcLogPostProb(&initVals[w * numParams]);
    sampler.setInitialWalkerPos(initVals.data(), auxVals.data());
    sampler.runMCMC(numSteps);
    sampler.sliceAndBurnChain(1, 20);
    auto startItt = sampler.getStepIttBegin();
    auto endItt = sampler.getStepIttEnd();

    const std::vector<double> percentiles = {16.0, 50.0, 84.0};
    Analysis::ExactPercentiles<double> exact(numParams, numWalkers);
    exact.processChainData(startItt, endItt, 1, percentiles);
    Analysis::PercentileAndMaximumFinder<double> pamf(numParams, numWalkers, 10000);
    pamf.processChainData(startItt, endItt, 1);

    std::printf("%lld samples of each parameter\n", exact.getNumPoints());
    std::printf("Parameter, percentile: exact value [the samples on either side] | PercentileAndMaximumFinder\n");
    for (int p = 0; p < numParams; ++p)
        for (int k = 0; k < 3; ++k)
            std::printf("P%d, %g: %.10g [%.10g, %.10g] | %.10g\n", p, percentiles[k], exact.getValueFromPercentile(p, k), exact.getLowerValue(p, k),
                        exact.getHigherValue(p, k), pamf.getValueFromPercentile(p, percentiles[k]));

    // and back: the exact percentile of the three values just found
    std::vector<double> values(numParams * 3);
    for (int p = 0; p < numParams; ++p)
        for (int k = 0; k < 3; ++k) values[p * 3 + k] = exact.getValueFromPercentile(p, k);
    exact.processValues(startItt, endItt, 1, values);
    std::printf("Parameter, value: exact percentile (samples below / not above) | PercentileAndMaximumFinder\n");
    for (int p = 0; p < numParams; ++p)
        for (int k = 0; k < 3; ++k)
            std::printf("P%d, %.10g: %.6f (%lld / %lld) | %.6f\n", p, values[p * 3 + k], exact.getPercentileFromValue(p, k), exact.getCountBelow(p, k),
                        exact.getCountNotAbove(p, k), pamf.getPercentileFromValue(p, values[p * 3 + k]));
    return 0;
}
