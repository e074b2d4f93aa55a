// Example: the reference's SkewedGaussian/StretchMove demo with its analysis section, with the chain kept in GPU memory.
//
// The program text is the reference-style flow -- runMCMC, sliceAndBurnChain, AutoCorrCalc, CovarianceMatrix,
// CornerHistograms, PercentileAndMaximumFinder -- unchanged.  What keeps the chain on the device is one variable of the
// environment, MCMCPP_CHAIN_MEMORY=device (set here when the caller has not chosen): the run stores its steps into one device
// allocation, sliceAndBurnChain compacts them there with a kernel, and the four analysis classes read them where they lie.
// The last lines print the chain's memory kind and the bytes of stored steps that came to the host: none, until the program
// dereferences an iterator.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/skewed_gaussian_device_chain.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o skewed_device_chain
//   ./skewed_device_chain [stored_steps] [output directory]
//   MCMCPP_CHAIN_MEMORY=heap ./skewed_device_chain        (the same program with a host chain: the same numbers)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "Analysis/AutoCorrCalc.h"
#include "Analysis/CornerHistograms.h"
#include "Analysis/CovarianceMatrix.h"
#include "Analysis/PercentileAndMaximumFinder.h"
#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/StretchMove.h"

namespace Analysis = MCMC::Analysis;

int main(int argc, char** argv)
{
    setenv("MCMCPP_CHAIN_MEMORY", "device", 0);  // (0: a value the caller has set stays)
    typedef MCMC::Device::SkewedGaussian2D<double> Likelihood;
    typedef MCMC::Mover::StretchMove<double, Likelihood> Mover;
    const int runNumber = 0, numWalkers = 320, numParams = 2, cornerBinning = 100;
    const int numSteps = argc > 1 ? std::atoi(argv[1]) : 4019;
    const std::string dir = argc > 2 ? std::string(argv[2]) + "/" : std::string();

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
    std::printf("Acceptance Fraction: %llu/%llu\n", sampler.getAcceptedSteps(), sampler.getTotalSteps());

    Analysis::AutoCorrCalc<double> acCalc(numParams, numWalkers);
    auto startItt = sampler.getStepIttBegin();
    auto endItt = sampler.getStepIttEnd();
    acCalc.calcAutoCorrTimes(startItt, endItt, sampler.getStoredSteps());
    const double p0Ac = acCalc.retrieveAutoCorrelationTime(0);
    const double p1Ac = acCalc.retrieveAutoCorrelationTime(1);
    std::printf("P0 Calculated AutoCorrelation Time: %g\nP1 Calculated AutoCorrelation Time: %g\n", p0Ac, p1Ac);

    Analysis::CovarianceMatrix<double> cmCalc(numParams, numWalkers);
    int sliceInterval = static_cast<int>((p0Ac < p1Ac) ? std::ceil(p0Ac) : std::ceil(p1Ac));
    if (sliceInterval < 1) sliceInterval = 1;  // (a window that never closed gives a negative time)
    cmCalc.calculateCovar(startItt, endItt, sliceInterval);
    std::printf("Covariance matrix with slicing\n%g, %g\n%g, %g\n", cmCalc.getCovarianceMatrixElement(0, 0), cmCalc.getCovarianceMatrixElement(0, 1),
                cmCalc.getCovarianceMatrixElement(1, 0), cmCalc.getCovarianceMatrixElement(1, 1));

    Analysis::CornerHistograms<double> cornerHists(numParams, numWalkers, cornerBinning);
    cornerHists.calculateHistograms(startItt, endItt);
    cornerHists.saveHistsCsvFormat(dir + "chainHist");

    Analysis::PercentileAndMaximumFinder<double> pamf(numParams, numWalkers, 100 * cornerBinning);
    pamf.processChainData(startItt, endItt, 1);
    std::printf("The 15.9, 50, 84.1 percentiles are:\n");
    for (int p = 0; p < numParams; ++p)
        std::printf("P%d: %g, %g, %g\n", p, pamf.getValueFromPercentile(p, 15.9), pamf.getValueFromPercentile(p, 50), pamf.getValueFromPercentile(p, 84.1));

    const MCMC::Chain::Detail::MemoryKind kind = sampler.chain().memoryKind();
    std::printf("Chain memory: %s, %d stored steps, %lld of them in device memory\n",
                kind == MCMC::Chain::Detail::MemoryKind::Device ? "device" : (kind == MCMC::Chain::Detail::MemoryKind::Pinned ? "pinned" : "heap"),
                sampler.getStoredSteps(), static_cast<long long>(sampler.chain().deviceSteps().steps));
    std::printf("Bytes of stored steps copied to the host so far: %llu\n", sampler.chain().hostBytesFetched());
    const double* last = *(--sampler.getStepIttEnd());  // the iterators still hand out host pointers: this downloads one step
    std::printf("Last stored step, walker 0: %g, %g\n", last[0], last[1]);
    std::printf("Bytes of stored steps copied to the host so far: %llu\n", sampler.chain().hostBytesFetched());
    return 0;
}
