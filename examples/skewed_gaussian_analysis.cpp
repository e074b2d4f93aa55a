// Example: the analysis section of the reference's SkewedGaussian/StretchMove demo, written against this repository's
// headers: autocorrelation times, the covariance matrix with slicing, corner histograms (100 bins per axis), the
// percentile finder (10 000 bins), its CSV files, the peaks and the 15.9 / 50 / 84.1 percentiles -- every analysis class
// the reference's program uses, each counting or summing on the MI355X.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/skewed_gaussian_analysis.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o skewed_analysis
//   ./skewed_analysis [stored_steps] [output directory]
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

    std::printf("Calculating integrated autocorrelation times\n");
    Analysis::AutoCorrCalc<double> acCalc(numParams, numWalkers);
    auto startItt = sampler.getStepIttBegin();
    auto endItt = sampler.getStepIttEnd();
    acCalc.calcAutoCorrTimes(startItt, endItt, sampler.getStoredSteps());
    const double p0Ac = acCalc.retrieveAutoCorrelationTime(0);
    const double p1Ac = acCalc.retrieveAutoCorrelationTime(1);
    std::printf("P0 Calculated AutoCorrelation Time: %g\nP1 Calculated AutoCorrelation Time: %g\n", p0Ac, p1Ac);

    std::printf("Calculating the covariance matrix with slicing\n");
    Analysis::CovarianceMatrix<double> cmCalc(numParams, numWalkers);
    int sliceInterval = static_cast<int>((p0Ac < p1Ac) ? std::ceil(p0Ac) : std::ceil(p1Ac));
    if (sliceInterval < 1) sliceInterval = 1;  // (a window that never closed gives a negative time)
    cmCalc.calculateCovar(startItt, endItt, sliceInterval);
    std::printf("Covariance matrix with slicing\n%g, %g\n%g, %g\n", cmCalc.getCovarianceMatrixElement(0, 0), cmCalc.getCovarianceMatrixElement(0, 1),
                cmCalc.getCovarianceMatrixElement(1, 0), cmCalc.getCovarianceMatrixElement(1, 1));

    std::printf("Generating Corner Histograms\n");
    Analysis::CornerHistograms<double> cornerHists(numParams, numWalkers, cornerBinning);
    cornerHists.calculateHistograms(startItt, endItt);
    cornerHists.saveHistsCsvFormat(dir + "chainHist");

    std::printf("Generating Percentile and Peak Finding Histograms\n");
    Analysis::PercentileAndMaximumFinder<double> pamf(numParams, numWalkers, 100 * cornerBinning);
    pamf.processChainData(startItt, endItt, 1);
    pamf.writeHistogramsInCsvFormat(dir + "percentileHistograms");

    std::printf("Parameter, Peak Percentile, Peak Value, 34.1%% down, 34.1%% up\n");
    for (int p = 0; p < numParams; ++p)
    {
        const double peak = pamf.getValueOfPeak(p);
        const double percentile = pamf.getPercentileFromValue(p, peak);
        std::printf("P%d: %g, %g, %g, %g\n", p, percentile, peak, pamf.getValueFromPercentile(p, percentile - 34.1),
                    pamf.getValueFromPercentile(p, percentile + 34.1));
    }
    std::printf("The 15.9, 50, 84.1 percentiles are:\n");
    for (int p = 0; p < numParams; ++p)
        std::printf("P%d: %g, %g, %g\n", p, pamf.getValueFromPercentile(p, 15.9), pamf.getValueFromPercentile(p, 50), pamf.getValueFromPercentile(p, 84.1));
    std::printf("Samples clamped into the end bins (corner / percentile): %lld %lld / %lld %lld\n", cornerHists.getClampedCount(0),
                cornerHists.getClampedCount(1), pamf.getClampedCount(0), pamf.getClampedCount(1));
    return 0;
}
