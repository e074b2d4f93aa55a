// The reference-style program -- sample, sliceAndBurnChain, AutoCorrCalc, CovarianceMatrix, CornerHistograms,
// PercentileAndMaximumFinder -- timed phase by phase, for tools/bench_device_facade.py, which runs it with a host chain and with
// MCMCPP_CHAIN_MEMORY=device and takes the wall clock around the whole process.
//
//   bench_device_facade W D stored_steps interval
// D == 2: the reference's SkewedGaussian target (its own test shape is 320 x 2); otherwise a dense Gaussian with an AR(1)
// precision matrix.  Prints one JSON line: the phases in milliseconds, the chain's memory kind and hostBytesFetched().
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "Analysis/AutoCorrCalc.h"
#include "Analysis/CornerHistograms.h"
#include "Analysis/CovarianceMatrix.h"
#include "Analysis/PercentileAndMaximumFinder.h"
#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/StretchMove.h"

typedef std::chrono::steady_clock Clock;
static double msSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

template <class Calc>
static int program(Calc calc, int W, int D, int steps, int interval)
{
    namespace Analysis = MCMC::Analysis;
    typedef MCMC::Mover::StretchMove<double, Calc> Mover;
    const Clock::time_point start = Clock::now();
    Mover mover(D, 0, calc);
    MCMC::EnsembleSampler<double, Mover> sampler(0, W, D, mover, 8ULL << 30);
    sampler.setSlicingMode(interval > 1, interval);
    std::vector<double> pos(static_cast<size_t>(W) * D), aux(W);
    std::mt19937_64 engine(53);
    std::normal_distribution<double> spread(0.0, 1.5);
    for (double& v : pos) v = spread(engine);
    for (int w = 0; w < W; ++w) aux[w] = calc.calcLogPostProb(&pos[static_cast<size_t>(w) * D]);
    sampler.setInitialWalkerPos(pos.data(), aux.data());
    const double setupMs = msSince(start);

    Clock::time_point t = Clock::now();
    sampler.runMCMC(steps);
    const double sampleMs = msSince(t);
    t = Clock::now();
    sampler.sliceAndBurnChain(1, 20);
    const double sliceMs = msSince(t);

    auto first = sampler.getStepIttBegin();
    auto last = sampler.getStepIttEnd();
    t = Clock::now();
    Analysis::AutoCorrCalc<double> ac(D, W);
    ac.calcAutoCorrTimes(first, last, sampler.getStoredSteps());
    const double acMs = msSince(t);
    t = Clock::now();
    Analysis::CovarianceMatrix<double> cm(D, W);
    int slice = static_cast<int>(std::ceil(ac.retrieveAutoCorrelationTime(0)));
    if (slice < 1 || slice > 8) slice = 2;
    cm.calculateCovar(first, last, slice);
    const double covMs = msSince(t);
    t = Clock::now();
    Analysis::CornerHistograms<double> corner(D, W, 100);
    corner.calculateHistograms(first, last);
    const double cornerMs = msSince(t);
    t = Clock::now();
    Analysis::PercentileAndMaximumFinder<double> pamf(D, W, 10000);
    pamf.processChainData(first, last, 1);
    const double pamfMs = msSince(t);
    const bool device = sampler.chain().memoryKind() == MCMC::Chain::Detail::MemoryKind::Device;
    std::printf("{\"W\": %d, \"D\": %d, \"stored\": %d, \"interval\": %d, \"chain\": \"%s\", \"setup_ms\": %.3f, \"sample_ms\": %.3f, \"slice_ms\": %.3f, "
                "\"autocorr_ms\": %.3f, \"covariance_ms\": %.3f, \"corner_ms\": %.3f, \"percentile_ms\": %.3f, \"main_ms\": %.3f, \"host_bytes_fetched\": %llu, "
                "\"check\": %.17g}\n",
                W, D, steps, interval, device ? "device" : "host", setupMs, sampleMs, sliceMs, acMs, covMs, cornerMs, pamfMs, msSince(start),
                sampler.chain().hostBytesFetched(), cm.getCovarianceMatrixElement(0, 0) + pamf.getValueFromPercentile(0, 50) + corner.get1dHistBin(0, 50));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        std::fprintf(stderr, "usage: bench_device_facade W D stored_steps interval\n");
        return 2;
    }
    const int W = std::atoi(argv[1]), D = std::atoi(argv[2]), steps = std::atoi(argv[3]), interval = std::atoi(argv[4]);
    if (D == 2) return program(MCMC::Device::SkewedGaussian2D<double>(0.13), W, D, steps, interval);
    const std::vector<double> P = MCMC::Device::DenseGaussian<double>::ar1Precision(D, 0.5);
    return program(MCMC::Device::DenseGaussian<double>(D, P.data()), W, D, steps, interval);
}
