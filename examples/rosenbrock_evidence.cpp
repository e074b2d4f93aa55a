// Example: the evidence of a model from an ordinary run (an extension of this repository).  One ensemble samples the Rosenbrock
// density logp = -c (b (y - x^2)^2 + (a - x)^2) at D = 2, whose normalising constant is known: Z = pi / (c sqrt(b)).  No ladder:
// gaussianBridgeEvidence fits a Gaussian to the first half of the chain behind the burn-in and bridges the target and that
// normalised density with the second half (mcmcpp_hip_evidence_gaussian).  The chain is kept in GPU memory and read where it lies.
// Printed: the estimate of log Z with its standard error, the overlap of target and Gaussian, and log(pi / (c sqrt(b))).
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/rosenbrock_evidence.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o rosenbrock_evidence
//   ./rosenbrock_evidence [stored_steps [dump_file]]
// dump_file receives, as doubles: W, D, stored steps, burn-in, seed, the estimate, mcse, overlap, the mean [D], the factor [D][D]
// and the chain [steps][W][D] (tests/test_evidence_gaussian_facade.py compares with the Python wrapper on the same chain).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/StretchMove.h"

int main(int argc, char** argv)
{
    setenv("MCMCPP_CHAIN_MEMORY", "device", 0);  // (0: a value the caller has set stays)
    typedef MCMC::Device::Rosenbrock<double> Target;
    typedef MCMC::Mover::StretchMove<double, Target> Mover;
    const int runNumber = 3, numWalkers = 64, numParams = 2, seed = 11;
    const int numSteps = argc > 1 ? std::atoi(argv[1]) : 2000;
    const double a = 1.0, b = 4.0, c = 1.0;

    Target target(numParams, a, b, c);
    Mover mover(numParams, runNumber, target);
    MCMC::EnsembleSampler<double, Mover> sampler(runNumber, numWalkers, numParams, mover);
    std::vector<double> initVals(numWalkers * numParams), auxVals(numWalkers);
    std::mt19937_64 engine(53);
    std::normal_distribution<double> spread(1.0, 0.5);
    for (double& v : initVals) v = spread(engine);
    for (int w = 0; w < numWalkers; ++w) auxVals[w] = target.calcLogPostProb(&initVals[w * numParams]);
    sampler.setInitialWalkerPos(initVals.data(), auxVals.data());
    sampler.runMCMC(numSteps);

    const int burnIn = numSteps / 5;
    const MCMC::GaussianBridgeEvidence e = sampler.gaussianBridgeEvidence(burnIn, 1, seed);
    const double truth = std::log(3.14159265358979323846 / (c * std::sqrt(b)));
    std::printf("%d stored steps, burn-in %d, %lld draws bridged against as many proposals, %lld passes\n", sampler.getStoredSteps(), burnIn,
                static_cast<long long>(e.numDraws), static_cast<long long>(e.passes));
    std::printf("log Z estimate %.17g\nmcse %.17g\noverlap %.17g\nlog(pi / (c sqrt(b))) %.17g\n", e.logEvidence, e.mcse, e.overlap, truth);
    std::printf("within four standard errors: %s\n", std::fabs(e.logEvidence - truth) <= 4.0 * e.mcse ? "yes" : "no");

    if (argc > 2)
    {
        std::vector<double> out;
        const double head[] = {double(numWalkers), double(numParams), double(sampler.getStoredSteps()), double(burnIn), double(seed), e.logEvidence, e.mcse, e.overlap};
        out.insert(out.end(), head, head + 8);
        out.insert(out.end(), e.mean.begin(), e.mean.end());
        out.insert(out.end(), e.chol.begin(), e.chol.end());
        for (auto itt = sampler.getStepIttBegin(); itt != sampler.getStepIttEnd(); ++itt)
        {
            const double* step = *itt;
            out.insert(out.end(), step, step + numWalkers * numParams);
        }
        std::FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 1;
        std::fclose(f);
    }
    return 0;
}
