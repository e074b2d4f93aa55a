// Example: parallel tempering on the Rosenbrock density (an extension of this repository).  Four ensembles run on a ladder
// c_k = beta_k c of Device::Rosenbrock (logp = -c sum ..., so scaling c flattens the target): rung 0 is the target of
// interest, the flatter rungs cross the curved valley easily and hand their states down through replica-exchange rounds.
// Printed: every rung's acceptance fraction of the stretch move, every pair's swap fraction, and the table of rung 0's
// posterior (Analysis::PosteriorSummary), whose chain is an ordinary chain.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/rosenbrock_tempered.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o rosenbrock_tempered
//   ./rosenbrock_tempered [stored_steps [exchange_every]]
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <vector>

#include "Analysis/PosteriorSummary.h"
#include "Device/Calculators.h"
#include "ReplicaExchangeSampler.h"

int main(int argc, char** argv)
{
    typedef MCMC::Device::Rosenbrock<double> Target;
    const int numWalkers = 512, numParams = 4, runNumber = 7;
    const int numSteps = argc > 1 ? std::atoi(argv[1]) : 2000;
    const int exchangeEvery = argc > 2 ? std::atoi(argv[2]) : 5;
    const double betas[] = {1.0, 0.5, 0.25, 0.125};
    const int numRungs = static_cast<int>(sizeof betas / sizeof betas[0]);

    std::vector<Target> ladder;
    for (int k = 0; k < numRungs; ++k) ladder.push_back(Target(numParams, 1.0, 100.0, 0.05 * betas[k]));
    MCMC::ReplicaExchangeSampler<double, Target> sampler(runNumber, numWalkers, numParams, ladder);

    for (int k = 0; k < numRungs; ++k)
    {
        std::vector<double> initVals(numWalkers * numParams), auxVals(numWalkers);
        std::mt19937_64 engine(53 + k);
        std::normal_distribution<double> spread(0.0, 1.5);
        for (double& v : initVals) v = spread(engine);
        for (int w = 0; w < numWalkers; ++w) auxVals[w] = ladder[k].calcLogPostProb(&initVals[w * numParams]);
        sampler.setInitialWalkerPos(k, initVals.data(), auxVals.data());
    }
    sampler.runMCMC(numSteps, exchangeEvery);

    std::printf("%d stored steps per rung, %llu exchange rounds\n", sampler.getStoredSteps(), static_cast<unsigned long long>(sampler.getExchangeRounds()));
    for (int k = 0; k < numRungs; ++k) std::printf("rung %d (beta %.3f): acceptance fraction %.4f\n", k, betas[k], sampler.getAcceptanceFraction(k));
    for (int k = 0; k + 1 < numRungs; ++k) std::printf("pair %d-%d: swap fraction %.4f\n", k, k + 1, sampler.getSwapFraction(k));

    // rung 0, the first fifth of the chain as burn-in
    MCMC::Analysis::PosteriorSummary<double> ps(numParams, numWalkers);
    auto startItt = sampler.getStepIttBegin(0);
    startItt += numSteps / 5;
    ps.addChain(startItt, sampler.getStepIttEnd(0), 1);
    ps.calculate();
    ps.writeTable(std::cout);
    return 0;
}
