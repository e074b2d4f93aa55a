// Example: the evidence ratio across a whole tempering ladder, by pairs and by all rungs at once (an extension of this
// repository).  Three ensembles run on the ladder P_k = beta_k P of Device::DenseGaussian, beta = 1, 0.7, 0.49, in D = 4
// dimensions: the ladder of gaussian_evidence_bridge.cpp.  The targets exp(-x' P_k x / 2) are not normalised:
// Z_k = (2 pi)^(D/2) / sqrt(det P_k), so log(Z_p / Z_{p+1}) = (D / 2) log(beta_{p+1} / beta_p) exactly.
// ReplicaExchangeSampler::evidenceBridge estimates each pair on its own and adds the pairs' errors as if they were independent;
// ReplicaExchangeSampler::evidenceMbar (the multistate Bennett acceptance ratio) solves for all rungs jointly from every draw
// of every rung and takes the error of the total from the covariance of the estimates.
// Printed: the ratios of both beside the closed form, then the totals with their standard errors.
//
//   g++ -std=c++11 -O2 -I include/MCMCpp -I include examples/gaussian_evidence_mbar.cpp
//       -L mcmcpp_amd -lmcmcpp_hip -Wl,-rpath,$PWD/mcmcpp_amd -o gaussian_evidence_mbar
//   ./gaussian_evidence_mbar [stored_steps [exchange_every]]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "Device/Calculators.h"
#include "ReplicaExchangeSampler.h"

int main(int argc, char** argv)
{
    typedef MCMC::Device::DenseGaussian<double> Target;
    const int numWalkers = 256, numParams = 4, runNumber = 11;
    const int numSteps = argc > 1 ? std::atoi(argv[1]) : 1000;
    const int exchangeEvery = argc > 2 ? std::atoi(argv[2]) : 5;
    const double betas[] = {1.0, 0.7, 0.49};
    const int numRungs = static_cast<int>(sizeof betas / sizeof betas[0]);

    // P = A A' / D + I, a fixed correlated precision matrix
    std::vector<double> a(numParams * numParams), prec(numParams * numParams);
    std::mt19937_64 matrixEngine(5);
    std::normal_distribution<double> unit(0.0, 1.0);
    for (double& v : a) v = unit(matrixEngine);
    for (int i = 0; i < numParams; ++i)
        for (int j = 0; j < numParams; ++j)
        {
            double s = 0.0;
            for (int l = 0; l < numParams; ++l) s += a[i * numParams + l] * a[j * numParams + l];
            prec[i * numParams + j] = s / numParams + (i == j ? 1.0 : 0.0);
        }

    std::vector<Target> ladder;
    for (int k = 0; k < numRungs; ++k)
    {
        std::vector<double> scaled(prec);
        for (double& v : scaled) v *= betas[k];
        ladder.push_back(Target(numParams, scaled.data()));
    }
    MCMC::ReplicaExchangeSampler<double, Target> sampler(runNumber, numWalkers, numParams, ladder);
    for (int k = 0; k < numRungs; ++k)
    {
        std::vector<double> initVals(numWalkers * numParams), auxVals(numWalkers);
        std::mt19937_64 engine(53 + k);
        for (double& v : initVals) v = unit(engine);
        for (int w = 0; w < numWalkers; ++w) auxVals[w] = ladder[k].calcLogPostProb(&initVals[w * numParams]);
        sampler.setInitialWalkerPos(k, initVals.data(), auxVals.data());
    }
    sampler.runMCMC(numSteps, exchangeEvery);

    // the first fifth of every rung's chain as burn-in
    const MCMC::EvidenceBridge b = sampler.evidenceBridge(numSteps / 5, 1);
    const MCMC::EvidenceMbar m = sampler.evidenceMbar(numSteps / 5, 1);
    std::printf("%d stored steps per rung, %lld draws per rung used, %lld passes of the joint solve, converged %lld\n", sampler.getStoredSteps(),
                static_cast<long long>(m.numDraws), static_cast<long long>(m.passes), static_cast<long long>(m.converged));
    std::printf("log(Z_p / Z_p+1)    pairwise       mcse            mbar       mcse   analytic\n");
    double analyticTotal = 0.0;
    for (int p = 0; p + 1 < numRungs; ++p)
    {
        const double analytic = 0.5 * numParams * std::log(betas[p + 1] / betas[p]);
        analyticTotal += analytic;
        std::printf("pair %d-%d  %14.9f  %9.6f  %14.9f  %9.6f  %9.6f\n", p, p + 1, b.logRatio[p], b.mcse[p], m.logRatio[p], m.mcse[p], analytic);
    }
    std::printf("total     %14.9f  %9.6f  %14.9f  %9.6f  %9.6f\n", b.logRatioTotal, b.mcseTotal, m.logRatioTotal, m.mcseTotal, analyticTotal);
    return 0;
}
