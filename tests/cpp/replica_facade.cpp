// replica_facade.cpp -- MCMC::ReplicaExchangeSampler driven by tests/test_replica_facade.py.
//   replica_facade mismatch                          rungs whose calculators differ: the constructor's message, exit code 3 (no device)
//   replica_facade run IN OUT W D steps every seed   a Rosenbrock ladder c = 0.05 * (1, 0.5, 0.25) from the state in IN
//                                                    (pos [3][W][D], logp [3][W], doubles); rung 0's stored steps to OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "Device/Calculators.h"
#include "ReplicaExchangeSampler.h"

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "mismatch") == 0)
    {
        typedef MCMC::Device::DenseGaussian<double> Dense;
        const std::vector<double> p3 = Dense::ar1Precision(3, 0.5), p4 = Dense::ar1Precision(4, 0.5);
        std::vector<Dense> rungs;
        rungs.push_back(Dense(3, p3.data()));
        rungs.push_back(Dense(4, p4.data()));
        try
        {
            MCMC::ReplicaExchangeSampler<double, Dense> s(1, 64, 3, rungs);
        }
        catch (const std::invalid_argument& e)
        {
            std::printf("%s\n", e.what());
            return 3;
        }
        return 0;
    }
    if (argc != 9 || std::strcmp(argv[1], "run") != 0) return 2;
    typedef MCMC::Device::Rosenbrock<double> Target;
    const int W = std::atoi(argv[4]), D = std::atoi(argv[5]), steps = std::atoi(argv[6]), every = std::atoi(argv[7]), seed = std::atoi(argv[8]);
    const int K = 3;
    const double betas[K] = {1.0, 0.5, 0.25};
    std::vector<Target> ladder;
    for (int k = 0; k < K; ++k) ladder.push_back(Target(D, 1.0, 100.0, 0.05 * betas[k]));
    std::vector<double> pos((size_t)K * W * D), logp((size_t)K * W);
    FILE* in = std::fopen(argv[2], "rb");
    if (!in || std::fread(pos.data(), sizeof(double), pos.size(), in) != pos.size() || std::fread(logp.data(), sizeof(double), logp.size(), in) != logp.size()) return 4;
    std::fclose(in);
    MCMC::ReplicaExchangeSampler<double, Target> sampler(seed, W, D, ladder);
    for (int k = 0; k < K; ++k)
    {
        // (the host calculator gives the log-posteriors the caller computed)
        for (int w = 0; w < W; ++w)
            if (ladder[k].calcLogPostProb(&pos[((size_t)k * W + w) * D]) != logp[(size_t)k * W + w]) return 5;
        sampler.setInitialWalkerPos(k, &pos[(size_t)k * W * D], &logp[(size_t)k * W]);
    }
    if (!sampler.runMCMC(steps, every)) return 6;
    if (sampler.getStoredSteps() != steps + 1) return 7;
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 8;
    for (MCMC::ReplicaExchangeSampler<double, Target>::StepItt it = sampler.getStepIttBegin(0); it != sampler.getStepIttEnd(0); ++it)
        std::fwrite(*it, sizeof(double), (size_t)W * D, out);
    std::fclose(out);
    for (int k = 0; k < K; ++k) std::printf("acceptance %d %.17g\n", k, sampler.getAcceptanceFraction(k));
    for (int k = 0; k + 1 < K; ++k) std::printf("swap %d %.17g\n", k, sampler.getSwapFraction(k));
    std::printf("rounds %llu\n", (unsigned long long)sampler.getExchangeRounds());
    return 0;
}
