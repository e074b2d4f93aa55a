// gaussian_bridge_facade.cpp -- gaussianBridgeEvidence as ParallelEnsembleSampler and ReplicaExchangeSampler reach it
// (tests/test_evidence_gaussian_facade.py compiles and links this with -Werror; examples/rosenbrock_evidence.cpp covers
// EnsembleSampler).  With an argument it runs both on the GPU and prints the two estimates; without one it only says so.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "Device/Calculators.h"
#include "Movers/StretchMove.h"
#include "ParallelEnsembleSampler.h"
#include "ReplicaExchangeSampler.h"

typedef MCMC::Device::Rosenbrock<double> Target;
typedef MCMC::Mover::StretchMove<double, Target> Mover;

static void place(Target& target, int seed, int numWalkers, int numParams, std::vector<double>& pos, std::vector<double>& aux)
{
    pos.resize(static_cast<std::size_t>(numWalkers) * numParams);
    aux.resize(static_cast<std::size_t>(numWalkers));
    std::mt19937_64 engine(seed);
    std::normal_distribution<double> spread(1.0, 0.5);
    for (double& v : pos) v = spread(engine);
    for (int w = 0; w < numWalkers; ++w) aux[w] = target.calcLogPostProb(&pos[w * numParams]);
}

int main(int argc, char**)
{
    if (argc < 2)
    {
        std::printf("compiled; give an argument to run on the GPU\n");
        return 0;
    }
    setenv("MCMCPP_CHAIN_MEMORY", "device", 0);  // (as the example: the parallel sampler's chain is read in place, the rungs' chains are host chains)
    const int numWalkers = 64, numParams = 2, steps = 200;
    std::vector<double> pos, aux;

    Target target(numParams, 1.0, 4.0, 1.0);
    Mover mover(numParams, 3, target);
    MCMC::ParallelEnsembleSampler<double, Mover> parallel(3, 2, numWalkers, numParams, mover);
    place(target, 53, numWalkers, numParams, pos, aux);
    parallel.setInitialWalkerPos(pos.data(), aux.data());
    parallel.runMCMC(steps);
    const MCMC::GaussianBridgeEvidence a = parallel.gaussianBridgeEvidence(steps / 5, 1, 11);
    std::printf("parallel %.17g %.17g\n", a.logEvidence, a.mcse);

    std::vector<Target> ladder;
    ladder.push_back(Target(numParams, 1.0, 4.0, 1.0));
    ladder.push_back(Target(numParams, 1.0, 4.0, 0.5));
    MCMC::ReplicaExchangeSampler<double, Target> tempered(3, numWalkers, numParams, ladder);
    for (int k = 0; k < 2; ++k)
    {
        place(ladder[k], 53 + k, numWalkers, numParams, pos, aux);
        tempered.setInitialWalkerPos(k, pos.data(), aux.data());
    }
    tempered.runMCMC(steps, 5);
    for (int k = 0; k < 2; ++k)
    {
        const MCMC::GaussianBridgeEvidence r = tempered.gaussianBridgeEvidence(k, steps / 5, 1, 11);
        std::printf("rung %d %.17g %.17g\n", k, r.logEvidence, r.mcse);
    }
    return 0;
}
