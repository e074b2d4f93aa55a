// evidence_mbar_facade.cpp -- ReplicaExchangeSampler::evidenceMbar on a small dense-Gaussian ladder, for
// tests/test_evidence_mbar_facade.py:  evidence_mbar_facade <out file>
// Writes, as raw doubles: K, stored steps n, W, D, burn-in, slice interval, num_draws; the K precision matrices [K][D][D]; the
// stored steps of every rung [K][n][W][D]; then log_z [K], cov [K][K], log_ratio, mcse [K-1], ess [K], nonfinite [K][K],
// log_ratio_total, mcse_total, passes, converged.  The test gives the same chains to the C entry point through a handle of its own.
#include <cstdio>
#include <random>
#include <vector>

#include "Device/Calculators.h"
#include "ReplicaExchangeSampler.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    typedef MCMC::Device::DenseGaussian<double> Target;
    const int W = 32, D = 4, K = 3, steps = 120, burn = 21, slice = 2;
    const double betas[K] = {1.0, 0.7, 0.49};
    std::vector<double> out;
    std::vector<Target> ladder;
    std::vector<double> matrices;
    for (int k = 0; k < K; ++k)
    {
        std::vector<double> prec(D * D);
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) prec[i * D + j] = betas[k] * ((i == j ? 1.5 : 0.0) + 0.25 / (1.0 + (i > j ? i - j : j - i)));
        matrices.insert(matrices.end(), prec.begin(), prec.end());
        ladder.push_back(Target(D, prec.data()));
    }
    MCMC::ReplicaExchangeSampler<double, Target> sampler(3, W, D, ladder);
    std::normal_distribution<double> unit(0.0, 1.0);
    for (int k = 0; k < K; ++k)
    {
        std::vector<double> pos(W * D), aux(W);
        std::mt19937_64 engine(7 + k);
        for (double& v : pos) v = unit(engine);
        for (int w = 0; w < W; ++w) aux[w] = ladder[k].calcLogPostProb(&pos[w * D]);
        sampler.setInitialWalkerPos(k, pos.data(), aux.data());
    }
    if (!sampler.runMCMC(steps, 3)) return 3;
    const MCMC::EvidenceMbar r = sampler.evidenceMbar(burn, slice);
    const int n = sampler.getStoredSteps();
    const double head[7] = {double(K), double(n), double(W), double(D), double(burn), double(slice), double(r.numDraws)};
    out.assign(head, head + 7);
    out.insert(out.end(), matrices.begin(), matrices.end());
    for (int k = 0; k < K; ++k)
        for (auto itt = sampler.getStepIttBegin(k); itt != sampler.getStepIttEnd(k); ++itt) out.insert(out.end(), *itt, *itt + W * D);
    if (r.numRungs != K || r.at(1, 2) != 5u || r.logZ.size() != 3u || r.cov.size() != 9u || r.logRatio.size() != 2u || r.nonfinite.size() != 9u) return 4;
    out.insert(out.end(), r.logZ.begin(), r.logZ.end());
    out.insert(out.end(), r.cov.begin(), r.cov.end());
    out.insert(out.end(), r.logRatio.begin(), r.logRatio.end());
    out.insert(out.end(), r.mcse.begin(), r.mcse.end());
    out.insert(out.end(), r.ess.begin(), r.ess.end());
    for (std::int64_t c : r.nonfinite) out.push_back(double(c));
    out.push_back(r.logRatioTotal);
    out.push_back(r.mcseTotal);
    out.push_back(double(r.passes));
    out.push_back(double(r.converged));
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 5;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 6;
}
