/*
 * Analysis/GelmanRubin.h -- the Gelman-Rubin potential scale reduction (split R-hat, BDA3 form) of every parameter over the
 * chains of several samplers, computed on the MI355X: have independent ensembles of one target converged to one distribution?
 *
 * An EXTENSION: not in the reference, which has no convergence diagnostic across chains.
 *
 *     MCMC::Analysis::GelmanRubin<double> gr(numParams, numWalkers);
 *     gr.addChain(samplerA.getStepIttBegin(), samplerA.getStepIttEnd(), sliceInterval);   // once per chain, the same number
 *     gr.addChain(samplerB.getStepIttBegin(), samplerB.getStepIttEnd(), sliceInterval);   // of steps in each
 *     gr.calculate();                    // split = true: every walker's first and second half are two sequences
 *     gr.getRhat(p);  gr.getMean(p);  gr.getWithin(p);  gr.getBetween(p);
 *     gr.getChainMean(k, p);  gr.getChainWithin(k, p);   // which ensemble disagrees
 *     gr.getSequenceLength();  gr.getNumSequences();
 *
 * Every walker of every chain is a sequence (two with split: used steps [0, L) and [n - L, n), L = n / 2): M = K H W sequences
 * of L steps.  within is the mean of the sequences' variances, between the variance of their means (B / L in BDA3's notation),
 * rhat = sqrt(((L - 1) / L within + between) / within).  All results are double; include/mcmcpp_hip.h
 * (mcmcpp_hip_gelman_rubin) has the definition to the last rounding: every sum has one fixed shape, so a figure is a function of
 * the samples alone, wherever the chains lie.
 *
 * Host chains go to the library in one call.  The steps of device chains (MCMCPP_CHAIN_MEMORY=device) are read where they lie
 * and no step comes to the host: every sampler's chain is an allocation of its own, so each is its own call
 * (mcmcpp_hip_gelman_rubin_device with one chain), which leaves the M x P sequence means and sums of squares; those few numbers
 * are then combined here by the header's rules.  No GPU, no result: failures abort with the library's message, like everything
 * else in this facade.
 */
#ifndef MCMCPP_ANALYSIS_GELMANRUBIN_H
#define MCMCPP_ANALYSIS_GELMANRUBIN_H

#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../Chain/ChainStepIterator.h"
#include "../Device/HipBackend.h"
#include "Detail/ChainSet.h"

namespace MCMC
{
namespace Analysis
{
template <class ParamType>
class GelmanRubin
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    GelmanRubin(int numParams, int numWalkers) : pCount(numParams), wCount(numWalkers), chains(numParams, numWalkers), seqLength(0), seqCount(0)
    {
        assert(pCount > 0);
        assert(wCount > 0);
    }

    /// One chain: every sliceInterval'th step of [start, end), beginning with `start`.  Every chain must give the same number
    /// of used steps.
    void addChain(IttType start, IttType end, int sliceInterval) { chains.addChain(start, end, sliceInterval); }

    void calculate(bool split = true)
    {
        const int K = chains.size(), dt = Device::HipDtype<ParamType>::value;
        assert(K >= 1);
        const std::size_t P = static_cast<std::size_t>(pCount);
        rhat.assign(P, 0.0);
        mean.assign(P, 0.0);
        within.assign(P, 0.0);
        between.assign(P, 0.0);
        chainMean.assign(K * P, 0.0);
        chainWithin.assign(K * P, 0.0);
        if (!chains.anyDevice())
        {
            check("mcmcpp_hip_gelman_rubin",
                  mcmcpp_hip_gelman_rubin(dt, -1, chains.hostPointers(), K, chains.used(), wCount, pCount, split ? 1 : 0, rhat.data(), mean.data(), within.data(),
                                          between.data(), chainMean.data(), chainWithin.data(), NULL, NULL, &seqLength, &seqCount));
            return;
        }
        // chains in device memory, each an allocation of its own: the sequences of every chain where it lies, then the M x P
        // sequence figures combined by the rules of include/mcmcpp_hip.h
        const int H = split ? 2 : 1;
        const std::size_t perChain = static_cast<std::size_t>(H) * wCount * P;
        std::vector<double> seqMean(K * perChain), seqM2(K * perChain);
        for (int k = 0; k < K; ++k)
        {
            const typename Detail::ChainSet<ParamType>::ChainSteps& c = chains.chain(k);
            std::int64_t count = 0;
            // (a single chain of one walker, unsplit, has one sequence and is refused; so it is for K such chains)
            if (c.onDevice)
                check("mcmcpp_hip_gelman_rubin_device",
                      mcmcpp_hip_gelman_rubin_device(dt, -1, c.span.first, 1, 0, c.span.steps, c.slice, wCount, pCount, split ? 1 : 0, NULL, NULL, NULL, NULL, NULL,
                                                     NULL, &seqMean[k * perChain], &seqM2[k * perChain], &seqLength, &count));
            else
                check("mcmcpp_hip_gelman_rubin",
                      mcmcpp_hip_gelman_rubin(dt, -1, c.steps.empty() ? NULL : c.steps.data(), 1, c.used, wCount, pCount, split ? 1 : 0, NULL, NULL, NULL, NULL, NULL,
                                              NULL, &seqMean[k * perChain], &seqM2[k * perChain], &seqLength, &count));
        }
        seqCount = static_cast<std::int64_t>(K) * H * wCount;
        combine(seqMean, seqM2, K, H);
    }

    double getRhat(int pNum) const { return rhat[pNum]; }
    double getMean(int pNum) const { return mean[pNum]; }
    double getWithin(int pNum) const { return within[pNum]; }
    double getBetween(int pNum) const { return between[pNum]; }
    double getChainMean(int chain, int pNum) const { return chainMean[static_cast<std::size_t>(chain) * pCount + pNum]; }
    double getChainWithin(int chain, int pNum) const { return chainWithin[static_cast<std::size_t>(chain) * pCount + pNum]; }
    long long getSequenceLength() const { return seqLength; }
    long long getNumSequences() const { return seqCount; }

private:
    /// sum_fixed of include/mcmcpp_hip.h over f(m), m in [m0, m0 + N): slices of max(1024, ceil(N / 64) rounded up to 64) terms,
    /// each summed in ascending order from +0, the slice sums added in ascending order
    template <class F>
    static double sumFixed(std::int64_t m0, std::int64_t N, F f)
    {
        std::int64_t per = ((N + 63) / 64 + 63) / 64 * 64;
        if (per < 1024) per = 1024;
        volatile double total = 0.0;  // (volatile: every addition rounded to double, whatever the compiler's flags)
        for (std::int64_t b = 0; b < N; b += per)
        {
            volatile double acc = 0.0;
            for (std::int64_t m = b; m < N && m < b + per; ++m) acc = acc + f(m0 + m);
            total = b == 0 ? acc : total + acc;
        }
        return total;
    }

    struct Column
    {
        const std::vector<double>* v;
        std::size_t P, p;
        double scale, center;
        bool square;
        double operator()(std::int64_t m) const
        {
            volatile double x = (*v)[static_cast<std::size_t>(m) * P + p];
            if (square)
            {
                x = x - center;
                x = x * x;
                return x;
            }
            x = x / scale;
            return x;
        }
    };

    void combine(const std::vector<double>& seqMean, const std::vector<double>& seqM2, int K, int H)
    {
        const std::size_t P = static_cast<std::size_t>(pCount);
        const std::int64_t M = seqCount, perChain = static_cast<std::int64_t>(H) * wCount;
        const double L = static_cast<double>(seqLength), Lm1 = static_cast<double>(seqLength - 1);
        for (std::size_t p = 0; p < P; ++p)
        {
            const Column means = {&seqMean, P, p, 1.0, 0.0, false}, vars = {&seqM2, P, p, Lm1, 0.0, false};
            volatile double w = sumFixed(0, M, vars) / static_cast<double>(M);
            volatile double mu = sumFixed(0, M, means) / static_cast<double>(M);
            const Column dev = {&seqMean, P, p, 1.0, mu, true};
            volatile double b = sumFixed(0, M, dev) / static_cast<double>(M - 1);
            volatile double varplus = w * Lm1;
            varplus = varplus / L;
            varplus = varplus + b;
            varplus = varplus / w;
            within[p] = w;
            mean[p] = mu;
            between[p] = b;
            rhat[p] = std::sqrt(varplus);
            for (int k = 0; k < K; ++k)
            {
                chainMean[k * P + p] = sumFixed(k * perChain, perChain, means) / static_cast<double>(perChain);
                chainWithin[k * P + p] = sumFixed(k * perChain, perChain, vars) / static_cast<double>(perChain);
            }
        }
    }

    static void check(const char* what, int rc)
    {
        if (rc != MCMCPP_HIP_OK) Detail::ChainSet<ParamType>::fail(what, rc, mcmcpp_hip_gelman_rubin_last_error());
    }

    int pCount;
    int wCount;
    Detail::ChainSet<ParamType> chains;
    std::int64_t seqLength;
    std::int64_t seqCount;
    std::vector<double> rhat, mean, within, between;  ///< [P]
    std::vector<double> chainMean, chainWithin;       ///< [K][P]
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_GELMANRUBIN_H
