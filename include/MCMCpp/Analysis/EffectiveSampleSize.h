/*
 * Analysis/EffectiveSampleSize.h -- the effective sample size and the integrated autocorrelation time of every parameter over
 * the chains of several samplers, computed on the MI355X: how many independent draws are the chains worth?  The multi-sequence
 * estimator of BDA3 / Stan that goes with the split R-hat of Analysis/GelmanRubin.h, over the same sequences.
 *
 * An EXTENSION: not in the reference, whose AutoCorrCalc takes one pooled chain and knows nothing of the between-chain
 * variance, so that it reports a short time for chains that have not mixed.
 *
 *     MCMC::Analysis::EffectiveSampleSize<double> ess(numParams, numWalkers);
 *     ess.addChain(samplerA.getStepIttBegin(), samplerA.getStepIttEnd(), sliceInterval);   // once per chain, the same number
 *     ess.addChain(samplerB.getStepIttBegin(), samplerB.getStepIttEnd(), sliceInterval);   // of steps in each
 *     ess.calculate();                   // split = true, maxLag = 0: the window may reach lag L - 1
 *     ess.getEss(p);  ess.getTau(p);  ess.getLagsUsed(p);  ess.windowClosed(p);
 *     ess.getRhat(p);  ess.getMean(p);  ess.getWithin(p);  ess.getBetween(p);
 *     ess.getSequenceLength();  ess.getNumSequences();
 *
 * Every walker of every chain is a sequence (two with split), M = K H W sequences of L steps, as in GelmanRubin.h.  The
 * autocovariance at lag t is the mean over the sequences of their own lagged products around their own means,
 * rho_t = 1 - (within - gamma_t) / varplus, and tau = -1 + 2 (sum of the pairs rho_2k + rho_2k+1 by Geyer's initial monotone
 * sequence rule), not below 1 / log10(M L); ess = M L / tau.  include/mcmcpp_hip.h (mcmcpp_hip_effective_sample_size) has the
 * definition to the last rounding: a figure is a function of the samples alone, wherever the chains lie.
 *
 * Host chains go to the library in one call through their step pointers.  One device chain (MCMCPP_CHAIN_MEMORY=device) is
 * read where it lies.  Several device chains are allocations of their own, and the sum over the sequences spans all of them:
 * they are gathered, device to device, into one allocation that the call then reads; no step comes to the host.  With
 * MCMCPP_DEVICE_ANALYSIS=0, or where only some chains are device chains, the selected steps are downloaded instead.  No GPU, no
 * result: failures abort with the library's message, like everything else in this facade.
 */
#ifndef MCMCPP_ANALYSIS_EFFECTIVESAMPLESIZE_H
#define MCMCPP_ANALYSIS_EFFECTIVESAMPLESIZE_H

#include <cassert>
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
class EffectiveSampleSize
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    EffectiveSampleSize(int numParams, int numWalkers) : pCount(numParams), wCount(numWalkers), chains(numParams, numWalkers), seqLength(0), seqCount(0)
    {
        assert(pCount > 0);
        assert(wCount > 0);
    }

    /// One chain: every sliceInterval'th step of [start, end), beginning with `start`.  Every chain must give the same number
    /// of used steps.
    void addChain(IttType start, IttType end, int sliceInterval) { chains.addChain(start, end, sliceInterval); }

    void calculate(bool split = true, long long maxLag = 0)
    {
        const int K = chains.size(), dt = Device::HipDtype<ParamType>::value;
        assert(K >= 1);
        const std::size_t P = static_cast<std::size_t>(pCount);
        ess.assign(P, 0.0);
        tau.assign(P, 0.0);
        lagsUsed.assign(P, 0);
        closed.assign(P, 0);
        rhat.assign(P, 0.0);
        mean.assign(P, 0.0);
        within.assign(P, 0.0);
        between.assign(P, 0.0);
        if (chains.sameSpans())
        {
            int rc;
            {
                const typename Detail::ChainSet<ParamType>::DeviceSource src(chains);  // one chain where it lies, several gathered
                rc = mcmcpp_hip_effective_sample_size_device(dt, -1, src.first, K, 0, src.steps, src.slice, wCount, pCount, split ? 1 : 0, maxLag, 0, ess.data(), tau.data(),
                                                             lagsUsed.data(), closed.data(), NULL, NULL, rhat.data(), mean.data(), within.data(), between.data(),
                                                             &seqLength, &seqCount);
            }
            if (rc != MCMCPP_HIP_OK) chains.fail("mcmcpp_hip_effective_sample_size_device", rc, mcmcpp_hip_effective_sample_size_last_error());
            return;
        }
        const void* const* all = chains.hostPointers();
        const int rc = mcmcpp_hip_effective_sample_size(dt, -1, all, K, chains.used(), wCount, pCount, split ? 1 : 0, maxLag, 0, ess.data(), tau.data(), lagsUsed.data(),
                                                        closed.data(), NULL, NULL, rhat.data(), mean.data(), within.data(), between.data(), &seqLength, &seqCount);
        if (rc != MCMCPP_HIP_OK) chains.fail("mcmcpp_hip_effective_sample_size", rc, mcmcpp_hip_effective_sample_size_last_error());
    }

    double getEss(int pNum) const { return ess[pNum]; }
    double getTau(int pNum) const { return tau[pNum]; }
    long long getLagsUsed(int pNum) const { return lagsUsed[pNum]; }
    bool windowClosed(int pNum) const { return closed[pNum] != 0; }
    double getRhat(int pNum) const { return rhat[pNum]; }
    double getMean(int pNum) const { return mean[pNum]; }
    double getWithin(int pNum) const { return within[pNum]; }
    double getBetween(int pNum) const { return between[pNum]; }
    long long getSequenceLength() const { return seqLength; }
    long long getNumSequences() const { return seqCount; }

private:
    int pCount;
    int wCount;
    Detail::ChainSet<ParamType> chains;
    std::int64_t seqLength;
    std::int64_t seqCount;
    std::vector<double> ess, tau, rhat, mean, within, between;  ///< [P]
    std::vector<std::int64_t> lagsUsed, closed;                 ///< [P]
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_EFFECTIVESAMPLESIZE_H
