/*
 * Analysis/RankDiagnostics.h -- rank-normalised split R-hat, bulk-ESS and tail-ESS of every parameter over the chains of
 * several samplers, computed on the MI355X: the convergence figures of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021)
 * that Stan, ArviZ and `posterior` report, over the same sequences as Analysis/GelmanRubin.h and Analysis/EffectiveSampleSize.h.
 *
 * An EXTENSION: not in the reference.  The raw-value R-hat and ESS of the two classes above miss chains that differ in scale
 * only and say nothing of the tails; on skewed targets these are the figures to read.
 *
 *     MCMC::Analysis::RankDiagnostics<double> rd(numParams, numWalkers);
 *     rd.addChain(samplerA.getStepIttBegin(), samplerA.getStepIttEnd(), sliceInterval);   // once per chain, the same number
 *     rd.addChain(samplerB.getStepIttBegin(), samplerB.getStepIttEnd(), sliceInterval);   // of steps in each
 *     rd.calculate();                    // split = true, maxLag = 0: the windows may reach lag L - 1
 *     rd.getRhat(p);  rd.getRhatRank(p);  rd.getRhatFolded(p);          // rhat = the larger of the two
 *     rd.getEssBulk(p);  rd.getEssTail(p);  rd.getEssTailLower(p);  rd.getEssTailUpper(p);
 *     rd.getMedian(p);  rd.getQ05(p);  rd.getQ95(p);  rd.bulkWindowClosed(p);  rd.tailWindowsClosed(p);
 *     rd.getSequenceLength();  rd.getNumSequences();
 *
 * Every draw of a parameter is ranked among all of them (average ranks for ties, which an ensemble sampler makes whenever it
 * rejects a move), the rank becomes a normal score, and the existing estimators run on the scores: include/mcmcpp_hip.h
 * (mcmcpp_hip_normal_scores, mcmcpp_hip_rank_diagnostics) has the definition to the last rounding.
 *
 * Host chains go to the library in one call through their step pointers.  One device chain (MCMCPP_CHAIN_MEMORY=device) is
 * read where it lies; several are gathered, device to device, into one allocation that the call then reads.  With
 * MCMCPP_DEVICE_ANALYSIS=0, or where only some chains are device chains, the selected steps are downloaded instead.  No GPU, no
 * result: failures abort with the library's message, like everything else in this facade.
 */
#ifndef MCMCPP_ANALYSIS_RANKDIAGNOSTICS_H
#define MCMCPP_ANALYSIS_RANKDIAGNOSTICS_H

#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../Chain/ChainStepIterator.h"
#include "../Device/HipBackend.h"
#include "Detail/DeviceSpan.h"

namespace MCMC
{
namespace Analysis
{
template <class ParamType>
class RankDiagnostics
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    RankDiagnostics(int numParams, int numWalkers) : pCount(numParams), wCount(numWalkers), used(0), seqLength(0), seqCount(0)
    {
        assert(pCount > 0);
        assert(wCount > 0);
    }

    /// One chain: every sliceInterval'th step of [start, end), beginning with `start`.  Every chain must give the same number
    /// of used steps.
    void addChain(IttType start, IttType end, int sliceInterval)
    {
        assert(sliceInterval >= 1);
        chains.push_back(ChainSteps(start, end));
        ChainSteps& c = chains.back();
        c.slice = sliceInterval;
        if (Detail::deviceSpan(start, end, &c.span) && c.span.steps > 0)
        {
            c.onDevice = true;
            c.used = (c.span.steps + sliceInterval - 1) / sliceInterval;
        }
        else
            hostSteps(c);
        assert(chains.size() == 1 || c.used == chains.front().used);
        used = c.used;
    }

    void calculate(bool split = true, long long maxLag = 0)
    {
        const int K = static_cast<int>(chains.size()), dt = Device::HipDtype<ParamType>::value;
        assert(K >= 1);
        const std::size_t P = static_cast<std::size_t>(pCount);
        for (int i = 0; i < kDoubles; ++i) values[i].assign(P, 0.0);
        closedBulk.assign(P, 0);
        closedTail.assign(P, 0);
        int onDevice = 0;
        for (int k = 0; k < K; ++k) onDevice += chains[k].onDevice ? 1 : 0;
        bool sameSpans = onDevice == K;
        for (int k = 1; k < K && sameSpans; ++k) sameSpans = chains[k].span.steps == chains[0].span.steps && chains[k].slice == chains[0].slice;
        if (sameSpans)
        {
            // one chain is read where it lies; several are gathered into one allocation, chain behind chain
            const std::int64_t steps = chains[0].span.steps;
            const std::uint64_t chainBytes = static_cast<std::uint64_t>(steps) * wCount * P * sizeof(ParamType);
            const void* first = chains[0].span.first;
            void* gathered = NULL;
            if (K > 1)
            {
                gathered = mcmcpp_hip_device_alloc(-1, chainBytes * K);
                if (!gathered) fail("mcmcpp_hip_device_alloc", MCMCPP_HIP_E_NOMEM, mcmcpp_hip_device_chain_last_error());
                for (int k = 0; k < K; ++k)
                {
                    const int rc = mcmcpp_hip_device_copy(static_cast<char*>(gathered) + chainBytes * k, chains[k].span.first, chainBytes);
                    if (rc != MCMCPP_HIP_OK) fail("mcmcpp_hip_device_copy", rc, mcmcpp_hip_device_chain_last_error());
                }
                first = gathered;
            }
            const int rc = mcmcpp_hip_rank_diagnostics_device(dt, -1, first, K, 0, steps, chains[0].slice, wCount, pCount, split ? 1 : 0, maxLag, values[0].data(),
                                                              values[1].data(), values[2].data(), values[3].data(), values[4].data(), values[5].data(), values[6].data(),
                                                              values[7].data(), values[8].data(), values[9].data(), closedBulk.data(), closedTail.data(), &seqLength,
                                                              &seqCount);
            mcmcpp_hip_device_free(gathered);
            if (rc != MCMCPP_HIP_OK) fail("mcmcpp_hip_rank_diagnostics_device", rc, mcmcpp_hip_rank_diagnostics_last_error());
            return;
        }
        std::vector<const void*> all;
        for (int k = 0; k < K; ++k)
        {
            if (chains[k].onDevice)
            {
                chains[k].onDevice = false;
                chains[k].used = Detail::downloadSteps(chains[k].start, chains[k].end, chains[k].slice, chains[k].staging);
                stagingPointers(chains[k]);
            }
            all.insert(all.end(), chains[k].steps.begin(), chains[k].steps.end());
        }
        const int rc = mcmcpp_hip_rank_diagnostics(dt, -1, all.empty() ? NULL : all.data(), K, used, wCount, pCount, split ? 1 : 0, maxLag, values[0].data(),
                                                   values[1].data(), values[2].data(), values[3].data(), values[4].data(), values[5].data(), values[6].data(),
                                                   values[7].data(), values[8].data(), values[9].data(), closedBulk.data(), closedTail.data(), &seqLength, &seqCount);
        if (rc != MCMCPP_HIP_OK) fail("mcmcpp_hip_rank_diagnostics", rc, mcmcpp_hip_rank_diagnostics_last_error());
    }

    double getRhat(int pNum) const { return values[0][pNum]; }
    double getRhatRank(int pNum) const { return values[1][pNum]; }
    double getRhatFolded(int pNum) const { return values[2][pNum]; }
    double getEssBulk(int pNum) const { return values[3][pNum]; }
    double getEssTail(int pNum) const { return values[4][pNum]; }
    double getEssTailLower(int pNum) const { return values[5][pNum]; }
    double getEssTailUpper(int pNum) const { return values[6][pNum]; }
    double getMedian(int pNum) const { return values[7][pNum]; }
    double getQ05(int pNum) const { return values[8][pNum]; }
    double getQ95(int pNum) const { return values[9][pNum]; }
    bool bulkWindowClosed(int pNum) const { return closedBulk[pNum] != 0; }
    bool tailWindowsClosed(int pNum) const { return closedTail[pNum] != 0; }
    long long getSequenceLength() const { return seqLength; }
    long long getNumSequences() const { return seqCount; }

private:
    struct ChainSteps
    {
        ChainSteps(const IttType& s, const IttType& e) : onDevice(false), used(0), slice(1), start(s), end(e)
        {
            span.first = NULL;
            span.steps = 0;
        }
        bool onDevice;
        std::int64_t used;
        int slice;
        IttType start, end;
        Detail::DeviceSpan<ParamType> span;
        std::vector<const void*> steps;
        std::vector<ParamType> staging;
    };

    void stagingPointers(ChainSteps& c) const
    {
        c.steps.clear();
        for (std::int64_t k = 0; k < c.used; ++k) c.steps.push_back(c.staging.data() + static_cast<std::size_t>(k) * wCount * pCount);
    }

    /// the used steps of a chain that is read through host pointers
    void hostSteps(ChainSteps& c) const
    {
        if (!Detail::pointersStay(c.start))
        {
            c.used = Detail::downloadSteps(c.start, c.end, c.slice, c.staging);
            stagingPointers(c);
            return;
        }
        long long index = 0;
        for (IttType itt(c.start); itt != c.end; ++itt, ++index)
            if (index % c.slice == 0) c.steps.push_back(*itt);
        c.used = static_cast<std::int64_t>(c.steps.size());
    }

    static void fail(const char* what, int rc, const char* msg)
    {
        std::fprintf(stderr, "MCMCpp (MI355X): %s failed with code %d: %s\n", what, rc, msg ? msg : "");
        std::abort();
    }

    enum { kDoubles = 10 };  ///< rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper, median, q05, q95
    int pCount;
    int wCount;
    std::int64_t used;
    std::int64_t seqLength;
    std::int64_t seqCount;
    std::vector<ChainSteps> chains;
    std::vector<double> values[kDoubles];         ///< [P] each
    std::vector<std::int64_t> closedBulk, closedTail;  ///< [P]
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_RANKDIAGNOSTICS_H
