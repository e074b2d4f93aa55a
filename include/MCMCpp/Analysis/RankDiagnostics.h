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
#include "Detail/ChainSet.h"

namespace MCMC
{
namespace Analysis
{
template <class ParamType>
class RankDiagnostics
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    RankDiagnostics(int numParams, int numWalkers) : pCount(numParams), wCount(numWalkers), chains(numParams, numWalkers), seqLength(0), seqCount(0)
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
        for (int i = 0; i < kDoubles; ++i) values[i].assign(P, 0.0);
        closedBulk.assign(P, 0);
        closedTail.assign(P, 0);
        if (chains.sameSpans())
        {
            int rc;
            {
                const typename Detail::ChainSet<ParamType>::DeviceSource src(chains);  // one chain where it lies, several gathered
                rc = mcmcpp_hip_rank_diagnostics_device(dt, -1, src.first, K, 0, src.steps, src.slice, wCount, pCount, split ? 1 : 0, maxLag, values[0].data(), values[1].data(),
                                                        values[2].data(), values[3].data(), values[4].data(), values[5].data(), values[6].data(), values[7].data(),
                                                        values[8].data(), values[9].data(), closedBulk.data(), closedTail.data(), &seqLength, &seqCount);
            }
            if (rc != MCMCPP_HIP_OK) chains.fail("mcmcpp_hip_rank_diagnostics_device", rc, mcmcpp_hip_rank_diagnostics_last_error());
            return;
        }
        const void* const* all = chains.hostPointers();
        const int rc = mcmcpp_hip_rank_diagnostics(dt, -1, all, K, chains.used(), wCount, pCount, split ? 1 : 0, maxLag, values[0].data(), values[1].data(), values[2].data(),
                                                   values[3].data(), values[4].data(), values[5].data(), values[6].data(), values[7].data(), values[8].data(),
                                                   values[9].data(), closedBulk.data(), closedTail.data(), &seqLength, &seqCount);
        if (rc != MCMCPP_HIP_OK) chains.fail("mcmcpp_hip_rank_diagnostics", rc, mcmcpp_hip_rank_diagnostics_last_error());
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
    enum { kDoubles = 10 };  ///< rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper, median, q05, q95
    int pCount;
    int wCount;
    Detail::ChainSet<ParamType> chains;
    std::int64_t seqLength;
    std::int64_t seqCount;
    std::vector<double> values[kDoubles];         ///< [P] each
    std::vector<std::int64_t> closedBulk, closedTail;  ///< [P]
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_RANKDIAGNOSTICS_H
