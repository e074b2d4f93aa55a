/*
 * Analysis/PosteriorSummary.h -- the summary row of every parameter over the chains of several samplers, computed on the
 * MI355X: mean, sd, quantiles and a highest-density interval, each with its Monte Carlo standard error and effective sample
 * size (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021, section 4), over the same sequences as Analysis/RankDiagnostics.h.
 * The row Stan, `posterior` and ArviZ print; the standard error says how many digits of a reported figure are real.
 *
 * An EXTENSION: not in the reference.
 *
 *     MCMC::Analysis::PosteriorSummary<double> ps(numParams, numWalkers);
 *     ps.addChain(samplerA.getStepIttBegin(), samplerA.getStepIttEnd(), sliceInterval);   // once per chain, the same number
 *     ps.addChain(samplerB.getStepIttBegin(), samplerB.getStepIttEnd(), sliceInterval);   // of steps in each
 *     ps.calculate();                    // quantiles 0.05, 0.5, 0.95 and the 94 % interval; split = true, maxLag = 0
 *     ps.getMean(p);  ps.getMcseMean(p);  ps.getSd(p);  ps.getMcseSd(p);  ps.getEssMean(p);  ps.getEssSd(p);
 *     ps.getQuantile(p, i);  ps.getMcseQuantile(p, i);  ps.getEssQuantile(p, i);  ps.getHdiLower(p);  ps.getHdiUpper(p);
 *     ps.writeTable(std::cout);
 *
 * include/mcmcpp_hip.h (mcmcpp_hip_posterior_summary) has the definition to the last rounding.
 *
 * Host chains go to the library in one call through their step pointers.  One device chain (MCMCPP_CHAIN_MEMORY=device) is
 * read where it lies; several are gathered, device to device, into one allocation that the call then reads.  With
 * MCMCPP_DEVICE_ANALYSIS=0, or where only some chains are device chains, the selected steps are downloaded instead.  No GPU, no
 * result: failures abort with the library's message, like everything else in this facade.
 */
#ifndef MCMCPP_ANALYSIS_POSTERIORSUMMARY_H
#define MCMCPP_ANALYSIS_POSTERIORSUMMARY_H

#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <ostream>
#include <vector>

#include "../Chain/ChainStepIterator.h"
#include "../Device/HipBackend.h"
#include "Detail/ChainSet.h"

namespace MCMC
{
namespace Analysis
{
template <class ParamType>
class PosteriorSummary
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    PosteriorSummary(int numParams, int numWalkers) : pCount(numParams), wCount(numWalkers), chains(numParams, numWalkers), seqLength(0), seqCount(0), hdiProb(0.0)
    {
        assert(pCount > 0);
        assert(wCount > 0);
    }

    /// One chain: every sliceInterval'th step of [start, end), beginning with `start`.  Every chain must give the same number
    /// of used steps.
    void addChain(IttType start, IttType end, int sliceInterval) { chains.addChain(start, end, sliceInterval); }

    /// The quantiles 0.05, 0.5 and 0.95 and the 94 % highest-density interval
    void calculate(bool split = true, long long maxLag = 0)
    {
        const double defaults[3] = {0.05, 0.5, 0.95};
        calculate(std::vector<double>(defaults, defaults + 3), 0.94, split, maxLag);
    }

    /// quantileProbs: up to 16 probabilities inside (0, 1).  hdiProbability: 0 for no interval.
    void calculate(const std::vector<double>& quantileProbs, double hdiProbability, bool split = true, long long maxLag = 0)
    {
        const int K = chains.size(), dt = Device::HipDtype<ParamType>::value, Q = static_cast<int>(quantileProbs.size());
        assert(K >= 1);
        probs = quantileProbs;
        hdiProb = hdiProbability;
        const std::size_t P = static_cast<std::size_t>(pCount);
        for (int i = 0; i < kPerParam; ++i) values[i].assign(P, 0.0);
        for (int i = 0; i < kPerQuantile; ++i) tables[i].assign(P * Q, 0.0);
        rankLower.assign(P * Q, 0);
        rankUpper.assign(P * Q, 0);
        const double* pr = Q ? probs.data() : NULL;
        if (chains.sameSpans())
        {
            int rc;
            {
                const typename Detail::ChainSet<ParamType>::DeviceSource src(chains);  // one chain where it lies, several gathered
                rc = mcmcpp_hip_posterior_summary_device(dt, -1, src.first, K, 0, src.steps, src.slice, wCount, pCount, split ? 1 : 0, maxLag, pr, Q, hdiProb, values[0].data(),
                                                         values[1].data(), values[2].data(), values[3].data(), values[4].data(), values[5].data(), tables[0].data(),
                                                         tables[1].data(), tables[2].data(), rankLower.data(), rankUpper.data(), values[6].data(), values[7].data(),
                                                         &seqLength, &seqCount);
            }
            if (rc != MCMCPP_HIP_OK) chains.fail("mcmcpp_hip_posterior_summary_device", rc, mcmcpp_hip_posterior_summary_last_error());
            return;
        }
        const void* const* all = chains.hostPointers();
        const int rc = mcmcpp_hip_posterior_summary(dt, -1, all, K, chains.used(), wCount, pCount, split ? 1 : 0, maxLag, pr, Q, hdiProb, values[0].data(), values[1].data(),
                                                    values[2].data(), values[3].data(), values[4].data(), values[5].data(), tables[0].data(), tables[1].data(),
                                                    tables[2].data(), rankLower.data(), rankUpper.data(), values[6].data(), values[7].data(), &seqLength, &seqCount);
        if (rc != MCMCPP_HIP_OK) chains.fail("mcmcpp_hip_posterior_summary", rc, mcmcpp_hip_posterior_summary_last_error());
    }

    double getMean(int pNum) const { return values[0][pNum]; }
    double getSd(int pNum) const { return values[1][pNum]; }
    double getMcseMean(int pNum) const { return values[2][pNum]; }
    double getEssMean(int pNum) const { return values[3][pNum]; }
    double getEssSd(int pNum) const { return values[4][pNum]; }
    double getMcseSd(int pNum) const { return values[5][pNum]; }
    double getHdiLower(int pNum) const { return values[6][pNum]; }  ///< (0 where no interval was asked for)
    double getHdiUpper(int pNum) const { return values[7][pNum]; }
    int getNumQuantiles() const { return static_cast<int>(probs.size()); }
    double getQuantileProb(int i) const { return probs[i]; }
    double getHdiProb() const { return hdiProb; }
    double getQuantile(int pNum, int i) const { return tables[0][at(pNum, i)]; }
    double getEssQuantile(int pNum, int i) const { return tables[1][at(pNum, i)]; }
    double getMcseQuantile(int pNum, int i) const { return tables[2][at(pNum, i)]; }
    long long getMcseRankLower(int pNum, int i) const { return rankLower[at(pNum, i)]; }
    long long getMcseRankUpper(int pNum, int i) const { return rankUpper[at(pNum, i)]; }
    long long getSequenceLength() const { return seqLength; }
    long long getNumSequences() const { return seqCount; }

    /// One row per parameter: mean, its standard error, sd, its standard error, every quantile with its standard error, the
    /// interval, and the effective sample sizes of the mean and of the sd
    void writeTable(std::ostream& out) const
    {
        const int Q = getNumQuantiles();
        out << "param |         mean  mcse_mean |           sd    mcse_sd |";
        for (int i = 0; i < Q; ++i) out << "      q" << std::setw(6) << std::left << probs[i] << std::right << "       mcse |";
        if (hdiProb != 0.0) out << " hdi " << std::setw(5) << std::left << hdiProb << std::right << "  lower        upper |";
        out << " ess_mean   ess_sd\n";
        for (int p = 0; p < pCount; ++p)
        {
            out << "P" << std::setw(4) << std::left << p << std::right << " | " << std::setprecision(6) << std::setw(12) << getMean(p) << " " << std::setw(10) << getMcseMean(p)
                << " | " << std::setw(12) << getSd(p) << " " << std::setw(10) << getMcseSd(p) << " |";
            for (int i = 0; i < Q; ++i) out << " " << std::setw(12) << getQuantile(p, i) << " " << std::setw(10) << getMcseQuantile(p, i) << " |";
            if (hdiProb != 0.0) out << " " << std::setw(12) << getHdiLower(p) << " " << std::setw(12) << getHdiUpper(p) << " |";
            out << " " << std::setprecision(1) << std::fixed << std::setw(8) << getEssMean(p) << " " << std::setw(8) << getEssSd(p) << "\n";
            out.unsetf(std::ios_base::floatfield);
        }
    }

private:
    std::size_t at(int pNum, int i) const { return static_cast<std::size_t>(pNum) * probs.size() + i; }

    enum { kPerParam = 8, kPerQuantile = 3 };  ///< mean, sd, mcse_mean, ess_mean, ess_sd, mcse_sd, hdi_lower, hdi_upper; quantile, ess_quantile, mcse_quantile
    int pCount;
    int wCount;
    Detail::ChainSet<ParamType> chains;
    std::int64_t seqLength;
    std::int64_t seqCount;
    double hdiProb;
    std::vector<double> probs;
    std::vector<double> values[kPerParam];     ///< [P] each
    std::vector<double> tables[kPerQuantile];  ///< [P][Q] each
    std::vector<std::int64_t> rankLower, rankUpper;
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_POSTERIORSUMMARY_H
