/*
 * Analysis/ExactPercentiles.h -- exact percentiles of every parameter over the samples in a chain, and the exact percentile
 * of given values, selected and counted on the MI355X.
 *
 * An EXTENSION: not in the reference.  The reference's PercentileAndMaximumFinder interpolates inside one of its bins, reads
 * parameter 0's cumulative sums for every parameter and tweaks its upper bound the wrong way; this repository reproduces that
 * class bit for bit (PercentileAndMaximumFinder.h) and leaves it alone.  This class stands beside it:
 *
 *     MCMC::Analysis::ExactPercentiles<double> ep(numParams, numWalkers);
 *     ep.processChainData(sampler.getStepIttBegin(), sampler.getStepIttEnd(), sliceInterval, {2.5, 16.0, 50.0, 84.0, 97.5});
 *     ep.getValueFromPercentile(p, k);   // the k-th requested percentile of parameter p
 *     ep.getLowerValue(p, k);  ep.getHigherValue(p, k);  ep.getNumPoints();
 *     ep.processValues(begin, end, sliceInterval, values);   // values[p * K + k]: K values per parameter
 *     ep.getPercentileFromValue(p, k);  ep.getCountBelow(p, k);  ep.getCountNotAbove(p, k);
 *
 * With N samples of a parameter (steps used x walkers) and a percentile c: h = (c / 100) (N - 1) in double; getLowerValue is
 * the sample of rank floor(h) in the order -inf < ... < -0 < +0 < ... < +inf, getHigherValue the one of rank ceil(h), and
 * getValueFromPercentile is lower + (higher - lower) (h - floor(h)), computed in double and rounded once to ParamType (the
 * "linear" rule of numpy.quantile).  getPercentileFromValue is ParamType(100) * ParamType(count below) / ParamType(N).
 * The samples are selected by libmcmcpp_hip.so (include/mcmcpp_hip.h, mcmcpp_hip_order_statistics / _rank_counts): integer
 * counts only, so every figure is exact.  The steps of a device chain (MCMCPP_CHAIN_MEMORY=device) are read where they lie;
 * no step comes to the host.  No GPU, no result: failures abort with the library's message, like everything else in this
 * facade.
 */
#ifndef MCMCPP_ANALYSIS_EXACTPERCENTILES_H
#define MCMCPP_ANALYSIS_EXACTPERCENTILES_H

#include <cassert>
#include <cmath>
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
class ExactPercentiles
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    ExactPercentiles(int numParams, int numWalkers) : pCount(numParams), wCount(numWalkers), numPoints(0), perCount(0), valCount(0)
    {
        assert(pCount > 0);
        assert(wCount > 0);
    }

    /// Selects the requested percentiles (each in [0, 100], at most 32) of every parameter over every sliceInterval'th step of
    /// [start, end), beginning with `start`.
    void processChainData(IttType start, IttType end, int sliceInterval, const std::vector<double>& percentiles)
    {
        Selection sel(start, end, sliceInterval, wCount, pCount);
        numPoints = sel.used * wCount;
        perCount = static_cast<int>(percentiles.size());
        assert(perCount >= 1 && 2 * perCount <= 64);
        std::vector<std::int64_t> ranks(2 * static_cast<std::size_t>(perCount));
        fraction.assign(perCount, 0.0);
        for (int k = 0; k < perCount; ++k)
        {
            assert(percentiles[k] >= 0.0 && percentiles[k] <= 100.0);
            const double h = (percentiles[k] / 100.0) * static_cast<double>(numPoints - 1);
            ranks[k] = static_cast<std::int64_t>(std::floor(h));
            ranks[perCount + k] = static_cast<std::int64_t>(std::ceil(h));
            fraction[k] = h - std::floor(h);
        }
        selected.assign(static_cast<std::size_t>(pCount) * 2 * perCount, ParamType(0));
        const int dt = Device::HipDtype<ParamType>::value, n = 2 * perCount;
        if (sel.onDevice)
            check("mcmcpp_hip_order_statistics_device",
                  mcmcpp_hip_order_statistics_device(dt, -1, sel.span.first, sel.span.steps, sliceInterval, wCount, pCount, ranks.data(), n, selected.data()));
        else
            check("mcmcpp_hip_order_statistics", mcmcpp_hip_order_statistics(dt, -1, sel.pointers(), sel.used, wCount, pCount, ranks.data(), n, selected.data()));
    }

    ParamType getLowerValue(int pNum, int k) const { return selected[static_cast<std::size_t>(pNum) * 2 * perCount + k]; }
    ParamType getHigherValue(int pNum, int k) const { return selected[static_cast<std::size_t>(pNum) * 2 * perCount + perCount + k]; }
    ParamType getValueFromPercentile(int pNum, int k) const
    {
        const ParamType lower = getLowerValue(pNum, k), higher = getHigherValue(pNum, k);
        if (lower == higher) return lower;  // (also where both are infinite)
        const double lo = static_cast<double>(lower), hi = static_cast<double>(higher);
        return static_cast<ParamType>(lo + (hi - lo) * fraction[k]);
    }
    /// samples of one parameter used by the last processChainData / processValues
    long long getNumPoints() const { return numPoints; }

    /// Counts, for the K = values.size() / numParams values of every parameter (values[p * K + k]), the samples below and the
    /// samples not above each, over the same selection of steps.
    void processValues(IttType start, IttType end, int sliceInterval, const std::vector<ParamType>& values)
    {
        Selection sel(start, end, sliceInterval, wCount, pCount);
        numPoints = sel.used * wCount;
        valCount = static_cast<int>(values.size() / static_cast<std::size_t>(pCount));
        assert(valCount >= 1 && values.size() == static_cast<std::size_t>(valCount) * pCount);
        below.assign(values.size(), 0);
        notAbove.assign(values.size(), 0);
        const int dt = Device::HipDtype<ParamType>::value;
        if (sel.onDevice)
            check("mcmcpp_hip_rank_counts_device", mcmcpp_hip_rank_counts_device(dt, -1, sel.span.first, sel.span.steps, sliceInterval, wCount, pCount,
                                                                                 values.data(), valCount, below.data(), notAbove.data()));
        else
            check("mcmcpp_hip_rank_counts",
                  mcmcpp_hip_rank_counts(dt, -1, sel.pointers(), sel.used, wCount, pCount, values.data(), valCount, below.data(), notAbove.data()));
    }

    long long getCountBelow(int pNum, int k) const { return below[static_cast<std::size_t>(pNum) * valCount + k]; }
    long long getCountNotAbove(int pNum, int k) const { return notAbove[static_cast<std::size_t>(pNum) * valCount + k]; }
    ParamType getPercentileFromValue(int pNum, int k) const
    {
        return static_cast<ParamType>(100) * static_cast<ParamType>(getCountBelow(pNum, k)) / static_cast<ParamType>(numPoints);
    }

private:
    /// The steps the other analysis classes' loops would use: a span of a device chain, or host pointers (for a device chain
    /// with MCMCPP_DEVICE_ANALYSIS=0, to copies of the selected steps).
    struct Selection
    {
        Selection(IttType start, IttType end, int sliceInterval, int wCount, int pCount) : onDevice(false), used(0)
        {
            assert(sliceInterval >= 1);
            if (Detail::deviceSpan(start, end, &span) && span.steps > 0)
            {
                onDevice = true;
                used = (span.steps + sliceInterval - 1) / sliceInterval;
            }
            else if (!Detail::pointersStay(start))
            {
                used = Detail::downloadSteps(start, end, sliceInterval, staging);
                for (std::int64_t k = 0; k < used; ++k) steps.push_back(staging.data() + static_cast<std::size_t>(k) * wCount * pCount);
            }
            else
            {
                long long index = 0;
                for (IttType itt(start); itt != end; ++itt, ++index)
                    if (index % sliceInterval == 0) steps.push_back(*itt);
                used = static_cast<std::int64_t>(steps.size());
            }
        }
        const void* const* pointers() const { return steps.empty() ? nullptr : steps.data(); }

        bool onDevice;
        std::int64_t used;
        Detail::DeviceSpan<ParamType> span;
        std::vector<const void*> steps;
        std::vector<ParamType> staging;
    };

    static void check(const char* what, int rc)
    {
        if (rc == MCMCPP_HIP_OK) return;
        const char* msg = mcmcpp_hip_order_statistics_last_error();
        std::fprintf(stderr, "MCMCpp (MI355X): %s failed with code %d: %s\n", what, rc, msg ? msg : "");
        std::abort();
    }

    int pCount;
    int wCount;
    long long numPoints;
    int perCount;
    int valCount;
    std::vector<double> fraction;          ///< [K]: h - floor(h) of every requested percentile
    std::vector<ParamType> selected;       ///< [P][2K]: the order statistics of ranks floor(h), then of ranks ceil(h)
    std::vector<std::int64_t> below;       ///< [P][K]
    std::vector<std::int64_t> notAbove;    ///< [P][K]
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_EXACTPERCENTILES_H
