/*
 * Analysis/Detail/DeviceHistograms.h -- what CornerHistograms and PercentileAndMaximumFinder share: the
 * mcmcpp_hip_histograms handle (include/mcmcpp_hip.h), the selection of the steps the reference's loops use (every
 * sliceInterval'th step of [start, end), beginning with `start`), and the arrays the library returns.  The steps of a device
 * chain (MCMCPP_CHAIN_MEMORY=device) are counted where they lie (mcmcpp_hip_histograms_compute_device).  Not part of the
 * reference's API.
 */
#ifndef MCMCPP_ANALYSIS_DETAIL_DEVICEHISTOGRAMS_H
#define MCMCPP_ANALYSIS_DETAIL_DEVICEHISTOGRAMS_H

#include <cassert>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../Chain/ChainStepIterator.h"
#include "../../Device/HipBackend.h"
#include "DeviceSpan.h"

namespace MCMC
{
namespace Analysis
{
namespace Detail
{
/// static_cast<int>(v) as x86-64 computes it (INT_MIN for NaN and values outside int), without the undefined behaviour
template <class T>
inline int truncToInt(T v)
{
    const double d = static_cast<double>(v);
    if (!(d > -2147483649.0 && d < 2147483648.0)) return INT_MIN;
    return static_cast<int>(d);
}

template <class ParamType>
class DeviceHistograms
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    DeviceHistograms(int numParams, int numWalkers, int bins, bool withPairs)
        : pCount(numParams), wCount(numWalkers), bCount(bins), pairs(withPairs), numPoints(0),
          bounds(2 * static_cast<size_t>(numParams), ParamType(0)), single(static_cast<size_t>(numParams) * bins, 0),
          clamped(numParams, 0), handle(nullptr)
    {
        assert(pCount > 0);
        assert(wCount > 0);
        assert(bCount > 1);
        const int rc = mcmcpp_hip_histograms_create(Device::HipDtype<ParamType>::value, -1, wCount, pCount, bCount, withPairs ? 1 : 0, &handle);
        if (rc != MCMCPP_HIP_OK) die("mcmcpp_hip_histograms_create", rc, mcmcpp_hip_histograms_last_error(nullptr));
        if (withPairs) twoAxis.assign(static_cast<size_t>(pCount) * (pCount - 1) / 2 * bCount * bCount, 0);
    }
    ~DeviceHistograms()
    {
        if (handle) mcmcpp_hip_histograms_destroy(handle);
    }
    DeviceHistograms(const DeviceHistograms&) = delete;
    DeviceHistograms& operator=(const DeviceHistograms&) = delete;

    /// Counts the steps the reference's calculateHistograms / processChainData would use and fetches every result.
    void compute(IttType start, IttType end, int sliceInterval)
    {
        assert(sliceInterval >= 1);
        std::vector<const void*> steps;
        DeviceSpan<ParamType> span;
        if (deviceSpan(start, end, &span) && span.steps > 0)
            check("mcmcpp_hip_histograms_compute_device", mcmcpp_hip_histograms_compute_device(handle, span.first, span.steps, sliceInterval));
        else
        {
            std::vector<ParamType> staging;  // (a device chain with the device path switched off: copies of the steps used)
            if (!pointersStay(start))
            {
                const std::int64_t n = downloadSteps(start, end, sliceInterval, staging);
                for (std::int64_t k = 0; k < n; ++k) steps.push_back(staging.data() + static_cast<std::size_t>(k) * wCount * pCount);
            }
            else
            {
                long long index = 0;
                for (IttType itt(start); itt != end; ++itt, ++index)
                    if (index % sliceInterval == 0) steps.push_back(*itt);
            }
            check("mcmcpp_hip_histograms_compute",
                  mcmcpp_hip_histograms_compute(handle, steps.empty() ? nullptr : steps.data(), static_cast<std::int64_t>(steps.size())));
        }
        std::int64_t n = 0;
        check("mcmcpp_hip_histograms_result", mcmcpp_hip_histograms_result(handle, &n, bounds.data(), single.data(),
                                                                             pairs ? twoAxis.data() : nullptr, clamped.data()));
        numPoints = n;
    }

    int pCount;
    int wCount;
    int bCount;
    bool pairs;
    long long numPoints;
    std::vector<ParamType> bounds;       ///< [P][2]: low edge, bin width (the reference's paramBounds after findBinning)
    std::vector<std::int64_t> single;    ///< [P][bins]
    std::vector<std::int64_t> twoAxis;   ///< [P(P-1)/2][bins][bins], pair i > j at i(i-1)/2 + j, element [bin_i][bin_j]
    std::vector<std::int64_t> clamped;   ///< [P]: samples whose bin fell outside [0, bins) and were clamped

private:
    void check(const char* what, int rc) const
    {
        if (rc != MCMCPP_HIP_OK) die(what, rc, mcmcpp_hip_histograms_last_error(handle));
    }
    static void die(const char* what, int rc, const char* msg)
    {
        std::fprintf(stderr, "MCMCpp (MI355X): %s failed with code %d: %s\n", what, rc, msg ? msg : "");
        std::abort();
    }

    mcmcpp_hip_histograms* handle;
};

}  // namespace Detail
}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_DETAIL_DEVICEHISTOGRAMS_H
