/*
 * Analysis/PercentileAndMaximumFinder.h -- fine 1-D histograms of every parameter of the samples in a chain, counted on
 * the MI355X, with cumulative sums, percentile <-> value lookups and the peak computed on the host.
 *
 * Same class, constructor and methods as the reference (/root/reference/MCMCpp/Analysis/PercentileAndMaximumFinder.h):
 *
 *     MCMC::Analysis::PercentileAndMaximumFinder<double> pf(numParams, numWalkers, 10000);   // default 1000 bins
 *     pf.processChainData(sampler.getStepIttBegin(), sampler.getStepIttEnd(), sliceInterval);
 *     pf.getValueOfPeak(p);  pf.getPercentileFromValue(p, v);  pf.getValueFromPercentile(p, 84.1);
 *     pf.writeHistogramsInCsvFormat("percentileHistograms");      // <base>_p<i>.csv, <base>_cs_p<i>.csv
 *
 * Counting goes through libmcmcpp_hip.so (mcmcpp_hip_histograms_*, the binning of CornerHistograms.h).  The queries are
 * the reference's arithmetic, operation for operation, in ParamType, on the returned arrays; results are bit-identical
 * to the reference's wherever the reference is defined (tests/test_histograms.py).  Where it is not:
 *   - out-of-range bins are clamped and counted, as in CornerHistograms.h (getClampedCount, an extension); counts and
 *     cumulative sums are 64-bit;
 *   - getPercentileFromValue reads the cumulative sums at the same flat index as the reference, which does not offset
 *     it by the parameter (so every parameter reads parameter 0's sums, and a value in the extra bin above the range
 *     reads the next cell); an index past the end of the array is clamped to its last cell;
 *   - getValueFromPercentile's bisection stops where the reference's would repeat one step forever (first + 1 == last
 *     with the count above cell `first`), with `last`, the cell the search was converging on.
 * No GPU, no result: failures abort with the library's message, like everything else in this facade.
 */
#ifndef MCMCPP_ANALYSIS_PERCENTILES_H
#define MCMCPP_ANALYSIS_PERCENTILES_H

#include <cstdint>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "Detail/DeviceHistograms.h"

namespace MCMC
{
namespace Analysis
{
template <class ParamType>
class PercentileAndMaximumFinder
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    PercentileAndMaximumFinder(int numParams, int numWalkers, int binsPerAxis = 1000)
        : hist(numParams, numWalkers, binsPerAxis, false), cbCount(binsPerAxis + 1),
          cumSum(static_cast<size_t>(numParams) * (binsPerAxis + 1), 0), binned(false)
    {
    }

    /// Uses every sliceInterval'th step of [start, end), beginning with `start`.
    void processChainData(IttType start, IttType end, int sliceInterval = 1)
    {
        binned = false;
        hist.compute(start, end, sliceInterval);
        for (int p = 0; p < hist.pCount; ++p)
        {
            std::int64_t* cs = &cumSum[static_cast<size_t>(p) * cbCount];
            cs[0] = 0;
            for (int b = 0; b < hist.bCount; ++b) cs[b + 1] = cs[b] + hist.single[static_cast<size_t>(p) * hist.bCount + b];
        }
        binned = true;
    }

    /// Percentile ([0, 100]) of `val`, interpolated on the cumulative sums; -1 outside the range (or before any data).
    ParamType getPercentileFromValue(int pIndex, const ParamType& val)
    {
        const ParamType lo = lowEdge(pIndex), w = width(pIndex);
        if (!binned || val < lo || val > (lo + w * (hist.bCount + 1))) return static_cast<ParamType>(-1);
        const int binNum = Detail::truncToInt<ParamType>((val - lo) / w);
        const int cbinNum = binNum + 1;
        const ParamType x1 = ((cbinNum - 1) * w) + lo;
        const ParamType x2 = (cbinNum * w) + lo;
        const ParamType y1 = static_cast<ParamType>(flatCumSum(static_cast<long long>(cbinNum) - 1));
        const ParamType y2 = static_cast<ParamType>(flatCumSum(cbinNum));
        const ParamType m = (y2 - y1) / (x2 - x1);
        const ParamType b = ((x2 * y1) - (x1 * y2)) / (x2 - x1);
        const ParamType entries = static_cast<ParamType>(Detail::truncToInt<ParamType>((val * m) + b));
        return static_cast<ParamType>(100) * (entries / static_cast<ParamType>(hist.numPoints));
    }

    /// Value at percentile `per`, interpolated on the cumulative sums; the range's minimum - 1e4 outside [0, 100].
    ParamType getValueFromPercentile(int pIndex, const ParamType& per)
    {
        if (!binned || (0 > per) || (100 < per)) return static_cast<ParamType>(lowEdge(pIndex) - 1e4);
        const int entries = Detail::truncToInt<ParamType>((per / static_cast<ParamType>(100)) * static_cast<ParamType>(hist.numPoints));
        const std::int64_t* cs = &cumSum[static_cast<size_t>(pIndex) * cbCount];
        int first = 0, last = cbCount - 1;
        if (entries == 0)
            first = last = 1;
        else
            while (first != last)
            {
                const int mid = (first + last) / 2;
                if (cs[mid] >= entries)
                {
                    if (cs[mid - 1] <= entries)
                        first = last = mid;
                    else
                        last = mid;
                }
                else if (mid == first)
                    first = last;  // the reference repeats this step forever
                else
                    first = mid;
            }
        const ParamType x1 = static_cast<ParamType>(cs[last - 1]);
        const ParamType x2 = static_cast<ParamType>(cs[last]);
        const ParamType y1 = ((last - 1) * width(pIndex)) + lowEdge(pIndex);
        const ParamType y2 = (last * width(pIndex)) + lowEdge(pIndex);
        const ParamType m = (y2 - y1) / (x2 - x1);
        const ParamType b = ((x2 * y1) - (x1 * y2)) / (x2 - x1);
        return (entries * m) + b;
    }

    /// Centre of the first fullest bin.
    ParamType getValueOfPeak(int pIndex)
    {
        if (!binned) return static_cast<ParamType>(lowEdge(pIndex) - 1e4);
        const std::int64_t* h = &hist.single[static_cast<size_t>(pIndex) * hist.bCount];
        int binMax = 0;
        std::int64_t maxVal = -1;
        for (int b = 0; b < hist.bCount; ++b)
            if (h[b] > maxVal)
            {
                maxVal = h[b];
                binMax = b;
            }
        return static_cast<ParamType>(((binMax + 0.5) * width(pIndex)) + lowEdge(pIndex));
    }

    ParamType getParamMinimum(int pIndex) { return lowEdge(pIndex); }
    ParamType getParamMaximum(int pIndex) { return lowEdge(pIndex) + (width(pIndex) * hist.bCount); }

    /// <base>_p<i>.csv (histogram) and <base>_cs_p<i>.csv (cumulative sum) for every parameter, in the reference's layout.
    void writeHistogramsInCsvFormat(const std::string& fileNameBase)
    {
        for (int p = 0; p < hist.pCount; ++p)
        {
            writeCsv(p, fileNameBase + "_p", hist.bCount, lowEdge(p), &hist.single[static_cast<size_t>(p) * hist.bCount]);
            writeCsv(p, fileNameBase + "_cs_p", cbCount, lowEdge(p) - width(p), &cumSum[static_cast<size_t>(p) * cbCount]);
        }
    }

    ParamType getHistBinLowEdge(int pNum, int binNum) { return lowEdge(pNum) + (binNum * width(pNum)); }
    ParamType getHistBinHighEdge(int pNum, int binNum) { return lowEdge(pNum) + ((binNum + 1) * width(pNum)); }

    /// Extension (not in the reference): samples of parameter p whose bin fell outside [0, binsPerAxis) and were clamped.
    long long getClampedCount(int pNum) { return hist.clamped[pNum]; }

private:
    ParamType lowEdge(int p) const { return hist.bounds[2 * p]; }
    ParamType width(int p) const { return hist.bounds[2 * p + 1]; }
    std::int64_t flatCumSum(long long k) const
    {
        const long long last = static_cast<long long>(cumSum.size()) - 1;
        return cumSum[static_cast<size_t>(k < 0 ? 0 : (k > last ? last : k))];
    }

    void writeCsv(int p, const std::string& prefix, int cells, ParamType firstEdge, const std::int64_t* v)
    {
        std::ostringstream name;
        name << prefix << p << ".csv";
        std::ofstream out(name.str().c_str());
        out << "# Lines starting with a '#' in the first column are ignored\n";
        out << "# X-axis: nbins, first bin low edge, last bin high edge\n";
        out << cells << ", " << firstEdge << ", " << (lowEdge(p) + (hist.bCount * width(p))) << "\n";
        out << "# bin number, value\n";
        for (int b = 0; b < cells; ++b) out << b << ", " << v[b] << "\n";
    }

    Detail::DeviceHistograms<ParamType> hist;
    int cbCount;
    std::vector<std::int64_t> cumSum;
    bool binned;
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_PERCENTILES_H
