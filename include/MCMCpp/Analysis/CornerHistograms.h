/*
 * Analysis/CornerHistograms.h -- the 1-D histogram of every parameter and the 2-D histogram of every parameter pair of
 * the samples in a chain (the panels of a corner plot), counted on the MI355X.
 *
 * Same class, constructor and methods as the reference (/root/reference/MCMCpp/Analysis/CornerHistograms.h):
 *
 *     MCMC::Analysis::CornerHistograms<double> ch(numParams, numWalkers);          // binsPerAxis = 100
 *     ch.calculateHistograms(sampler.getStepIttBegin(), sampler.getStepIttEnd(), sliceInterval);
 *     ch.get1dHistBin(p, bin);  ch.get2dHistBin(p1, p2, binx, biny);  ch.getHistBinLowEdge(p, bin);
 *     ch.saveHistsCsvFormat("chainHist");                                        // chainHist_p<i>.csv, chainHist_p<i>_p<j>.csv
 *
 * The selected steps are handed to libmcmcpp_hip.so (include/mcmcpp_hip.h, mcmcpp_hip_histograms_*), which finds every
 * parameter's range, applies the reference's bound tweak and width in the chain's element type, bins every sample with
 * the reference's expression and counts P(P-1)/2 pair histograms in LDS.  Every sample the reference bins in range lands
 * in the reference's bin; bin edges and CSV files are the reference's (tests/test_histograms.py, against fixtures the
 * reference produced).  Two deliberate differences:
 *   - the reference's upper-bound tweak moves every positive maximum (and, for data <= 0, a sample at exactly 0) past the
 *     last bin, and it then writes outside its arrays; here such a sample is clamped into bin 0 or bins - 1 and counted:
 *     getClampedCount(p), an extension;
 *   - counts are 64-bit (the reference's are int).
 * No GPU, no result: failures abort with the library's message, like everything else in this facade.
 */
#ifndef MCMCPP_ANALYSIS_CORNERHISTOGRAMS_H
#define MCMCPP_ANALYSIS_CORNERHISTOGRAMS_H

#include <cstdint>
#include <fstream>
#include <sstream>
#include <string>

#include "Detail/DeviceHistograms.h"

namespace MCMC
{
namespace Analysis
{
template <class ParamType>
class CornerHistograms
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    CornerHistograms(int numParams, int numWalkers, int binsPerAxis = 100) : hist(numParams, numWalkers, binsPerAxis, true) {}

    /// Uses every sliceInterval'th step of [start, end), beginning with `start`.
    void calculateHistograms(IttType start, IttType end, int sliceInterval = 1) { hist.compute(start, end, sliceInterval); }

    /// <base>_p<i>.csv for every parameter and <base>_p<i>_p<j>.csv for every pair j < i, in the reference's layout.
    void saveHistsCsvFormat(const std::string& fileNameBase)
    {
        for (int i = 0; i < hist.pCount; ++i)
        {
            write1d(i, fileNameBase);
            for (int j = 0; j < i; ++j) write2d(i, j, fileNameBase);
        }
    }

    ParamType getHistBinLowEdge(int pNum, int binNum) { return lowEdge(pNum) + (binNum * width(pNum)); }
    ParamType getHistBinHighEdge(int pNum, int binNum) { return lowEdge(pNum) + ((binNum + 1) * width(pNum)); }
    ParamType get1dHistBin(int pNum, int bin) { return static_cast<ParamType>(hist.single[static_cast<size_t>(pNum) * hist.bCount + bin]); }
    /// p1 > p2; binx is p2's bin, biny is p1's (the reference's accessor)
    ParamType get2dHistBin(int p1, int p2, int binx, int biny)
    {
        return static_cast<ParamType>(hist.twoAxis[(static_cast<size_t>(p1) * (p1 - 1) / 2 + p2) * hist.bCount * hist.bCount +
                                                   static_cast<size_t>(biny) * hist.bCount + binx]);
    }

    /// Extension (not in the reference): samples of parameter p whose bin fell outside [0, binsPerAxis) and were clamped.
    long long getClampedCount(int pNum) { return hist.clamped[pNum]; }

private:
    ParamType lowEdge(int p) const { return hist.bounds[2 * p]; }
    ParamType width(int p) const { return hist.bounds[2 * p + 1]; }
    ParamType topEdge(int p) const { return lowEdge(p) + (hist.bCount * width(p)); }

    void write1d(int p, const std::string& base)
    {
        std::ostringstream name;
        name << base << "_p" << p << ".csv";
        std::ofstream out(name.str().c_str());
        out << "# Lines starting with a '#' in the first column are ignored\n";
        out << "# X-axis: nbins, first bin low edge, last bin high edge\n";
        out << hist.bCount << ", " << lowEdge(p) << ", " << topEdge(p) << "\n";
        out << "# bin number, value\n";
        const std::int64_t* h = &hist.single[static_cast<size_t>(p) * hist.bCount];
        for (int b = 0; b < hist.bCount; ++b) out << b << ", " << h[b] << "\n";
    }

    void write2d(int p1, int p2, const std::string& base)
    {
        std::ostringstream name;
        name << base << "_p" << p1 << "_p" << p2 << ".csv";
        std::ofstream out(name.str().c_str());
        out << "# Lines starting with a '#' in the first column are ignored\n";
        out << "# X-axis: nbins, first bin low edge, last bin high edge\n";
        out << hist.bCount << ", " << lowEdge(p1) << ", " << topEdge(p1) << "\n";
        out << "# Y-axis: nbins, first bin low edge, last bin high edge\n";
        out << hist.bCount << ", " << lowEdge(p2) << ", " << topEdge(p2) << "\n";
        out << "# x-bin number, y-bin number, value\n";
        const size_t b2 = static_cast<size_t>(hist.bCount) * hist.bCount;
        const std::int64_t* h = &hist.twoAxis[(static_cast<size_t>(p1) * (p1 - 1) / 2 + p2) * b2];
        for (int a = 0; a < hist.bCount; ++a)
            for (int b = 0; b < hist.bCount; ++b) out << a << ", " << b << ", " << h[static_cast<size_t>(a) * hist.bCount + b] << "\n";
    }

    Detail::DeviceHistograms<ParamType> hist;
};

}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_CORNERHISTOGRAMS_H
