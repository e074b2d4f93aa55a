// histogram_ref_driver.cpp -- runs the REFERENCE's Analysis::CornerHistograms and Analysis::PercentileAndMaximumFinder over
// the reference's own Chain, for tests/golden/make_histogram_golden.py (which compiles it into a temporary directory).
//   usage: histogram_ref_driver <input.bin> <output.bin> <csv dir or ->
// input:  int32 dtype (0 f64, 1 f32), W, P, n_steps, slice, corner_bins, pct_bins, n_val, n_per;
//         T steps[n_steps][W][P]; T val_queries[P][n_val]; T per_queries[P][n_per]
// output: corner paramBounds[P][2] (T), 1-D [P][cb] (int32), 2-D [P(P-1)/2][cb*cb] (int32);
//         finder paramBounds[P][2], hists[P][pb], cumSum[P][pb+1], numPoints (int32);
//         getPercentileFromValue[P][n_val], getValueFromPercentile[P][n_per], getValueOfPeak[P],
//         getParamMinimum[P], getParamMaximum[P] (T)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

// the arrays the results live in are private members of the reference classes
#define private public
#include "Chain/Chain.h"
#include "Analysis/CornerHistograms.h"
#include "Analysis/PercentileAndMaximumFinder.h"
#undef private

static FILE* g_out;
template <class V>
static void put(const V* p, size_t n)
{
    if (n && std::fwrite(p, sizeof(V), n, g_out) != n) std::exit(3);
}

template <class T>
static int run(FILE* in, int W, int P, int n, int slice, int cb, int pb, int nv, int np, const char* csv)
{
    std::vector<T> steps(static_cast<size_t>(n) * W * P), vq(static_cast<size_t>(P) * nv), pq(static_cast<size_t>(P) * np);
    if (std::fread(steps.data(), sizeof(T), steps.size(), in) != steps.size()) return 2;
    if (vq.size() && std::fread(vq.data(), sizeof(T), vq.size(), in) != vq.size()) return 2;
    if (pq.size() && std::fread(pq.data(), sizeof(T), pq.size(), in) != pq.size()) return 2;
    MCMC::Chain::Chain<T> chain(W, P, static_cast<unsigned long long>(steps.size() + 64) * sizeof(T) * 4);
    for (int k = 0; k < n; ++k)
    {
        for (int w = 0; w < W; ++w) chain.storeWalker(w, &steps[(static_cast<size_t>(k) * W + w) * P]);
        chain.incrementChainStep();
    }
    MCMC::Analysis::CornerHistograms<T> corner(P, W, cb);
    corner.calculateHistograms(chain.getStepIteratorBegin(), chain.getStepIteratorEnd(), slice);
    MCMC::Analysis::PercentileAndMaximumFinder<T> finder(P, W, pb);
    finder.processChainData(chain.getStepIteratorBegin(), chain.getStepIteratorEnd(), slice);
    if (csv[0] != '-')
    {
        corner.saveHistsCsvFormat(std::string(csv) + "/corner");
        finder.writeHistogramsInCsvFormat(std::string(csv) + "/finder");
    }
    put(corner.paramBounds, 2 * static_cast<size_t>(P));
    put(corner.singleAxisHists, static_cast<size_t>(P) * cb);
    for (int q = 0; q < corner.numTwoAxis; ++q) put(corner.twoAxisHists[q], static_cast<size_t>(cb) * cb);
    put(finder.paramBounds, 2 * static_cast<size_t>(P));
    put(finder.hists, static_cast<size_t>(P) * pb);
    put(finder.cumSum, static_cast<size_t>(P) * (pb + 1));
    put(&finder.numPoints, 1);
    std::vector<T> r;
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < nv; ++k) r.push_back(finder.getPercentileFromValue(p, vq[static_cast<size_t>(p) * nv + k]));
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < np; ++k) r.push_back(finder.getValueFromPercentile(p, pq[static_cast<size_t>(p) * np + k]));
    for (int p = 0; p < P; ++p) r.push_back(finder.getValueOfPeak(p));
    for (int p = 0; p < P; ++p) r.push_back(finder.getParamMinimum(p));
    for (int p = 0; p < P; ++p) r.push_back(finder.getParamMaximum(p));
    put(r.data(), r.size());
    delete[] corner.paramBounds;  // (the reference's destructor leaks it)
    corner.paramBounds = nullptr;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    g_out = std::fopen(argv[2], "wb");
    if (!in || !g_out) return 1;
    int32_t h[9];
    if (std::fread(h, sizeof(int32_t), 9, in) != 9) return 2;
    const int rc = h[0] == 0 ? run<double>(in, h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], argv[3])
                             : run<float>(in, h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], argv[3]);
    std::fclose(in);
    std::fclose(g_out);
    return rc;
}
