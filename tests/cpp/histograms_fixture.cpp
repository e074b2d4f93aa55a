// histograms_fixture.cpp -- the facade's CornerHistograms and PercentileAndMaximumFinder over a Chain filled with a
// fixture's steps (tests/golden/hist_*.npz, produced by the reference): tests/test_histograms.py compares the output with
// the reference's.
//   usage: histograms_fixture <input.bin> <output.bin> <csv dir>      (needs an MI355X)
// input: tests/golden/histogram_ref_driver.cpp's input format.
// output (T unless noted): corner getHistBinLowEdge(p, 0), getHistBinHighEdge(p, bins-1) [P][2]; get1dHistBin [P][cb];
//   get2dHistBin(i, j, binx, biny) [pairs][biny][binx]; finder getPercentileFromValue [P][n_val]; getValueFromPercentile
//   [P][n_per]; getValueOfPeak, getParamMinimum, getParamMaximum [P] each; clamped counts of both [2][P] (int64)
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "Analysis/CornerHistograms.h"
#include "Analysis/PercentileAndMaximumFinder.h"
#include "Chain/Chain.h"

template <class T>
static int run(FILE* in, FILE* out, int W, int P, int n, int slice, int cb, int pb, int nv, int np, const std::string& dir)
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
    corner.saveHistsCsvFormat(dir + "/corner");
    MCMC::Analysis::PercentileAndMaximumFinder<T> finder(P, W, pb);
    finder.processChainData(chain.getStepIteratorBegin(), chain.getStepIteratorEnd(), slice);
    finder.writeHistogramsInCsvFormat(dir + "/finder");
    std::vector<T> r;
    for (int p = 0; p < P; ++p)
    {
        r.push_back(corner.getHistBinLowEdge(p, 0));
        r.push_back(corner.getHistBinHighEdge(p, cb - 1));
    }
    for (int p = 0; p < P; ++p)
        for (int b = 0; b < cb; ++b) r.push_back(corner.get1dHistBin(p, b));
    for (int i = 1; i < P; ++i)
        for (int j = 0; j < i; ++j)
            for (int by = 0; by < cb; ++by)
                for (int bx = 0; bx < cb; ++bx) r.push_back(corner.get2dHistBin(i, j, bx, by));
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < nv; ++k) r.push_back(finder.getPercentileFromValue(p, vq[static_cast<size_t>(p) * nv + k]));
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < np; ++k) r.push_back(finder.getValueFromPercentile(p, pq[static_cast<size_t>(p) * np + k]));
    for (int p = 0; p < P; ++p) r.push_back(finder.getValueOfPeak(p));
    for (int p = 0; p < P; ++p) r.push_back(finder.getParamMinimum(p));
    for (int p = 0; p < P; ++p) r.push_back(finder.getParamMaximum(p));
    std::fwrite(r.data(), sizeof(T), r.size(), out);
    for (int p = 0; p < P; ++p)
    {
        const int64_t c = corner.getClampedCount(p);
        std::fwrite(&c, sizeof c, 1, out);
    }
    for (int p = 0; p < P; ++p)
    {
        const int64_t c = finder.getClampedCount(p);
        std::fwrite(&c, sizeof c, 1, out);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t h[9];
    if (std::fread(h, sizeof(int32_t), 9, in) != 9) return 2;
    const int rc = h[0] == 0 ? run<double>(in, out, h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], argv[3])
                             : run<float>(in, out, h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], argv[3]);
    std::fclose(in);
    std::fclose(out);
    if (rc == 0) std::printf("histograms_fixture OK\n");
    return rc;
}
