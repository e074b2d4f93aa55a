// histograms_facade.cpp -- the facade's Analysis::CornerHistograms and Analysis::PercentileAndMaximumFinder on a chain
// the facade's own sampler produced.  Writes the chain and every result to <out.bin> and the CSV files to <dir>;
// tests/test_histograms.py checks them against the restatement of the same chain (tests/histogram_restatement.py).
//   usage: histograms_facade <out.bin> <dir>      (needs an MI355X)
// out.bin, per case: int32 dtype, W, P, n_steps, slice, corner bins, finder bins, n_val, n_per; T chain[n][W][P];
//   corner: T low edge / high edge of bins 0 and bins-1 [P][4], get1dHistBin [P][cb] (T), get2dHistBin [pairs][cb][cb] (T,
//   [biny][binx]), clamped [P] (int64); finder: getParamMinimum, getParamMaximum [P], clamped [P] (int64), value queries
//   [P][n_val] and getPercentileFromValue of them, percentile queries [P][n_per] and getValueFromPercentile of them,
//   getValueOfPeak [P]
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "Analysis/CornerHistograms.h"
#include "Analysis/PercentileAndMaximumFinder.h"
#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/StretchMove.h"

static FILE* g_out;
template <class V>
static void put(const V& v)
{
    std::fwrite(&v, sizeof(V), 1, g_out);
}

template <class T>
static void run(int W, int P, int steps, int slice, int cb, int pb, const std::string& dir, const char* tag)
{
    typedef MCMC::Device::Rosenbrock<T> Target;
    typedef MCMC::Mover::StretchMove<T, Target> Mover;
    Target target(P, T(1), T(100), T(0.05));
    Mover mover(P, 7, target);
    MCMC::EnsembleSampler<T, Mover> sampler(7, W, P, mover);
    std::vector<T> pos(static_cast<size_t>(W) * P), aux(W);
    unsigned long long s = 777;
    for (size_t k = 0; k < pos.size(); ++k)
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        pos[k] = T(((s >> 11) * (1.0 / 9007199254740992.0)) * 4.0 - 2.0);
    }
    for (int w = 0; w < W; ++w) aux[w] = target.calcLogPostProb(&pos[static_cast<size_t>(w) * P]);
    sampler.setInitialWalkerPos(pos.data(), aux.data());
    sampler.runMCMC(steps);

    MCMC::Analysis::CornerHistograms<T> corner(P, W, cb);
    corner.calculateHistograms(sampler.getStepIttBegin(), sampler.getStepIttEnd(), slice);
    corner.saveHistsCsvFormat(dir + "/" + tag + "_corner");
    MCMC::Analysis::PercentileAndMaximumFinder<T> finder(P, W, pb);
    finder.processChainData(sampler.getStepIttBegin(), sampler.getStepIttEnd(), slice);
    finder.writeHistogramsInCsvFormat(dir + "/" + tag + "_finder");

    const int nv = 9, np = 9;
    int n = 0;
    for (auto it = sampler.getStepIttBegin(); it != sampler.getStepIttEnd(); ++it) ++n;
    const int32_t head[9] = {sizeof(T) == 8 ? 0 : 1, W, P, n, slice, cb, pb, nv, np};
    std::fwrite(head, sizeof(int32_t), 9, g_out);
    for (auto it = sampler.getStepIttBegin(); it != sampler.getStepIttEnd(); ++it) std::fwrite(*it, sizeof(T), static_cast<size_t>(W) * P, g_out);
    for (int p = 0; p < P; ++p)
    {
        put(corner.getHistBinLowEdge(p, 0));
        put(corner.getHistBinHighEdge(p, 0));
        put(corner.getHistBinLowEdge(p, cb - 1));
        put(corner.getHistBinHighEdge(p, cb - 1));
    }
    for (int p = 0; p < P; ++p)
        for (int b = 0; b < cb; ++b) put(corner.get1dHistBin(p, b));
    for (int i = 1; i < P; ++i)
        for (int j = 0; j < i; ++j)
            for (int by = 0; by < cb; ++by)
                for (int bx = 0; bx < cb; ++bx) put(corner.get2dHistBin(i, j, bx, by));
    for (int p = 0; p < P; ++p) put(static_cast<int64_t>(corner.getClampedCount(p)));
    for (int p = 0; p < P; ++p) put(finder.getParamMinimum(p));
    for (int p = 0; p < P; ++p) put(finder.getParamMaximum(p));
    for (int p = 0; p < P; ++p) put(static_cast<int64_t>(finder.getClampedCount(p)));
    for (int p = 0; p < P; ++p)
    {
        const T lo = finder.getParamMinimum(p), hi = finder.getParamMaximum(p);
        for (int k = 0; k < nv; ++k)
        {
            const T v = lo + (hi - lo) * static_cast<T>(k - 1) / static_cast<T>(nv - 3);
            put(v);
            put(finder.getPercentileFromValue(p, v));
        }
    }
    const double pers[np] = {-1.0, 0.0, 2.5, 15.9, 50.0, 84.1, 97.5, 100.0, 100.5};
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < np; ++k)
        {
            const T per = static_cast<T>(pers[k]);
            put(per);
            put(finder.getValueFromPercentile(p, per));
        }
    for (int p = 0; p < P; ++p) put(finder.getValueOfPeak(p));
}

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    g_out = std::fopen(argv[1], "wb");
    if (!g_out) return 1;
    run<double>(64, 6, 60, 1, 16, 1000, argv[2], "f64");
    run<double>(200, 5, 40, 3, 100, 10000, argv[2], "f64_slice3");
    run<float>(96, 4, 50, 2, 12, 300, argv[2], "f32");
    std::fclose(g_out);
    std::printf("histograms_facade OK\n");
    return 0;
}
