// Driver of tests/test_device_facade.py: one reference-style program per case, written against the facade alone.  The test
// runs it twice -- with a host chain and with MCMCPP_CHAIN_MEMORY=device -- and compares the files it writes byte for byte.
//
//   device_facade <case> <out.bin> [libbatch_calc.so]
// out.bin receives everything the case computes (steps through both iterators, counts, analysis results); out.bin.cov the
// covariance matrices of the analysis case.  stdout carries what differs by design between the two runs, as key=value
// lines: the chain's memory kind, hostBytesFetched() at the points the test asks about, reallocations seen.
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "Analysis/AutoCorrCalc.h"
#include "Analysis/CornerHistograms.h"
#include "Analysis/CovarianceMatrix.h"
#include "Analysis/PercentileAndMaximumFinder.h"
#include "Device/Calculators.h"
#include "EnsembleSampler.h"
#include "Movers/DifferentialEvolution.h"
#include "Movers/StretchMove.h"
#include "ParallelEnsembleSampler.h"

using namespace MCMC;

static std::vector<unsigned char> out;
template <class V>
static void put(const V& v)
{
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    out.insert(out.end(), p, p + sizeof(V));
}
static void putBytes(const void* p, size_t n) { out.insert(out.end(), static_cast<const unsigned char*>(p), static_cast<const unsigned char*>(p) + n); }

static int save(const std::string& path, const std::vector<unsigned char>& bytes)
{
    FILE* fp = std::fopen(path.c_str(), "wb");
    if (!fp || std::fwrite(bytes.data(), 1, bytes.size(), fp) != bytes.size()) return 2;
    std::fclose(fp);
    return 0;
}

// the initial placement: a fixed pseudo-random scatter in [-2, 2) (the same in both runs; its log-posteriors come from the Calculator)
template <class T>
static std::vector<T> scatter(int W, int D)
{
    std::vector<T> pos(static_cast<size_t>(W) * D);
    std::uint64_t s = 0x9E3779B97F4A7C15ULL;
    for (T& v : pos)
    {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        v = static_cast<T>(static_cast<double>(s >> 11) / 9007199254740992.0 * 4.0 - 2.0);
    }
    return pos;
}

template <class T>
static std::vector<T> tridiagonalPrecision(int D)
{
    const double rho = 0.5;
    std::vector<T> P(static_cast<size_t>(D) * D, T(0));
    for (int i = 0; i < D; ++i)
    {
        P[static_cast<size_t>(i) * D + i] = static_cast<T>(((i == 0 || i == D - 1) ? 1.0 : 1.0 + rho * rho) / (1.0 - rho * rho));
        if (i + 1 < D) P[static_cast<size_t>(i) * D + i + 1] = P[static_cast<size_t>(i + 1) * D + i] = static_cast<T>(-rho / (1.0 - rho * rho));
    }
    return P;
}

static const char* kindName(Chain::Detail::MemoryKind k)
{
    return k == Chain::Detail::MemoryKind::Device ? "device" : (k == Chain::Detail::MemoryKind::Pinned ? "pinned" : "heap");
}

// every stored step through the step iterator and through the parameter-set iterator, and the counts
template <class T, class Sampler>
static void dumpChain(Sampler& s, int W, int D)
{
    put<std::int64_t>(s.getStoredSteps());
    put<std::uint64_t>(s.getAcceptedSteps());
    put<std::uint64_t>(s.getTotalSteps());
    std::int64_t steps = 0;
    for (auto it = s.getStepIttBegin(); it != s.getStepIttEnd(); ++it, ++steps) putBytes(*it, sizeof(T) * W * D);
    put(steps);
    std::int64_t sets = 0;
    for (auto it = s.getParamSetIttBegin(); it != s.getParamSetIttEnd(); ++it, ++sets) putBytes(*it, sizeof(T) * D);
    put(sets);
}

template <class T, class Sampler, class Calc>
static void place(Sampler& s, Calc& calc, int W, int D)
{
    std::vector<T> pos = scatter<T>(W, D), aux(W);
    for (int w = 0; w < W; ++w) aux[w] = calc.calcLogPostProb(&pos[static_cast<size_t>(w) * D]);
    s.setInitialWalkerPos(pos.data(), aux.data());
}

// ---- sampling cases -----------------------------------------------------------------------------------------------------
template <class T, class MoverType, class Calc>
static int sampleCase(Calc calc, int W, int D, int steps, int interval)
{
    MoverType mover(D, 0, calc);
    EnsembleSampler<T, MoverType> sampler(7, W, D, mover);
    sampler.setSlicingMode(interval > 1, interval);
    place<T>(sampler, calc, W, D);
    const bool ok = sampler.runMCMC(steps / 2) && sampler.runMCMC(steps - steps / 2);
    put<int>(ok);
    std::printf("kind=%s\n", kindName(sampler.chain().memoryKind()));
    std::printf("device_steps=%lld\n", static_cast<long long>(sampler.chain().deviceSteps().steps));
    std::printf("fetched_after_sampling=%llu\n", sampler.chain().hostBytesFetched());
    dumpChain<T>(sampler, W, D);
    // reset forgets the chain, the walkers stay; their positions become step 0 again
    sampler.reset();
    put<int>(sampler.getStoredSteps());
    sampler.storeCurrentWalkerPositions();
    put<int>(sampler.runMCMC(3));
    dumpChain<T>(sampler, W, D);
    return 0;
}

// the batch target: tests/cpp/batch_calc.hip's restatement of IsoGaussian, loaded at run time
typedef void* (*BatchCreate)(int, int, int, const void*, int);
typedef int (*BatchLogp)(void*, const void*, void*, std::int64_t, std::int32_t, void*);
static BatchLogp batchLogp = nullptr;
static void* batchUser = nullptr;
class BatchIso
{
public:
    static const int hipCalcId = Device::BatchCalcId;
    explicit BatchIso(int numParams) : host(numParams) {}
    double calcLogPostProb(double* x) { return host.calcLogPostProb(x); }
    int hipBatchLogPostProb(const double* dProposals, long long count, int numParams, double* dLogp, void* hipStream)
    {
        return batchLogp(batchUser, dProposals, dLogp, count, numParams, hipStream);
    }

private:
    Device::IsoGaussian<double> host;
};

// a PostStepAction that records the first walker of every step it sees, at every call
template <class T>
struct FirstWalkerRecorder
{
    int D;
    std::vector<T> seen;
    long calls;
    void performAction(const Chain::ChainStepIterator<T>& start, const Chain::ChainStepIterator<T>& end)
    {
        ++calls;
        for (Chain::ChainStepIterator<T> it(start); it != end; ++it) seen.insert(seen.end(), *it, *it + D);
    }
};

static int actionCase()
{
    const int W = 64, D = 4;
    typedef Device::IsoGaussian<double> Calc;
    typedef Mover::StretchMove<double, Calc> MoverType;
    Calc calc(D);
    MoverType mover(D, 0, calc);
    FirstWalkerRecorder<double> action;
    action.D = D;
    action.calls = 0;
    ParallelEnsembleSampler<double, MoverType, FirstWalkerRecorder<double> > sampler(7, 4, W, D, mover, 2147483648ULL, &action);
    sampler.setSamplingMode(2, 0);
    place<double>(sampler, calc, W, D);
    put<int>(sampler.runMCMC(40));
    std::printf("kind=%s\n", kindName(sampler.chain().memoryKind()));
    put<std::int64_t>(action.calls);
    put<std::int64_t>(static_cast<std::int64_t>(action.seen.size()));
    putBytes(action.seen.data(), sizeof(double) * action.seen.size());
    dumpChain<double>(sampler, W, D);
    return 0;
}

// ---- growth and budget --------------------------------------------------------------------------------------------------
static int growthCase()
{
    const int W = 64, D = 4;
    typedef Device::IsoGaussian<double> Calc;
    typedef Mover::StretchMove<double, Calc> MoverType;
    Calc calc(D);
    {
        MoverType mover(D, 0, calc);
        EnsembleSampler<double, MoverType> sampler(7, W, D, mover);
        place<double>(sampler, calc, W, D);
        int reallocations = 0;
        const double* base = sampler.chain().deviceSteps().base;
        const int runs[3] = {20, 20, 40};
        for (int r = 0; r < 3; ++r)
        {
            put<int>(sampler.runMCMC(runs[r]));
            const double* now = sampler.chain().deviceSteps().base;
            if (now != base) ++reallocations;
            base = now;
        }
        std::printf("kind=%s\nreallocations=%d\n", kindName(sampler.chain().memoryKind()), reallocations);
        dumpChain<double>(sampler, W, D);
    }
    {
        // a budget of 50 steps: the run that fills it reports false, with 50 steps stored
        MoverType mover(D, 0, calc);
        EnsembleSampler<double, MoverType> sampler(7, W, D, mover, 50ULL * W * D * sizeof(double));
        place<double>(sampler, calc, W, D);
        put<int>(sampler.runMCMC(30));
        put<int>(sampler.runMCMC(30));
        put<int>(sampler.runMCMC(1));
        dumpChain<double>(sampler, W, D);
    }
    return 0;
}

// ---- compaction ---------------------------------------------------------------------------------------------------------
template <class T, class Calc>
static int compactCase(Calc calc, int W, int D)
{
    typedef Mover::StretchMove<T, Calc> MoverType;
    const int stored = 61;  // the initial placement and 60 steps
    const int cases[6][2] = {{0, 1}, {20, 1}, {0, 5}, {7, 3}, {stored - 1, 1}, {3, stored}};  // (burnIn, interval)
    unsigned long long fetchedBySlicing = 0;
    for (int c = 0; c < 6; ++c)
    {
        MoverType mover(D, 0, calc);
        EnsembleSampler<T, MoverType> sampler(7, W, D, mover);
        place<T>(sampler, calc, W, D);
        put<int>(sampler.runMCMC(stored - 1));
        put<int>(sampler.getStoredSteps());
        const unsigned long long before = sampler.chain().hostBytesFetched();
        sampler.sliceAndBurnChain(cases[c][1], cases[c][0]);
        fetchedBySlicing += sampler.chain().hostBytesFetched() - before;
        if (c == 0) std::printf("kind=%s\n", kindName(sampler.chain().memoryKind()));
        std::printf("stored_after_case_%d=%d\n", c, sampler.getStoredSteps());
        dumpChain<T>(sampler, W, D);
        // the chain goes on from where the compaction left it
        put<int>(sampler.runMCMC(2));
        dumpChain<T>(sampler, W, D);
    }
    std::printf("fetched_by_slicing=%llu\n", fetchedBySlicing);
    return 0;
}

// ---- analysis -----------------------------------------------------------------------------------------------------------
static void putFile(const std::string& path)
{
    std::ifstream in(path.c_str(), std::ios::binary);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string text = ss.str();
    put<std::int64_t>(static_cast<std::int64_t>(text.size()));
    putBytes(text.data(), text.size());
}

static int analysisCase(const std::string& outPath)
{
    const int W = 64, D = 4, bins = 20;
    typedef Device::IsoGaussian<double> Calc;
    typedef Mover::StretchMove<double, Calc> MoverType;
    Calc calc(D);
    MoverType mover(D, 0, calc);
    EnsembleSampler<double, MoverType> sampler(7, W, D, mover);
    sampler.setSlicingMode(true, 3);
    place<double>(sampler, calc, W, D);
    put<int>(sampler.runMCMC(200));
    sampler.sliceAndBurnChain(2, 20);
    put<int>(sampler.getStoredSteps());
    std::vector<unsigned char> cov;
    for (int from = 0; from <= 5; from += 5)  // the whole chain, and a range that starts inside it
    {
        auto start = sampler.getStepIttBegin();
        start += from;
        const auto end = sampler.getStepIttEnd();
        const int samples = sampler.getStoredSteps() - from;
        Analysis::AutoCorrCalc<double> ac(D, W);
        ac.calcAutoCorrTimes(start, end, samples);
        for (int p = 0; p < D; ++p) put(ac.retrieveAutoCorrelationTime(p));
        ac.calcAutoCorrTimes(start, end, samples, W / 2);
        for (int p = 0; p < D; ++p) put(ac.retrieveAutoCorrelationTime(p));
        for (int slice = 1; slice <= 3; slice += 2)
        {
            Analysis::CovarianceMatrix<double> cm(D, W);
            cm.calculateCovar(start, end, slice);
            for (int i = 0; i < D; ++i)
                for (int j = 0; j < D; ++j)
                {
                    const double v[2] = {cm.getCovarianceMatrixElement(i, j), cm.getCorrelationMatrixElement(i, j)};
                    cov.insert(cov.end(), reinterpret_cast<const unsigned char*>(v), reinterpret_cast<const unsigned char*>(v) + sizeof v);
                }
            Analysis::CornerHistograms<double> corner(D, W, bins);
            corner.calculateHistograms(start, end, slice);
            corner.saveHistsCsvFormat(outPath + ".corner");
            for (int p = 0; p < D; ++p)
            {
                std::ostringstream name;
                name << outPath << ".corner_p" << p << ".csv";
                putFile(name.str());
                put<long long>(corner.getClampedCount(p));
                for (int b = 0; b < bins; ++b) put(corner.get1dHistBin(p, b));
                for (int q = 0; q < p; ++q)
                {
                    std::ostringstream pair;
                    pair << outPath << ".corner_p" << p << "_p" << q << ".csv";
                    putFile(pair.str());
                    for (int b = 0; b < bins; ++b) put(corner.get2dHistBin(p, q, b, (b * 7) % bins));
                }
            }
            Analysis::PercentileAndMaximumFinder<double> pamf(D, W, 50 * bins);
            pamf.processChainData(start, end, slice);
            for (int p = 0; p < D; ++p)
            {
                const double peak = pamf.getValueOfPeak(p);
                put(peak);
                put(pamf.getPercentileFromValue(p, peak));
                put(pamf.getValueFromPercentile(p, 15.9));
                put(pamf.getValueFromPercentile(p, 50.0));
                put(pamf.getValueFromPercentile(p, 84.1));
                put(pamf.getParamMinimum(p));
                put(pamf.getParamMaximum(p));
                put<long long>(pamf.getClampedCount(p));
            }
        }
    }
    std::printf("kind=%s\n", kindName(sampler.chain().memoryKind()));
    const unsigned long long before = sampler.chain().hostBytesFetched();
    std::printf("fetched_after_analysis=%llu\n", before);
    const double* first = *sampler.getStepIttBegin();
    putBytes(first, sizeof(double) * W * D);
    const double* again = *sampler.getStepIttBegin();  // the same step: no second copy
    put<int>(first == again);
    std::printf("fetched_by_one_dereference=%llu\n", sampler.chain().hostBytesFetched() - before);
    return save(outPath + ".cov", cov);
}

int main(int argc, char** argv)
{
    if (argc < 3)
    {
        std::printf("usage: device_facade case out.bin [libbatch_calc.so]\n");
        return 2;
    }
    const std::string which = argv[1], outPath = argv[2];
    int rc = 2;
    if (which == "stretch")
        rc = sampleCase<double, Mover::StretchMove<double, Device::IsoGaussian<double> > >(Device::IsoGaussian<double>(4), 64, 4, 200, 3);
    else if (which == "stretch_f32_96x16")
        rc = sampleCase<float, Mover::StretchMove<float, Device::DenseGaussian<float> > >(Device::DenseGaussian<float>(16, tridiagonalPrecision<float>(16).data()), 96,
                                                                                          16, 60, 2);
    else if (which == "stretch_f32_80x5")
        rc = sampleCase<float, Mover::StretchMove<float, Device::DenseGaussian<float> > >(Device::DenseGaussian<float>(5, tridiagonalPrecision<float>(5).data()), 80, 5,
                                                                                          60, 2);
    else if (which == "diffevo")
        rc = sampleCase<double, Mover::DifferentialEvolution<double, Device::IsoGaussian<double> > >(Device::IsoGaussian<double>(4), 64, 4, 100, 2);
    else if (which == "batch")
    {
        void* lib = argc > 3 ? dlopen(argv[3], RTLD_NOW) : nullptr;
        if (!lib)
        {
            std::printf("cannot load the batch callback library: %s\n", argc > 3 ? dlerror() : "no path given");
            return 2;
        }
        const BatchCreate create = reinterpret_cast<BatchCreate>(dlsym(lib, "batch_calc_create"));
        batchLogp = reinterpret_cast<BatchLogp>(dlsym(lib, "batch_calc_logp"));
        if (!create || !batchLogp) return 2;
        batchUser = create(0, 0, 4, nullptr, 0);
        if (!batchUser) return 2;
        rc = sampleCase<double, Mover::StretchMove<double, BatchIso> >(BatchIso(4), 64, 4, 100, 2);
    }
    else if (which == "action")
        rc = actionCase();
    else if (which == "growth")
        rc = growthCase();
    else if (which == "compact_64x4")
        rc = compactCase<double>(Device::IsoGaussian<double>(4), 64, 4);
    else if (which == "compact_80x5_f32")
        rc = compactCase<float>(Device::DenseGaussian<float>(5, tridiagonalPrecision<float>(5).data()), 80, 5);
    else if (which == "analysis")
        rc = analysisCase(outPath);
    if (rc != 0) return rc;
    if (save(outPath, out) != 0) return 2;
    std::printf("device_facade OK\n");
    return 0;
}
