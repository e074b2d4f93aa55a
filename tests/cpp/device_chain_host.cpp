// The host code of a device chain (include/MCMCpp/Chain/Chain.h with Detail::BlockMemory::onDevice), run on the CPU against a
// FAKE backend: plain malloc / free / memcpy behind the chain's obtain, release and copy pointers, and a compaction that
// executes the wave schedule of mcmcpp_amd/csrc/chain_compact_plan.hpp with memcpy (which, unlike memmove, may not be handed
// overlapping ranges: AddressSanitizer reports a wave that reads what it writes).  Every operation is mirrored on a host
// Chain; contents and counts have to agree.  tests/test_device_facade.py builds this with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Chain/Chain.h"
#include "chain_compact_plan.hpp"

using namespace MCMC::Chain;

static int failures = 0;
#define CHECK(cond)                                                     \
    do                                                                  \
    {                                                                   \
        if (!(cond))                                                    \
        {                                                               \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static long live = 0, obtained = 0, copiedBytes = 0;
static unsigned long long refuseAbove = ~0ULL;  // allocations larger than this fail (device memory exhausted)
static void* fakeObtain(int, unsigned long long bytes)
{
    if (bytes > refuseAbove) return nullptr;
    ++live;
    ++obtained;
    return std::malloc(bytes);
}
static void fakeRelease(void* p)
{
    --live;
    std::free(p);
}
static int fakeCopy(void* dst, const void* src, unsigned long long bytes)
{
    std::memcpy(dst, src, bytes);
    copiedBytes += static_cast<long>(bytes);
    return 0;
}
static int fakeCompact(int, void* steps, long long n, long long cells, int burn, int interval, long long* kept)
{
    double* base = static_cast<double*>(steps);
    *kept = mcmcpp::chain_compact_kept(n, burn, interval);
    mcmcpp::ChainCompactWave w;
    for (std::int64_t done = 0; mcmcpp::chain_compact_wave(done, *kept, burn, interval, &w); done = w.first + w.count)
        for (std::int64_t j = w.first; j < w.first + w.count; ++j)
            std::memcpy(base + j * cells, base + mcmcpp::chain_compact_source(j, burn, interval) * cells, sizeof(double) * cells);
    return 0;
}

static Detail::BlockMemory fake() { return Detail::BlockMemory::onDevice(-1, &fakeObtain, &fakeRelease, &fakeCopy, &fakeCompact); }

static void fill(double* dst, std::int64_t firstStep, std::int64_t count, std::int64_t cells)
{
    for (std::int64_t s = 0; s < count; ++s)
        for (std::int64_t c = 0; c < cells; ++c) dst[s * cells + c] = static_cast<double>((firstStep + s) * 1000 + c);
}

// what a run does: reserve, then write whole steps at the pointer handed out, then commit
static bool run(Chain<double>& chain, std::int64_t steps, std::int64_t* made)
{
    std::int64_t left = steps;
    chain.reserveSteps(left);
    while (left > 0)
    {
        std::int64_t room = 0;
        double* dst = chain.stepsContiguousFrom(&room);
        if (!dst || room < 1) return false;
        const std::int64_t now = left < room ? left : room;
        chain.expectSteps(now);
        fill(dst, *made, now, chain.getCellsPerStep());
        *made += now;
        chain.commitSteps(now);
        left -= now;
        if (chain.remainingSteps() == 0) return false;
    }
    return true;
}

static void same(Chain<double>& a, Chain<double>& b)
{
    CHECK(a.getStoredStepCount() == b.getStoredStepCount());
    ChainStepIterator<double> x = a.getStepIteratorBegin(), y = b.getStepIteratorBegin();
    for (; x != a.getStepIteratorEnd() && y != b.getStepIteratorEnd(); ++x, ++y)
        CHECK(std::memcmp(*x, *y, sizeof(double) * static_cast<size_t>(a.getCellsPerStep())) == 0);
    CHECK(x == a.getStepIteratorEnd() && y == b.getStepIteratorEnd());
    ChainPsetIterator<double> p = a.getPsetIteratorBegin(), q = b.getPsetIteratorBegin();
    for (; p != a.getPsetIteratorEnd() && q != b.getPsetIteratorEnd(); ++p, ++q)
        CHECK(std::memcmp(*p, *q, sizeof(double) * static_cast<size_t>(a.getCellsPerWalker())) == 0);
    CHECK(p == a.getPsetIteratorEnd() && q == b.getPsetIteratorEnd());
}

int main()
{
    const int W = 6, D = 3;
    const unsigned long long stepBytes = sizeof(double) * W * D;
    {
        // reserve, grow by doubling, commit
        Chain<double> dev(W, D, 1000 * stepBytes, Detail::DefaultBlockBytes, fake()), host(W, D, 1000 * stepBytes);
        CHECK(dev.memoryKind() == Detail::MemoryKind::Device && host.memoryKind() == Detail::MemoryKind::Heap);
        CHECK(dev.deviceSteps().base == nullptr && dev.deviceSteps().steps == 0 && host.deviceSteps().base == nullptr);
        dev.setFirstDeviceReservation(8);
        std::vector<double> first(W * D);
        fill(first.data(), 0, 1, W * D);
        for (int w = 0; w < W; ++w)
        {
            dev.storeWalker(w, first.data() + w * D);
            host.storeWalker(w, first.data() + w * D);
        }
        CHECK(dev.incrementChainStep() == IncrementStatus::NormalIncrement);
        host.incrementChainStep();
        CHECK(obtained == 1 && live == 1);
        std::int64_t madeDev = 1, madeHost = 1;
        CHECK(run(dev, 5, &madeDev) && run(host, 5, &madeHost));
        CHECK(obtained == 1);  // 6 steps fit the first reservation of 8
        const double* before = dev.deviceSteps().base;
        CHECK(run(dev, 5, &madeDev) && run(host, 5, &madeHost));
        CHECK(obtained == 2 && live == 1 && dev.deviceSteps().base != before);  // 11 > 8: one allocation of 16, the old one given back
        CHECK(run(dev, 5, &madeDev) && run(host, 5, &madeHost));
        CHECK(obtained == 2 && dev.deviceSteps().steps == 16);
        CHECK(run(dev, 30, &madeDev) && run(host, 30, &madeHost));  // 46 > 32: to what is needed
        CHECK(obtained == 3 && live == 1);
        same(dev, host);
        CHECK(dev.hostBytesFetched() == 46 * stepBytes + 46 * stepBytes);  // once per step for each of the two iterators
        // the same step again costs nothing; another step costs one step
        const unsigned long long fetched = dev.hostBytesFetched();
        ChainStepIterator<double> it = dev.getStepIteratorBegin();
        it += 7;
        const double* p = *it;
        CHECK(p[0] == 7000.0 && *it == p && dev.hostBytesFetched() == fetched + stepBytes);
        // iterator arithmetic touches no memory and saturates at both ends
        ChainStepIterator<double> jt = dev.getStepIteratorBegin();
        jt += 1000;
        CHECK(jt == dev.getStepIteratorEnd());
        jt -= 1000;
        CHECK(jt == dev.getStepIteratorBegin());
        --jt;
        CHECK(jt == dev.getStepIteratorBegin() && jt.stepIndex() == 0);
        ChainPsetIterator<double> pt = dev.getPsetIteratorEnd();
        ++pt;
        CHECK(pt == dev.getPsetIteratorEnd());
        CHECK(dev.hostBytesFetched() == fetched + stepBytes);
        CHECK(*dev.getStepIteratorEnd() == nullptr);  // nothing is stored there: nothing is fetched
        // compaction, every case of the suite, each mirrored on the host chain
        const int cases[6][2] = {{0, 1}, {20, 1}, {0, 5}, {7, 3}, {45, 1}, {3, 46}};
        for (int c = 0; c < 6; ++c)
        {
            Chain<double> d2(W, D, 1000 * stepBytes, Detail::DefaultBlockBytes, fake()), h2(W, D, 1000 * stepBytes);
            std::int64_t a = 0, b = 0;
            CHECK(run(d2, 46, &a) && run(h2, 46, &b));
            const unsigned long long f = d2.hostBytesFetched();
            d2.resetChainForSubSampling(cases[c][0], cases[c][1]);
            h2.resetChainForSubSampling(cases[c][0], cases[c][1]);
            CHECK(d2.hostBytesFetched() == f);
            same(d2, h2);
            CHECK(run(d2, 3, &a) && run(h2, 3, &b));  // and the chain goes on behind the kept steps
            same(d2, h2);
        }
        // every small (n, burn, interval) against a copy to a fresh array
        for (int n = 0; n <= 24; ++n)
            for (int burn = 0; burn <= n; ++burn)
                for (int interval = 1; interval <= 7; ++interval)
                {
                    Chain<double> d3(2, 1, 1000 * stepBytes, Detail::DefaultBlockBytes, fake()), h3(2, 1, 1000 * stepBytes);
                    std::int64_t a = 0, b = 0;
                    if (n > 0) CHECK(run(d3, n, &a) && run(h3, n, &b));
                    d3.resetChainForSubSampling(burn, interval);
                    h3.resetChainForSubSampling(burn, interval);
                    same(d3, h3);
                }
        // reset keeps the memory
        const long allocations = obtained;
        dev.resetChain();
        host.resetChain();
        CHECK(dev.getStoredStepCount() == 0 && dev.deviceSteps().steps == 0);
        madeDev = madeHost = 0;
        CHECK(run(dev, 40, &madeDev) && run(host, 40, &madeHost));
        CHECK(obtained == allocations);
        same(dev, host);
    }
    CHECK(live == 0);  // the one owner gave everything back
    {
        // the byte budget: both chains report false at the same stored-step count
        Chain<double> dev(W, D, 10 * stepBytes, Detail::DefaultBlockBytes, fake()), host(W, D, 10 * stepBytes);
        std::int64_t a = 0, b = 0;
        CHECK(run(dev, 4, &a) && run(host, 4, &b));
        CHECK(!run(dev, 20, &a) && !run(host, 20, &b));
        CHECK(dev.getStoredStepCount() == 10 && host.getStoredStepCount() == 10 && a == b);
        CHECK(!run(dev, 1, &a) && !run(host, 1, &b));
        CHECK(dev.stepsContiguousFrom(nullptr) == nullptr);
        same(dev, host);
    }
    {
        // device memory that runs out before the budget: the doubling falls back to what is needed, then the run reports false
        Chain<double> dev(W, D, 1000 * stepBytes, Detail::DefaultBlockBytes, fake());
        std::int64_t a = 0;
        CHECK(run(dev, 8, &a));
        refuseAbove = 12 * stepBytes;
        CHECK(run(dev, 2, &a));   // 10 steps: 16 refused, 10 granted
        CHECK(run(dev, 2, &a));   // 12 steps: 20 refused, 12 granted
        CHECK(!run(dev, 2, &a));  // 14: refused; the chain keeps its 12 steps
        CHECK(dev.getStoredStepCount() == 12 && a == 12);
        ChainStepIterator<double> it = dev.getStepIteratorBegin();
        it += 11;
        CHECK((*it)[0] == 11000.0);
        refuseAbove = ~0ULL;
    }
    CHECK(live == 0);
    if (failures == 0) std::printf("device_chain_host OK\n");
    return failures == 0 ? 0 : 1;
}
