/*
 * Chain/ChainBlock.h -- one contiguous slab of stored ensemble steps.
 *
 * Output format kept from the reference (/root/reference/MCMCpp/Chain/ChainBlock.h:125-131): positions
 * only, cell = step*W*D + walker*D + param, every step holds all W walkers.  Unlike the reference's fixed
 * 10 000-step blocks indexed with 32-bit int (ChainBlock.h:31,115-123 -- the size product overflows at
 * 16 384 x 32 and above), a block here is sized in bytes and indexed with 64-bit integers.
 */
#ifndef MCMCPP_CHAIN_CHAINBLOCK_H
#define MCMCPP_CHAIN_CHAINBLOCK_H

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace MCMC
{
namespace Chain
{
namespace Detail
{
/// Default slab size; the number of steps per block follows from it and the ensemble size.
static const unsigned long long DefaultBlockBytes = 256ULL << 20;

/// The three kinds of memory a Chain keeps its stored steps in.
enum class MemoryKind : char
{
    Heap,    ///< the default
    Pinned,  ///< blocks from a provider (the samplers: pinned host memory, MCMCPP_CHAIN_MEMORY=pinned)
    Device   ///< ONE contiguous allocation of GPU memory (MCMCPP_CHAIN_MEMORY=device): the chain never crosses the host link
};

/// Where a block's memory comes from.  The default is the heap (64-byte aligned like the reference's autoAlignedAlloc,
/// Utility/Misc.h:77-102); the MI355X samplers hand out pinned host memory (mcmcpp_hip_host_alloc) so that the step
/// launches write stored steps straight into the block.  A failed `obtain` falls back to the heap.
/// A device chain (onDevice) takes its allocation from obtainOn / release, moves bytes with copy (host or device memory on
/// either side; 0 = done) and compacts itself with compact (Chain::resetChainForSubSampling in place; 0 = done).  The
/// samplers bind the four to the C ABI (mcmcpp_hip_device_alloc / _free / _copy / _chain_compact); this header needs none of it.
struct BlockMemory
{
    void* (*obtain)(unsigned long long bytes);
    void (*release)(void*);
    void* (*obtainOn)(int device, unsigned long long bytes);
    int (*copy)(void* dst, const void* src, unsigned long long bytes);
    int (*compact)(int device, void* steps, long long numSteps, long long cellsPerStep, int burnIn, int interval, long long* kept);
    int device;  ///< device ordinal of a device chain (-1: the current device)
    MemoryKind kind;
    BlockMemory() : obtain(nullptr), release(nullptr), obtainOn(nullptr), copy(nullptr), compact(nullptr), device(-1), kind(MemoryKind::Heap) {}
    BlockMemory(void* (*get)(unsigned long long), void (*put)(void*))
        : obtain(get), release(put), obtainOn(nullptr), copy(nullptr), compact(nullptr), device(-1), kind(get && put ? MemoryKind::Pinned : MemoryKind::Heap)
    {
    }
    static BlockMemory onDevice(int deviceOrdinal, void* (*get)(int, unsigned long long), void (*put)(void*),
                                int (*move)(void*, const void*, unsigned long long),
                                int (*compactFn)(int, void*, long long, long long, int, int, long long*))
    {
        BlockMemory m;
        m.obtainOn = get;
        m.release = put;
        m.copy = move;
        m.compact = compactFn;
        m.device = deviceOrdinal;
        m.kind = MemoryKind::Device;
        return m;
    }
};

/// The one owner of a device chain's allocation: `capacity` steps behind `cells`, given back by the destructor.  Move-only.
template <class ParamType>
class DeviceSlab
{
public:
    DeviceSlab() : cells(nullptr), capacitySteps(0), releaseFn(nullptr) {}
    DeviceSlab(const BlockMemory& mem, std::int64_t steps, std::int64_t cellsInStep) : cells(nullptr), capacitySteps(0), releaseFn(mem.release)
    {
        if (steps < 1 || !mem.obtainOn || !mem.release) return;
        cells = static_cast<ParamType*>(mem.obtainOn(mem.device, static_cast<unsigned long long>(steps) * static_cast<unsigned long long>(cellsInStep) * sizeof(ParamType)));
        if (cells) capacitySteps = steps;
    }
    ~DeviceSlab()
    {
        if (cells) releaseFn(cells);
    }
    DeviceSlab(const DeviceSlab&) = delete;
    DeviceSlab& operator=(const DeviceSlab&) = delete;
    DeviceSlab(DeviceSlab&& o) : cells(o.cells), capacitySteps(o.capacitySteps), releaseFn(o.releaseFn)
    {
        o.cells = nullptr;
        o.capacitySteps = 0;
    }
    DeviceSlab& operator=(DeviceSlab&& o)  // (o gives back what this held)
    {
        ParamType* c = cells;
        cells = o.cells;
        o.cells = c;
        const std::int64_t n = capacitySteps;
        capacitySteps = o.capacitySteps;
        o.capacitySteps = n;
        void (*r)(void*) = releaseFn;
        releaseFn = o.releaseFn;
        o.releaseFn = r;
        return *this;
    }
    bool valid() const { return cells != nullptr; }
    ParamType* get() const { return cells; }
    std::int64_t capacity() const { return capacitySteps; }

private:
    ParamType* cells;  ///< DEVICE memory: never dereferenced on the host
    std::int64_t capacitySteps;
    void (*releaseFn)(void*);
};
}

template <class ParamType>
class ChainBlock
{
public:
    /// touchPages: write to every page of a heap block now (the Chain does this on the thread that obtains blocks ahead of
    /// their use, so that the first-touch page faults -- about 45 ms per 256 MiB -- are not paid by whoever fills the block)
    ChainBlock(std::int64_t stepsInBlock, std::int64_t cellsInStep, const Detail::BlockMemory& mem = Detail::BlockMemory(), bool touchPages = false)
        : capacitySteps(stepsInBlock), cellsPerStep(cellsInStep), usedSteps(0), cells(nullptr), releaseFn(nullptr)
    {
        const std::size_t bytes = static_cast<std::size_t>(capacitySteps) * static_cast<std::size_t>(cellsPerStep) * sizeof(ParamType);
        void* p = nullptr;
        if (mem.obtain && mem.release) p = mem.obtain(bytes ? bytes : 64);
        if (p)
            releaseFn = mem.release;
        else if (posix_memalign(&p, 64, bytes ? bytes : 64) != 0)
            p = nullptr;
        else if (touchPages)
            for (std::size_t off = 0; off < bytes; off += 4096) static_cast<volatile char*>(p)[off] = 0;
        cells = static_cast<ParamType*>(p);
    }
    ~ChainBlock()
    {
        if (releaseFn)
            releaseFn(cells);
        else
            std::free(cells);
    }
    ChainBlock(const ChainBlock&) = delete;
    ChainBlock& operator=(const ChainBlock&) = delete;

    bool valid() const { return cells != nullptr; }
    bool full() const { return usedSteps >= capacitySteps; }
    std::int64_t capacity() const { return capacitySteps; }
    std::int64_t used() const { return usedSteps; }
    void setUsed(std::int64_t n) { usedSteps = n; }
    ParamType* step(std::int64_t k) { return cells + static_cast<std::size_t>(k) * static_cast<std::size_t>(cellsPerStep); }
    const ParamType* step(std::int64_t k) const { return cells + static_cast<std::size_t>(k) * static_cast<std::size_t>(cellsPerStep); }

private:
    std::int64_t capacitySteps;
    std::int64_t cellsPerStep;
    std::int64_t usedSteps;
    ParamType* cells;
    void (*releaseFn)(void*);
};

}  // namespace Chain
}  // namespace MCMC
#endif  // MCMCPP_CHAIN_CHAINBLOCK_H
