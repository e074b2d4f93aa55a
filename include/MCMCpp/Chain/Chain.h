/*
 * Chain/Chain.h -- the sampler's output: every stored ensemble step, walker-major.
 *
 * Same role and cell layout as the reference's Chain (/root/reference/MCMCpp/Chain/Chain.h:61-151): the
 * sampler stores one full step at a time, users read it back through ChainStepIterator (W*D contiguous
 * values per step) or ChainPsetIterator (D values per walker).  Differences, all deliberate:
 *   - 64-bit step and cell indices and byte-sized blocks (the reference overflows 32-bit int at the
 *     BASELINE ensemble sizes, ChainBlock.h:31,116-128);
 *   - whole steps arrive from the GPU, so besides the reference's per-walker storeWalker() there is a bulk
 *     path (stepsContiguousFrom / commitSteps) that lets the device-to-host copy land in place;
 *   - iterators address steps by global index instead of walking a linked list, which removes the
 *     off-by-one defects of the reference's ChainPsetIterator (ChainPsetIterator.h:131-142,154);
 *   - a third memory kind besides heap and pinned blocks: a DEVICE chain (Detail::BlockMemory::onDevice) is ONE contiguous
 *     allocation [steps][W][D] of GPU memory, which the sampler's run writes in place and the analysis classes read in place
 *     (deviceSteps()).  It grows by doubling, bounded by the same byte budget, and is compacted in place by a kernel.  The
 *     iterators still hand out host pointers: dereferencing one downloads that step into a buffer the chain owns, keyed by
 *     step index (the pointer holds until a different step is dereferenced), and hostBytesFetched() counts those bytes.
 */
#ifndef MCMCPP_CHAIN_CHAIN_H
#define MCMCPP_CHAIN_CHAIN_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <vector>

#include "ChainBlock.h"
#include "ChainPsetIterator.h"
#include "ChainStepIterator.h"

namespace MCMC
{
namespace Chain
{

/// Result of advancing the chain by one stored step (names as in the reference, Chain.h:34-38).
enum class IncrementStatus : char
{
    NormalIncrement,  ///< stayed inside the current block
    NewBlock,         ///< the next step will land in a fresh block
    EndOfChain        ///< the byte budget is exhausted: nothing more can be stored
};

/// A device chain's stored steps where they lie: `steps` committed steps of W*D values each behind `base` (DEVICE memory).
template <class ParamType>
struct DeviceSteps
{
    ParamType* base;
    std::int64_t steps;
};

template <class ParamType>
class Chain
{
public:
    typedef ChainPsetIterator<ParamType> PsetIterator;
    typedef ChainStepIterator<ParamType> StepIterator;

    /// maxSize: byte budget for stored steps (the reference's maxChainSizeBytes).  At least one step is always storable.
    Chain(int numWalkers, int numParams, unsigned long long maxSize, unsigned long long blockBytes = Detail::DefaultBlockBytes,
          const Detail::BlockMemory& memory = Detail::BlockMemory())
        : blockMemory(memory), walkerCount(numWalkers), cellsPerWalker(numParams),
          cellsPerStep(static_cast<std::int64_t>(numWalkers) * numParams), stepCount(0), firstReserve(0), fetchedStep(-1), fetchedBytes(0)
    {
        const unsigned long long stepBytes = static_cast<unsigned long long>(cellsPerStep) * sizeof(ParamType);
        maxSteps = static_cast<std::int64_t>(maxSize / stepBytes);
        if (maxSteps < 1) maxSteps = 1;
        stepsPerBlock = static_cast<std::int64_t>(blockBytes / stepBytes);
        if (stepsPerBlock < 1) stepsPerBlock = 1;
        if (stepsPerBlock > maxSteps) stepsPerBlock = maxSteps;
    }
    ~Chain()
    {
        if (nextBlock.valid()) delete nextBlock.get();
        for (ChainBlock<ParamType>* b : blocks) delete b;
    }
    Chain(const Chain&) = delete;
    Chain& operator=(const Chain&) = delete;

    // ---- writing, one walker at a time (reference API: Chain.h:93,204-236) ---------------------------
    /// Copy one walker's parameters into the step being assembled.
    void storeWalker(int walkerNum, const ParamType* walkerData)
    {
        if (onDevice())  // (assembled on the host; incrementChainStep uploads it)
        {
            if (assembling.empty()) assembling.resize(static_cast<std::size_t>(cellsPerStep));
            std::memcpy(assembling.data() + static_cast<std::size_t>(walkerNum) * cellsPerWalker, walkerData, sizeof(ParamType) * cellsPerWalker);
            return;
        }
        ParamType* dst = writableStep();
        if (dst) std::memcpy(dst + static_cast<std::size_t>(walkerNum) * cellsPerWalker, walkerData, sizeof(ParamType) * cellsPerWalker);
    }
    /// Close the step being assembled.
    IncrementStatus incrementChainStep()
    {
        if (stepCount >= maxSteps) return IncrementStatus::EndOfChain;
        if (onDevice())
        {
            if (!reserveSteps(1)) return IncrementStatus::EndOfChain;
            if (assembling.empty()) assembling.resize(static_cast<std::size_t>(cellsPerStep));
            deviceCopy(deviceStep(stepCount), assembling.data(), 1);
            ++stepCount;
            return stepCount >= maxSteps ? IncrementStatus::EndOfChain : IncrementStatus::NormalIncrement;
        }
        if (!writableStep()) return IncrementStatus::EndOfChain;
        ++stepCount;
        blocks[static_cast<std::size_t>((stepCount - 1) / stepsPerBlock)]->setUsed((stepCount - 1) % stepsPerBlock + 1);
        if (prefetchBlocks) maybePrefetch(stepCount);
        if (stepCount >= maxSteps) return IncrementStatus::EndOfChain;
        return (stepCount % stepsPerBlock == 0) ? IncrementStatus::NewBlock : IncrementStatus::NormalIncrement;
    }

    // ---- writing, whole steps at once (device-to-host copies land here) -------------------------------
    /// Room left under the byte budget.
    std::int64_t remainingSteps() const { return maxSteps - stepCount; }
    /// Pointer where the next stored step goes and how many consecutive steps fit there contiguously (0 when full).
    ParamType* stepsContiguousFrom(std::int64_t* contiguous)
    {
        if (onDevice())  // a DEVICE pointer: behind the committed steps, as far as the allocation reaches
        {
            const bool room = stepCount < maxSteps && reserveSteps(1);
            if (contiguous) *contiguous = room ? slab.capacity() - stepCount : 0;
            return room ? deviceStep(stepCount) : nullptr;
        }
        ParamType* p = (stepCount < maxSteps) ? writableStep() : nullptr;
        if (contiguous)
        {
            std::int64_t room = p ? stepsPerBlock - stepCount % stepsPerBlock : 0;
            if (room > maxSteps - stepCount) room = maxSteps - stepCount;
            *contiguous = room;
        }
        return p;
    }
    /// Announce that `count` steps are about to be written at the pointer handed out by stepsContiguousFrom (a device run
    /// in progress): lets the block behind the current one be obtained while they are being made.
    void expectSteps(std::int64_t count)
    {
        if (prefetchBlocks) maybePrefetch(stepCount + count);
    }
    /// Declare `count` steps written at the pointer handed out by stepsContiguousFrom.
    void commitSteps(std::int64_t count)
    {
        if (onDevice())
        {
            stepCount = (count > slab.capacity() - stepCount) ? slab.capacity() : stepCount + count;
            return;
        }
        for (std::int64_t k = 0; k < count; ++k) incrementChainStep();
    }

    /// A device chain makes room for `count` more steps now (a run knows how many it stores before it launches): the
    /// allocation grows to what is needed or to twice its size, whichever is more, within the byte budget, and the committed
    /// steps are copied over inside device memory.  False when not even one more step fits (budget or device memory
    /// exhausted).  Host chains obtain their blocks as they go: nothing to do, true.
    bool reserveSteps(std::int64_t count)
    {
        if (!onDevice()) return true;
        std::int64_t need = (count > maxSteps - stepCount) ? maxSteps : stepCount + count;
        if (need <= slab.capacity()) return slab.capacity() > stepCount;
        std::int64_t want = slab.valid() ? 2 * slab.capacity() : firstReserve;
        if (want < need) want = need;
        if (want > maxSteps) want = maxSteps;
        Detail::DeviceSlab<ParamType> bigger(blockMemory, want, cellsPerStep);
        if (!bigger.valid() && want > need) bigger = Detail::DeviceSlab<ParamType>(blockMemory, need, cellsPerStep);
        if (!bigger.valid()) return slab.capacity() > stepCount;
        if (stepCount > 0) deviceCopy(bigger.get(), slab.get(), stepCount);
        slab = static_cast<Detail::DeviceSlab<ParamType>&&>(bigger);  // (the old allocation goes with `bigger`)
        return true;
    }
    /// Steps the first allocation of a device chain holds at the least (the samplers' test knob; 0: what is asked for).
    void setFirstDeviceReservation(std::int64_t steps) { firstReserve = steps; }

    /// Obtain every block one block ahead of its use, on a helper thread (the samplers switch this on; off by default so
    /// that a Chain used alone never starts a thread).
    void setBlockPrefetch(bool on) { prefetchBlocks = on; }

    // ---- bookkeeping -------------------------------------------------------------------------------------
    std::int64_t getStoredStepCount() const { return stepCount; }
    std::int64_t getMaxStepCount() const { return maxSteps; }
    int getWalkerCount() const { return walkerCount; }
    int getCellsPerWalker() const { return cellsPerWalker; }
    std::int64_t getCellsPerStep() const { return cellsPerStep; }
    /// Heap, pinned blocks, or one device allocation.
    Detail::MemoryKind memoryKind() const { return blockMemory.kind; }
    /// A device chain's committed steps in place (base == nullptr for a host chain, or before anything is stored).
    DeviceSteps<ParamType> deviceSteps() const
    {
        DeviceSteps<ParamType> d;
        d.base = onDevice() ? slab.get() : nullptr;
        d.steps = onDevice() ? stepCount : 0;
        return d;
    }
    /// Device ordinal of a device chain (-1: the current device).
    int deviceOrdinal() const { return blockMemory.device; }
    /// Bytes copied from a device chain to the host so far (by dereferencing iterators / stepPtr).  0 for host chains.
    unsigned long long hostBytesFetched() const { return fetchedBytes; }

    /// Forget every stored step, keep the memory (reference: Chain.h:255-266).
    void resetChain()
    {
        stepCount = 0;
        fetchedStep = -1;
        for (ChainBlock<ParamType>* b : blocks) b->setUsed(0);
        if (nextBlock.valid()) delete nextBlock.get();  // (a block obtained ahead of a chain that starts over)
    }

    /// Drop `burnInSamples` leading steps, then keep every `interval`-th of the rest, compacting in place
    /// (reference: Chain.h:268-305, same special cases).
    void resetChainForSubSampling(int burnInSamples, int interval)
    {
        if (onDevice())  // the same selection, applied in place by a kernel; nothing comes to the host
        {
            long long kept = stepCount;
            if (stepCount > 0 && blockMemory.compact(blockMemory.device, slab.get(), stepCount, cellsPerStep, burnInSamples, interval, &kept) != 0)
                deviceDie("compacting");
            stepCount = kept;
            fetchedStep = -1;
            return;
        }
        if (burnInSamples == 0 && interval == 1) return;
        if (stepCount <= burnInSamples || (stepCount - burnInSamples) < interval)
        {
            resetChain();
            return;
        }
        const std::int64_t stored = stepCount;
        std::int64_t kept = 0;
        for (std::int64_t src = burnInSamples; src < stored; src += interval, ++kept)
            if (src != kept) std::memmove(stepPtr(kept), stepPtr(src), sizeof(ParamType) * static_cast<std::size_t>(cellsPerStep));
        stepCount = kept;
        for (std::size_t b = 0; b < blocks.size(); ++b)
        {
            const std::int64_t lo = static_cast<std::int64_t>(b) * stepsPerBlock;
            std::int64_t used = stepCount - lo;
            if (used < 0) used = 0;
            if (used > stepsPerBlock) used = stepsPerBlock;
            blocks[b]->setUsed(used);
        }
    }

    // ---- reading ---------------------------------------------------------------------------------------------
    PsetIterator getPsetIteratorBegin() { return PsetIterator(this, 0); }
    PsetIterator getPsetIteratorEnd() { return PsetIterator(this, stepCount * walkerCount); }
    StepIterator getStepIteratorBegin() { return StepIterator(this, 0); }
    StepIterator getStepIteratorEnd() { return StepIterator(this, stepCount); }

    /// W*D contiguous values of stored step k (k < getStoredStepCount()).
    ParamType* stepPtr(std::int64_t k)
    {
        if (onDevice())  // a HOST copy of that step, downloaded unless it is the one downloaded last
        {
            if (k < 0 || k >= stepCount) return nullptr;
            if (k != fetchedStep)
            {
                if (fetched.empty()) fetched.resize(static_cast<std::size_t>(cellsPerStep));
                deviceCopy(fetched.data(), deviceStep(k), 1);
                fetchedStep = k;
                fetchedBytes += static_cast<unsigned long long>(cellsPerStep) * sizeof(ParamType);
            }
            return fetched.data();
        }
        return blocks[static_cast<std::size_t>(k / stepsPerBlock)]->step(k % stepsPerBlock);
    }

private:
    bool onDevice() const { return blockMemory.kind == Detail::MemoryKind::Device; }
    ParamType* deviceStep(std::int64_t k) const { return slab.get() + static_cast<std::size_t>(k) * static_cast<std::size_t>(cellsPerStep); }
    void deviceCopy(void* dst, const void* src, std::int64_t steps)
    {
        if (blockMemory.copy(dst, src, static_cast<unsigned long long>(steps) * static_cast<unsigned long long>(cellsPerStep) * sizeof(ParamType)) != 0)
            deviceDie("copying steps of");
    }
    static void deviceDie(const char* what)
    {
        std::fprintf(stderr, "MCMCpp (MI355X): %s the device chain failed\n", what);
        std::abort();
    }

    /// Once the last block is half full, obtain the one behind it on a helper thread (a run that never gets that far never
    /// pays for a block it does not use).
    void maybePrefetch(std::int64_t stepsSoon)
    {
        if (nextBlock.valid() || blocks.empty()) return;
        const std::int64_t lastLo = static_cast<std::int64_t>(blocks.size() - 1) * stepsPerBlock;
        if (stepsSoon - lastLo < (blocks.back()->capacity() + 1) / 2) return;
        const std::int64_t nextLo = static_cast<std::int64_t>(blocks.size()) * stepsPerBlock;
        std::int64_t nextWant = stepsPerBlock;
        if (nextLo + nextWant > maxSteps) nextWant = maxSteps - nextLo;
        if (nextWant < 1) return;
        const std::int64_t cells = cellsPerStep;
        const Detail::BlockMemory mem = blockMemory;
        nextBlock = std::async(std::launch::async, [nextWant, cells, mem]() { return new ChainBlock<ParamType>(nextWant, cells, mem, true); });
    }

    /// The step being assembled (allocating its block on first use); nullptr when memory is exhausted.
    ParamType* writableStep()
    {
        const std::size_t b = static_cast<std::size_t>(stepCount / stepsPerBlock);
        while (blocks.size() <= b)
        {
            std::int64_t want = stepsPerBlock;
            const std::int64_t lo = static_cast<std::int64_t>(blocks.size()) * stepsPerBlock;
            if (lo + want > maxSteps) want = maxSteps - lo;
            if (want < 1) return nullptr;
            // A block is obtained ahead, on a thread of its own, while the sampler fills the second half of the current one: pinned
            // memory from a provider costs some 35 ms per 256 MiB block, heap memory as much in first-touch page faults
            // (which that thread takes by writing to every page).
            ChainBlock<ParamType>* nb = nullptr;
            if (nextBlock.valid())
            {
                nb = nextBlock.get();
                if (nb && nb->capacity() != want)
                {
                    delete nb;
                    nb = nullptr;
                }
            }
            if (!nb) nb = new ChainBlock<ParamType>(want, cellsPerStep, blockMemory);
            if (!nb->valid())
            {
                delete nb;
                return nullptr;
            }
            blocks.push_back(nb);
        }
        return blocks[b]->step(stepCount % stepsPerBlock);
    }

    std::vector<ChainBlock<ParamType>*> blocks;
    std::future<ChainBlock<ParamType>*> nextBlock;  ///< the block behind the last one, being obtained
    bool prefetchBlocks = false;                    ///< obtain blocks one ahead on a helper thread (setBlockPrefetch)
    Detail::BlockMemory blockMemory;
    int walkerCount;
    int cellsPerWalker;
    std::int64_t cellsPerStep;
    std::int64_t stepsPerBlock;
    std::int64_t maxSteps;
    std::int64_t stepCount;
    // ---- a device chain (blockMemory.kind == Device) uses these instead of blocks ----
    Detail::DeviceSlab<ParamType> slab;  ///< the one allocation: its only owner
    std::int64_t firstReserve;           ///< steps the first allocation holds at the least
    std::vector<ParamType> assembling;   ///< the step storeWalker assembles, on the host
    std::vector<ParamType> fetched;      ///< host copy of stored step `fetchedStep`
    std::int64_t fetchedStep;
    unsigned long long fetchedBytes;
};

}  // namespace Chain
}  // namespace MCMC
#endif  // MCMCPP_CHAIN_CHAIN_H
