/*
 * Device/SamplerCore.h -- what EnsembleSampler and ParallelEnsembleSampler share on the MI355X path.
 *
 * Reference behaviour kept (paths relative to /root/reference/MCMCpp):
 *   - walkers [0, W/2) are the red set, [W/2, W) the black set; chain slot = walker index  (EnsembleSampler.h:211-215)
 *   - setInitialWalkerPos stores the initial placement as chain step 0 and counts it as one accepted
 *     step per walker                                                       (EnsembleSampler.h:220-230, Walker/Walker.h:76,162-170)
 *   - runMCMC(n): n stored steps; with sub-sampling interval k every stored step is preceded by k-1
 *     unstored ensemble steps; returns false once the chain's byte budget is exhausted   (EnsembleSampler.h:284-310)
 *   - the PostStepAction runs once per ensemble step and sees the chain without the step being made
 *                                                                            (EnsembleSampler.h:291-293,356-359)
 *   - reset() forgets chain and counters, keeps positions and the random stream          (EnsembleSampler.h:312-322)
 * Beyond the reference: with MCMCPP_CHAIN_MEMORY=device the chain is one allocation of GPU memory (Chain/Chain.h).  The run
 * then stores through mcmcpp_hip_run_device, sliceAndBurnChain compacts it with a kernel and the analysis classes read it in
 * place: no stored step crosses the host link unless an iterator is dereferenced.
 * Not kept: the parallel sampler's run-to-run non-determinism (ParallelEnsembleSampler.h:71-76) and its
 * sub-sampling defect (Threading/RedBlkCtrlerSpinLock.h:297-300) -- both samplers follow the sequential
 * trajectory, the only reproducible one.
 */
#ifndef MCMCPP_DEVICE_SAMPLERCORE_H
#define MCMCPP_DEVICE_SAMPLERCORE_H

#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../Chain/Chain.h"
#include "../Utility/NoAction.h"
#include "../Utility/UserOjbectsTest.h"
#include "Calculators.h"
#include "GaussianBridge.h"
#include "HipBackend.h"

namespace MCMC
{
namespace Device
{

namespace Detail
{
/// How a Calculator reaches the device: a device functor named by hipCalcId with a parameter blob (the default), or a
/// batch target whose hipBatchLogPostProb the library calls back once per half-step (MCMCPP_HIP_CALC_BATCH).
template <class Calc, class ParamType, bool Batch = Utility::CheckBatchCalculator<Calc, ParamType>::value>
struct CalcBinding
{
    static const ParamType* params(const Calc& c) { return c.hipParams(); }
    static int paramCount(const Calc& c) { return c.hipParamCount(); }
    static void bind(const HipHandle&, Calc&) {}
};
template <class Calc, class ParamType>
struct CalcBinding<Calc, ParamType, true>
{
    static_assert(Calc::hipCalcId == BatchCalcId, "a Calculator with hipBatchLogPostProb declares hipCalcId = MCMC::Device::BatchCalcId");
    static const ParamType* params(const Calc&) { return nullptr; }
    static int paramCount(const Calc&) { return 0; }
    static int call(void* user, const void* proposals, void* logpOut, std::int64_t count, std::int32_t numParams, void* hipStream)
    {
        return static_cast<Calc*>(user)->hipBatchLogPostProb(static_cast<const ParamType*>(proposals), static_cast<long long>(count),
                                                             static_cast<int>(numParams), static_cast<ParamType*>(logpOut), hipStream);
    }
    /// the sampler's own copy of the Calculator (inside its Mover) is the callback's user pointer
    static void bind(const HipHandle& h, Calc& c)
    {
        h.check("mcmcpp_hip_set_batch_calculator", mcmcpp_hip_set_batch_calculator(h.get(), &call, &c, nullptr, nullptr));
    }
};
}  // namespace Detail

template <class ParamType, class Mover, class PostStepAction>
class SamplerCore
{
public:
    typedef Chain::Chain<ParamType> ChainType;
    typedef Chain::ChainPsetIterator<ParamType> PsetItt;
    typedef Chain::ChainStepIterator<ParamType> StepItt;

    static_assert(Mover::RunsOnDevice, "the MI355X samplers run movers that exist as device kernels: MCMC::Mover::StretchMove, MCMC::Mover::DifferentialEvolution");
    static_assert(Utility::CheckPerformAction<PostStepAction, void, const StepItt&, const StepItt&>::value,
                  "the PostStepAction needs 'void performAction(const StepItt& start, const StepItt& end)'");

    SamplerCore(int randSeed, long long stream, int numWalker, int numParameter, const Mover& move,
                unsigned long long maxChainSizeBytes, PostStepAction* stepAct, const Placement& where = Placement::fromEnvironment())
        : stepAction(stepAct),
          markovChain(numWalker, numParameter, maxChainSizeBytes, Chain::Detail::DefaultBlockBytes, chainMemory(where, numWalker, numParameter)),
          moveProposer(move), numParams(numParameter), numWalkers(numWalker), initialPlacementCounted(false)
    {
        markovChain.setBlockPrefetch(true);
        if (const char* first = std::getenv("MCMCPP_CHAIN_DEVICE_FIRST_STEPS"))  // (tests: a small first allocation, so that a short chain grows)
            markovChain.setFirstDeviceReservation(std::strtoll(first, nullptr, 10));
        assert(numWalkers % 2 == 0);             // EnsembleSampler.h:207
        assert(numWalkers > (2 * numParams));    // EnsembleSampler.h:208
        moveProposer.setPrng(randSeed, stream);  // EnsembleSampler.h:217 / RedBlkUpdater.h:86
        mcmcpp_hip_config cfg = mcmcpp_hip_config();
        cfg.struct_size = sizeof(cfg);
        cfg.dtype = HipDtype<ParamType>::value;
        cfg.num_walkers = numWalkers;
        cfg.num_params = numParams;
        cfg.calc_id = Mover::CalculatorType::hipCalcId;
        typedef Detail::CalcBinding<typename Mover::CalculatorType, ParamType> Binding;
        cfg.calc_params = Binding::params(moveProposer.getCalculator());
        cfg.calc_params_len = Binding::paramCount(moveProposer.getCalculator());
        cfg.seed = static_cast<std::uint64_t>(static_cast<long long>(randSeed));  // sign-extends like MultiSampler::setPrng
        cfg.stream = static_cast<std::uint64_t>(stream);
        cfg.gw_alpha_num = Mover::DistributionType::Numerator;
        cfg.gw_alpha_den = Mover::DistributionType::Denominator;
        cfg.mover = Mover::HipMoverId;
        const int G = where.count();
        ranks.resize(static_cast<std::size_t>(G));
        if (G == 1 && !where.splitEnsemble)
        {
            cfg.device = where.device(0);
            ranks[0].create(cfg);
            Binding::bind(ranks[0], moveProposer.getCalculator());
            return;
        }
        // One ensemble split over G devices: one handle per device, all ranks of one RCCL communicator.  The communicator's
        // rendezvous blocks until every rank has joined, so the handles are created concurrently.
        {
            // Honest about its status: the exchange logic of this path is validated (several ranks on one GPU through a
            // loop-back collective library), RCCL's transport between DIFFERENT GPUs has carried it with one rank only.
            bool distinct = false;
            for (int r = 1; r < G; ++r) distinct = distinct || where.device(r) != where.device(0);
            if (distinct && std::getenv("MCMCPP_QUIET") == nullptr)
                std::fprintf(stderr, "MCMCpp (MI355X): one ensemble split over %d GPUs -- note: this path has not yet run on multi-GPU hardware "
                                     "(DESIGN.md section 5); results are checkable against a single-GPU run, which they must equal bit for bit\n", G);
        }
        unsigned char commId[MCMCPP_HIP_COMM_ID_BYTES];
        HipHandle::checkCreate("mcmcpp_hip_comm_unique_id", mcmcpp_hip_comm_unique_id(commId));
        std::vector<std::thread> joiners;
        for (int r = 0; r < G; ++r)
            joiners.push_back(std::thread([this, cfg, r, G, &where, &commId]() {
                mcmcpp_hip_config mine = cfg;
                mine.device = where.device(r);
                mine.comm_world = G;
                mine.comm_rank = r;
                mine.comm_id = commId;
                ranks[static_cast<std::size_t>(r)].create(mine);
            }));
        for (std::thread& t : joiners) t.join();
    }

    void setInitialWalkerPos(ParamType* positions, ParamType* auxValues)
    {
        for (HipHandle& h : ranks) h.check("mcmcpp_hip_set_state", mcmcpp_hip_set_state(h.get(), positions, auxValues));
        for (int w = 0; w < numWalkers; ++w) markovChain.storeWalker(w, positions + static_cast<std::size_t>(w) * numParams);
        markovChain.incrementChainStep();
        initialPlacementCounted = true;
    }

    void storeCurrentWalkerPositions()
    {
        if (deviceChain())  // (one step, by way of the host: the chain's own upload path)
        {
            std::vector<ParamType> now(static_cast<std::size_t>(numWalkers) * numParams);
            ranks[0].check("mcmcpp_hip_get_state", mcmcpp_hip_get_state(ranks[0].get(), now.data(), nullptr, nullptr));
            for (int w = 0; w < numWalkers; ++w) markovChain.storeWalker(w, now.data() + static_cast<std::size_t>(w) * numParams);
            markovChain.incrementChainStep();
            return;
        }
        std::int64_t room = 0;
        ParamType* dst = markovChain.stepsContiguousFrom(&room);
        if (!dst || room < 1) return;
        ranks[0].check("mcmcpp_hip_get_state", mcmcpp_hip_get_state(ranks[0].get(), dst, nullptr, nullptr));
        markovChain.commitSteps(1);
    }

    /// numSteps stored steps, each the last of `interval` ensemble steps.  False when the chain filled up first.
    bool run(int numSteps, int interval)
    {
        std::int64_t left = numSteps;
        markovChain.reserveSteps(left);  // (a device chain grows once, in front of the run; host chains obtain blocks as they go)
        while (left > 0)
        {
            std::int64_t room = 0;
            ParamType* dst = markovChain.stepsContiguousFrom(&room);
            if (!dst || room < 1) return false;
            const std::int64_t now = left < room ? left : room;
            markovChain.expectSteps(now);
            if (deviceChain())
            {
                // dst is device memory: the launches store each step at its final place.  The PostStepAction sees the chain as
                // on the host path (one call per ensemble step, without the step being made); what it dereferences is downloaded.
                if (stepAction == nullptr)
                    ranks[0].check("mcmcpp_hip_run_device", mcmcpp_hip_run_device(ranks[0].get(), now, interval, dst, nullptr));
                else
                {
                    ranks[0].check("mcmcpp_hip_run_device_async", mcmcpp_hip_run_device_async(ranks[0].get(), now, interval, dst, nullptr));
                    for (std::int64_t k = 0; k < now; ++k)
                    {
                        ranks[0].check("mcmcpp_hip_wait_stored", mcmcpp_hip_wait_stored(ranks[0].get(), k + 1));
                        for (int j = 0; j < interval; ++j) stepAction->performAction(markovChain.getStepIteratorBegin(), markovChain.getStepIteratorEnd());
                        markovChain.commitSteps(1);
                    }
                    ranks[0].check("mcmcpp_hip_run_wait", mcmcpp_hip_run_wait(ranks[0].get()));
                }
                if (stepAction == nullptr) markovChain.commitSteps(now);
            }
            else if (stepAction == nullptr && ranks.size() == 1)
            {
                ranks[0].check("mcmcpp_hip_run", mcmcpp_hip_run(ranks[0].get(), now, interval, dst, nullptr));
                markovChain.commitSteps(now);
            }
            else
            {
                // Every rank steps on its handle's worker thread (a split ensemble's ranks meet in the exchanges), rank 0
                // receives the stored steps.  The PostStepAction runs here, beside the device: once per ensemble step, and
                // -- as in the reference, which calls it before the chain moves on to the next step
                // (EnsembleSampler.h:291-293,356-359) -- it sees the chain WITHOUT the step being made.  Nothing it can
                // observe changes during the interval-1 unstored steps, so their calls follow each other directly.
                for (std::size_t r = 0; r < ranks.size(); ++r)
                    ranks[r].check("mcmcpp_hip_run_async", mcmcpp_hip_run_async(ranks[r].get(), now, interval, r == 0 ? dst : nullptr, nullptr));
                for (std::int64_t k = 0; k < now; ++k)
                {
                    if (stepAction != nullptr)
                    {
                        ranks[0].check("mcmcpp_hip_wait_stored", mcmcpp_hip_wait_stored(ranks[0].get(), k + 1));
                        for (int j = 0; j < interval; ++j) stepAction->performAction(markovChain.getStepIteratorBegin(), markovChain.getStepIteratorEnd());
                        markovChain.commitSteps(1);
                    }
                }
                for (HipHandle& h : ranks) h.check("mcmcpp_hip_run_wait", mcmcpp_hip_run_wait(h.get()));
                if (stepAction == nullptr) markovChain.commitSteps(now);
            }
            left -= now;
            if (markovChain.remainingSteps() == 0) return false;  // budget reached with this step (EnsembleSampler.h:293,306)
        }
        return true;
    }

    void reset()
    {
        markovChain.resetChain();
        for (HipHandle& h : ranks) h.check("mcmcpp_hip_reset_counters", mcmcpp_hip_reset_counters(h.get()));
        initialPlacementCounted = false;
    }

    unsigned long long acceptedSteps()
    {
        unsigned long long total = 0;
        for (HipHandle& h : ranks)  // (a rank counts the walkers it updates)
        {
            std::uint64_t acc = 0;
            h.check("mcmcpp_hip_get_counters", mcmcpp_hip_get_counters(h.get(), &acc, nullptr, nullptr, nullptr));
            total += acc;
        }
        return total + (initialPlacementCounted ? static_cast<unsigned long long>(numWalkers) : 0ULL);
    }
    unsigned long long totalSteps()
    {
        std::uint64_t steps = 0;
        ranks[0].check("mcmcpp_hip_get_counters", mcmcpp_hip_get_counters(ranks[0].get(), nullptr, &steps, nullptr, nullptr));
        return static_cast<unsigned long long>(numWalkers) * (steps + (initialPlacementCounted ? 1ULL : 0ULL));
    }
    ParamType acceptanceFraction()
    {
        return static_cast<ParamType>(acceptedSteps()) / static_cast<ParamType>(totalSteps());
    }

    /// Walker positions, log-posteriors and per-walker accepted counts as they stand on the device (any may be null).
    void currentState(ParamType* positions, ParamType* logp, std::uint32_t* nAccept)
    {
        ranks[0].check("mcmcpp_hip_get_state", mcmcpp_hip_get_state(ranks[0].get(), positions, logp, nAccept));
    }
    /// Parity diagnostics of the device path (see include/mcmcpp_hip.h), summed over the devices.
    void diagnostics(std::uint64_t* nearTies, std::uint64_t* redraws)
    {
        std::uint64_t t = 0, r = 0;
        for (HipHandle& h : ranks)
        {
            std::uint64_t ht = 0, hr = 0;
            h.check("mcmcpp_hip_get_counters", mcmcpp_hip_get_counters(h.get(), nullptr, nullptr, &ht, &hr));
            t += ht;
            r += hr;
        }
        if (nearTies) *nearTies = t;
        if (redraws) *redraws = r;
    }
    int deviceCount() const { return static_cast<int>(ranks.size()); }

    /// The log-evidence of the sampled target from the chain as it stands (Device/GaussianBridge.h): a Gaussian fitted to the
    /// first half of every sliceInterval'th stored step behind the first burnIn, bridged with the second half against proposals
    /// from pcg64(seed, 0).  A device chain is read in place.  One device only: the library refuses a split ensemble.
    GaussianBridgeEvidence gaussianBridgeEvidence(int burnIn = 0, int sliceInterval = 1, std::uint64_t seed = 0)
    {
        return Device::gaussianBridgeEvidence(ranks[0], 0, markovChain, numWalkers, numParams, burnIn, sliceInterval, seed);
    }

    ChainType& chain() { return markovChain; }

protected:
    static void* pinnedObtain(unsigned long long bytes) { return mcmcpp_hip_host_alloc(bytes); }
    static void pinnedRelease(void* p) { mcmcpp_hip_host_free(p); }
    static void* deviceObtain(int device, unsigned long long bytes) { return mcmcpp_hip_device_alloc(device, bytes); }
    static void deviceRelease(void* p) { mcmcpp_hip_device_free(p); }
    static int deviceCopy(void* dst, const void* src, unsigned long long bytes)
    {
        const int rc = mcmcpp_hip_device_copy(dst, src, bytes);
        if (rc != MCMCPP_HIP_OK) std::fprintf(stderr, "MCMCpp (MI355X): mcmcpp_hip_device_copy failed with code %d: %s\n", rc, mcmcpp_hip_device_chain_last_error());
        return rc;
    }
    static int deviceCompact(int device, void* steps, long long numSteps, long long cellsPerStep, int burnIn, int interval, long long* kept)
    {
        std::int64_t left = 0;
        const int rc = mcmcpp_hip_device_chain_compact(HipDtype<ParamType>::value, device, steps, numSteps, cellsPerStep, burnIn, interval, &left);
        if (rc != MCMCPP_HIP_OK)
            std::fprintf(stderr, "MCMCpp (MI355X): mcmcpp_hip_device_chain_compact failed with code %d: %s\n", rc, mcmcpp_hip_device_chain_last_error());
        *kept = left;
        return rc;
    }
    bool deviceChain() const { return markovChain.memoryKind() == Chain::Detail::MemoryKind::Device; }
    /// Chain blocks come from the heap (stored steps pass through the library's pinned staging ring and are copied out by
    /// the host while the launches continue) unless MCMCPP_CHAIN_MEMORY=pinned asks for pinned host memory, into which the
    /// step launches write stored steps directly.  Measured at C2 (tools/bench_facade.cpp): pinned blocks win
    /// when the memory already exists (a chain that is reset and refilled); obtaining them costs as much as the page
    /// faults of fresh heap memory but stalls the launches while it lasts, so a growing chain is faster on the heap.
    /// MCMCPP_CHAIN_MEMORY=device keeps the chain in ONE allocation of the sampler's GPU instead (Chain/Chain.h): the run stores
    /// into it, sliceAndBurnChain and the analysis classes work on it where it lies.  Two cases keep a host chain and say so
    /// once on stderr: a placement of more than one device (a handle with a communicator refuses mcmcpp_hip_run_device), and
    /// an ensemble whose step is not a whole number of 16-byte pieces (fp32 with W*D = 2 mod 4: mcmcpp_hip_run_device wants
    /// every run's first step 16-byte aligned).
    static Chain::Detail::BlockMemory chainMemory(const Placement& where, int numWalker, int numParameter)
    {
        const char* v = std::getenv("MCMCPP_CHAIN_MEMORY");
        if (v && v[0] == 'p' && v[1] == 'i') return Chain::Detail::BlockMemory(&pinnedObtain, &pinnedRelease);
        if (v && v[0] == 'd' && v[1] == 'e')
        {
            const bool split = where.count() > 1 || where.splitEnsemble;
            const bool ragged = (static_cast<unsigned long long>(numWalker) * numParameter * sizeof(ParamType)) % 16 != 0;
            if (!split && !ragged)
                return Chain::Detail::BlockMemory::onDevice(where.device(0), &deviceObtain, &deviceRelease, &deviceCopy, &deviceCompact);
            static bool said = false;
            if (!said)
                std::fprintf(stderr, "MCMCpp (MI355X): MCMCPP_CHAIN_MEMORY=device: this sampler keeps its chain in host memory (%s)\n",
                             split ? "a placement of more than one device cannot store into device memory"
                                   : "a device chain needs steps of a whole number of 16 bytes");
            said = true;
        }
        return Chain::Detail::BlockMemory();
    }

    PostStepAction* stepAction;
    ChainType markovChain;
    Mover moveProposer;
    std::vector<HipHandle> ranks;  ///< one handle per device of the placement
    int numParams;
    int numWalkers;
    bool initialPlacementCounted;
};

}  // namespace Device
}  // namespace MCMC
#endif  // MCMCPP_DEVICE_SAMPLERCORE_H
