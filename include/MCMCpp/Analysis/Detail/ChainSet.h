/*
 * Analysis/Detail/ChainSet.h -- the chains of one multi-chain analysis (GelmanRubin.h, EffectiveSampleSize.h,
 * RankDiagnostics.h, PosteriorSummary.h): what addChain keeps of every chain, and the two forms in which the chains go to
 * the library.  Not part of the reference's API.
 *
 * A chain is a span of a device chain (DeviceSpan.h), read where it lies; host pointers to the used steps; or, for a device
 * chain whose device path is switched off, copies of the used steps.  Where every chain is a device span of the same length
 * and slice interval, DeviceSource hands them to a *_device entry point as one allocation: one chain where it lies, several
 * gathered, device to device, chain behind chain; no step comes to the host.  Otherwise hostPointers() downloads the used steps
 * of the device chains and gives the step pointers of all chains, chain behind chain.  Failures abort with the library's
 * message, like everything else in this facade.
 */
#ifndef MCMCPP_ANALYSIS_DETAIL_CHAINSET_H
#define MCMCPP_ANALYSIS_DETAIL_CHAINSET_H

#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "../../Chain/ChainStepIterator.h"
#include "../../Device/HipBackend.h"
#include "DeviceSpan.h"

namespace MCMC
{
namespace Analysis
{
namespace Detail
{
template <class ParamType>
class ChainSet
{
public:
    typedef Chain::ChainStepIterator<ParamType> IttType;

    struct ChainSteps
    {
        ChainSteps(const IttType& s, const IttType& e, int sliceInterval) : onDevice(false), used(0), slice(sliceInterval), start(s), end(e)
        {
            span.first = NULL;
            span.steps = 0;
        }
        bool onDevice;      ///< read through `span`; otherwise through `steps`
        std::int64_t used;  ///< every slice'th step of [start, end)
        int slice;
        IttType start, end;
        DeviceSpan<ParamType> span;
        std::vector<const void*> steps;  ///< into the chain's own memory, or into `staging`
        std::vector<ParamType> staging;
    };

    ChainSet(int numParams, int numWalkers) : pCount(numParams), wCount(numWalkers)
    {
        assert(pCount > 0);
        assert(wCount > 0);
    }

    /// One chain: every sliceInterval'th step of [start, end), beginning with `start`.  Every chain must give the same number
    /// of used steps.
    void addChain(IttType start, IttType end, int sliceInterval)
    {
        assert(sliceInterval >= 1);
        chains.push_back(ChainSteps(start, end, sliceInterval));
        ChainSteps& c = chains.back();
        if (deviceSpan(start, end, &c.span) && c.span.steps > 0)
        {
            c.onDevice = true;
            c.used = (c.span.steps + sliceInterval - 1) / sliceInterval;
        }
        else
            hostSteps(c);
        assert(chains.size() == 1 || c.used == chains.front().used);
    }

    int size() const { return static_cast<int>(chains.size()); }
    std::int64_t used() const { return chains.empty() ? 0 : chains.back().used; }
    const ChainSteps& chain(int k) const { return chains[k]; }

    bool anyDevice() const
    {
        for (std::size_t k = 0; k < chains.size(); ++k)
            if (chains[k].onDevice) return true;
        return false;
    }

    /// Is every chain a device span, all of one length and one slice interval?  Then DeviceSource reads them; else hostPointers().
    bool sameSpans() const
    {
        for (std::size_t k = 0; k < chains.size(); ++k)
            if (!chains[k].onDevice || chains[k].span.steps != chains[0].span.steps || chains[k].slice != chains[0].slice) return false;
        return true;
    }

    /// The chains of a set with sameSpans() as the *_device entry points take them: K chains of `steps` stored steps behind
    /// `first`, chain behind chain.  One chain is read where it lies; several are gathered into one allocation, which goes with
    /// this object.
    class DeviceSource
    {
    public:
        explicit DeviceSource(const ChainSet& set) : first(set.chains[0].span.first), K(set.size()), steps(set.chains[0].span.steps), slice(set.chains[0].slice), gathered(NULL)
        {
            if (K == 1) return;
            const std::uint64_t chainBytes = static_cast<std::uint64_t>(steps) * set.wCount * set.pCount * sizeof(ParamType);
            gathered = mcmcpp_hip_device_alloc(-1, chainBytes * K);
            if (!gathered) fail("mcmcpp_hip_device_alloc", MCMCPP_HIP_E_NOMEM, mcmcpp_hip_device_chain_last_error());
            for (int k = 0; k < K; ++k)
            {
                const int rc = mcmcpp_hip_device_copy(static_cast<char*>(gathered) + chainBytes * k, set.chains[k].span.first, chainBytes);
                if (rc != MCMCPP_HIP_OK) fail("mcmcpp_hip_device_copy", rc, mcmcpp_hip_device_chain_last_error());
            }
            first = gathered;
        }
        ~DeviceSource() { mcmcpp_hip_device_free(gathered); }

        const void* first;
        int K;
        std::int64_t steps;
        int slice;

    private:
        DeviceSource(const DeviceSource&);
        DeviceSource& operator=(const DeviceSource&);
        void* gathered;
    };

    /// The step pointers of all chains, chain behind chain ([size()][used()]; NULL where there are none), for the host-pointer
    /// entry points.  The used steps of a device chain are downloaded first.
    const void* const* hostPointers()
    {
        all.clear();
        for (std::size_t k = 0; k < chains.size(); ++k)
        {
            ChainSteps& c = chains[k];
            if (c.onDevice)
            {
                c.onDevice = false;
                c.used = downloadSteps(c.start, c.end, c.slice, c.staging);
                stagingPointers(c);
            }
            all.insert(all.end(), c.steps.begin(), c.steps.end());
        }
        return all.empty() ? NULL : all.data();
    }

    static void fail(const char* what, int rc, const char* msg)
    {
        std::fprintf(stderr, "MCMCpp (MI355X): %s failed with code %d: %s\n", what, rc, msg ? msg : "");
        std::abort();
    }

private:
    void stagingPointers(ChainSteps& c) const
    {
        c.steps.clear();
        for (std::int64_t k = 0; k < c.used; ++k) c.steps.push_back(c.staging.data() + static_cast<std::size_t>(k) * wCount * pCount);
    }

    /// the used steps of a chain that is read through host pointers
    void hostSteps(ChainSteps& c) const
    {
        if (!pointersStay(c.start))
        {
            c.used = downloadSteps(c.start, c.end, c.slice, c.staging);
            stagingPointers(c);
            return;
        }
        long long index = 0;
        for (IttType itt(c.start); itt != c.end; ++itt, ++index)
            if (index % c.slice == 0) c.steps.push_back(*itt);
        c.used = static_cast<std::int64_t>(c.steps.size());
    }

    int pCount;
    int wCount;
    std::deque<ChainSteps> chains;  ///< (a deque: adding a chain moves none of the others, whose `steps` may point into their `staging`)
    std::vector<const void*> all;
};
}  // namespace Detail
}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_DETAIL_CHAINSET_H
