/*
 * Analysis/Detail/DeviceSpan.h -- how the analysis classes find out that the steps of [start, end) can be read where they
 * lie.  A device chain (Chain/Chain.h, MCMCPP_CHAIN_MEMORY=device) is one contiguous allocation [steps][W][D], so an iterator
 * pair on it is a base pointer and a step count: the classes hand those to the *_device entry points of include/mcmcpp_hip.h
 * and no stored step comes to the host.  Every other pair -- a host chain, or MCMCPP_DEVICE_ANALYSIS=0 in the environment,
 * which switches the device path off -- is read through host pointers as before; for a device chain those are copies of the
 * selected steps, downloaded one by one through the iterators (downloadSteps).  Not part of the reference's API.
 */
#ifndef MCMCPP_ANALYSIS_DETAIL_DEVICESPAN_H
#define MCMCPP_ANALYSIS_DETAIL_DEVICESPAN_H

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../Chain/Chain.h"

namespace MCMC
{
namespace Analysis
{
namespace Detail
{
/// the steps of an iterator pair on a device chain: `steps` consecutive ones behind `first` (DEVICE memory)
template <class ParamType>
struct DeviceSpan
{
    const ParamType* first;
    std::int64_t steps;
};

inline bool deviceAnalysisEnabled()
{
    const char* v = std::getenv("MCMCPP_DEVICE_ANALYSIS");
    return !(v && v[0] == '0');
}

/// True, with the span, when [start, end) lies in one device chain and the device path is not switched off.
template <class ParamType>
inline bool deviceSpan(const Chain::ChainStepIterator<ParamType>& start, const Chain::ChainStepIterator<ParamType>& end, DeviceSpan<ParamType>* span)
{
    Chain::Chain<ParamType>* chain = start.owner();
    if (!chain || chain != end.owner() || chain->memoryKind() != Chain::Detail::MemoryKind::Device || !deviceAnalysisEnabled()) return false;
    const Chain::DeviceSteps<ParamType> all = chain->deviceSteps();
    const std::int64_t lo = start.stepIndex(), hi = end.stepIndex();
    if (!all.base || lo < 0 || hi > all.steps || lo > hi) return false;
    span->first = all.base + static_cast<std::size_t>(lo) * static_cast<std::size_t>(chain->getCellsPerStep());
    span->steps = hi - lo;
    return true;
}

/// Does `*it` hand out a pointer into the chain's own memory (true), or into a one-step buffer that the next dereference
/// overwrites (a device chain)?
template <class ParamType>
inline bool pointersStay(const Chain::ChainStepIterator<ParamType>& it)
{
    return !it.owner() || it.owner()->memoryKind() != Chain::Detail::MemoryKind::Device;
}

/// Copies of every stride'th step of [start, end) of a device chain, one behind the other in `staging`.
template <class ParamType>
inline std::int64_t downloadSteps(Chain::ChainStepIterator<ParamType> start, const Chain::ChainStepIterator<ParamType>& end, int stride, std::vector<ParamType>& staging)
{
    const std::size_t cells = static_cast<std::size_t>(start.owner()->getCellsPerStep());
    staging.clear();
    std::int64_t used = 0;
    for (; start != end; start += stride, ++used)
    {
        const ParamType* p = *start;
        staging.insert(staging.end(), p, p + cells);
    }
    return used;
}
}  // namespace Detail
}  // namespace Analysis
}  // namespace MCMC
#endif  // MCMCPP_ANALYSIS_DETAIL_DEVICESPAN_H
