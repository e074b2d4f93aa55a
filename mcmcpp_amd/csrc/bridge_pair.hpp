// bridge_pair.hpp -- one pair of the bridge estimate, from its two arrays of raw u in device memory to its figures: the solver's
// passes, the final pass's sums, the effective sample size of h_d(c*), and the edges, as include/mcmcpp_hip.h defines them
// under mcmcpp_hip_evidence_bridge.  bridge.hip has the kernels and the body; it calls this per pair of neighbouring rungs, and
// gaussian_bridge.hip (mcmcpp_hip_evidence_gaussian) calls it on the pair (target, fitted Gaussian).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>
#include <string>

#include "bridge_plan.hpp"
#include "sampler_base.hpp"

namespace mcmcpp
{
// The figures of a pair as the edges leave them where nothing is estimated: NaN, and no pass
struct BridgePairFigures
{
    double log_ratio = std::numeric_limits<double>::quiet_NaN(), mcse = log_ratio, overlap = log_ratio, ess[2] = {log_ratio, log_ratio};
    int64_t passes = 0, converged = 0;
};
// The tile and slice sums of a pass and the six sums the host reads back: allocated once per call, for N draws a direction
struct BridgePairScratch
{
    BridgePlan plan;
    DeviceBuffer<double> tiles, slices, out;
    hipError_t alloc(long long N)
    {
        plan = bridge_plan(N);
        if (const hipError_t e = tiles.alloc(8 * plan.tile_sum_doubles)) return e;
        if (const hipError_t e = slices.alloc(8 * plan.slice_sum_doubles)) return e;
        return out.alloc(8 * 6);
    }
};
// u[0], u[1]: N = n W doubles each, complete and free of NaN and +inf (the caller leaves such a pair's figures as they are);
// the final pass writes h_d(c*) over them.  `what` names the entry point in a nested failure's message.
int bridge_pair_compute(std::string& slot, const char* what, int device, const hipDeviceProp_t& prop, hipStream_t stream, const BridgePairScratch& scratch,
                        double* const u[2], long long n, int W, BridgePairFigures* out);
}  // namespace mcmcpp
