// rhat_state.hpp -- what rhat.hip computes on the device before the host takes over, for the entry points that start from it:
// mcmcpp_hip_gelman_rubin (rhat.hip) and mcmcpp_hip_effective_sample_size (ess.hip), whose first phase is the R-hat state,
// bit for bit.  One request, one argument check (before a device is opened), one function that leaves the sequences' means
// and sums of squares and the per-parameter figures in device memory and the latter on the host as well.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "analysis_host.hpp"
#include "rhat_plan.hpp"

namespace mcmcpp
{
struct RhatRequest
{
    const char* what;
    int32_t dtype, device;
    const void* const* steps;
    const void* device_steps;
    bool on_device;
    int32_t K;
    int64_t chain_stride_steps, n_steps, slice;
    int32_t W, P, split;
};

// The buffers belong to the caller, who declares the state in front of its Stream: the stream is idle and gone when they go.
//   seq  sequence_mean [M][P], then sequence_m2 [M][P]
//   res  mean, within, between [P]; chain_mean, chain_within [K][P]; h_res: the same on the host, valid once the stream that
//        rhat_sequences_state worked on has been synchronised
struct RhatState
{
    DeviceBuffer<> chunk;
    DeviceBuffer<double> first, state, seq, part, res;
    std::vector<double> h_res;
};

// Every check that needs no device, in the order and the words of mcmcpp_hip_gelman_rubin; *n = used steps of a chain
int rhat_check_request(std::string& slot, const RhatRequest& r, long long* n, RhatShape* shape);

// The series, sequence and combine launches on `stream`, and the copy of res into h_res behind them; returns without waiting
int rhat_sequences_state(std::string& slot, const RhatRequest& r, int device, const hipDeviceProp_t& prop, long long n, const RhatShape& shape, hipStream_t stream,
                         RhatState& st);
}  // namespace mcmcpp
