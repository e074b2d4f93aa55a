// rhat_state.hpp -- what rhat.hip computes on the device before the host takes over, for the entry points that start from it:
// mcmcpp_hip_gelman_rubin (rhat.hip) and mcmcpp_hip_effective_sample_size (ess.hip), whose first phase is the R-hat state,
// bit for bit.  One request, one argument check (before a device is opened), one function that leaves the sequences' means
// and sums of squares and the per-parameter figures in device memory and the latter on the host as well.
// And the bodies of those two entry points, for the files that need their figures of a chain they hold in device memory
// (rank.hip, summary.hip): on the caller's stream, into the caller's message slot.
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

// The two forms of a request, as an extern "C" entry receives its arguments
inline RhatRequest rhat_host_request(const char* what, int32_t dtype, int32_t device, const void* const* steps, int32_t K, int64_t n_steps, int32_t W, int32_t P, int32_t split)
{
    return RhatRequest{what, dtype, device, steps, nullptr, false, K, 0, n_steps, 1, W, P, split};
}
inline RhatRequest rhat_device_request(const char* what, int32_t dtype, int32_t device, const void* device_steps, int32_t K, int64_t chain_stride_steps, int64_t n_steps,
                                       int64_t slice, int32_t W, int32_t P, int32_t split)
{
    return RhatRequest{what, dtype, device, nullptr, device_steps, true, K, chain_stride_steps, n_steps, slice, W, P, split};
}

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
int rhat_sequences_state(std::string& slot, const RhatRequest& r, const hipDeviceProp_t& prop, long long n, const RhatShape& shape, hipStream_t stream, RhatState& st);

// Do the K chains of a device request lie inside one allocation of `device`?  An entry point asks once the device is open and
// before it allocates anything; nothing is asked of host chains, nor by a caller that passes memory of its own.
inline int rhat_check_device_steps(std::string& slot, const RhatRequest& r, int device)
{
    if (!r.on_device) return MCMCPP_HIP_OK;
    const size_t step_bytes = (r.dtype == MCMCPP_HIP_F64 ? sizeof(double) : sizeof(float)) * (size_t)r.W * (size_t)r.P;
    const long long chain_stride_steps = r.chain_stride_steps ? r.chain_stride_steps : r.n_steps;
    return check_device_steps(slot, r.what, r.device_steps, step_bytes * (size_t)((r.K - 1) * chain_stride_steps + r.n_steps), device);
}

// What mcmcpp_hip_gelman_rubin and mcmcpp_hip_effective_sample_size write; any pointer may be null
struct RhatOutputs
{
    double *rhat, *mean, *within, *between, *chain_mean, *chain_within, *sequence_mean, *sequence_m2;
    int64_t *sequence_length, *num_sequences;
};
struct EssOutputs
{
    double *ess, *tau;
    int64_t *lags_used, *closed;
    double *rho, *autocov, *rhat, *mean, *within, *between;
    int64_t *sequence_length, *num_sequences;
};

// The two entry points behind their checks: r has passed rhat_check_request (or is built from a request that has: n and shape
// are rhat_shape's of it), the device of `prop` is open and current, a device chain lies where r says.  They work on `stream`,
// the caller's, which is idle when they return; their device memory lives for the call.  A failure's message goes to `slot`.
int rhat_compute(std::string& slot, const RhatRequest& r, const hipDeviceProp_t& prop, long long n, const RhatShape& shape, hipStream_t stream, const RhatOutputs& out);
int ess_compute(std::string& slot, const RhatRequest& r, int64_t max_lag, int64_t n_functions, const hipDeviceProp_t& prop, long long n, const RhatShape& shape,
                hipStream_t stream, const EssOutputs& out);

// rc of one of the two, called by the entry point `caller` with a request whose `what` names the entry point whose body ran: a
// failure reads "<caller>: <what>: ..."
inline int nested_result(std::string& slot, const char* caller, int rc)
{
    if (rc) slot = std::string(caller) + ": " + slot;
    return rc;
}
}  // namespace mcmcpp
