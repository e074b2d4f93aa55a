// analysis_host.hpp -- the host code the analysis entry points share (moments.hip, autocorr.hip, histograms.hip, quantiles.hip,
// chain_ops.hip): the error path, the refusal of a device_steps pointer, and the source of stored steps a kernel reads a chunk
// at a time.  The arithmetic is step_chunks.hpp's (tested on the CPU); the owners and the range probe are sampler_base.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "sampler_base.hpp"
#include "step_chunks.hpp"

namespace mcmcpp
{
// Every family has its own *_last_error, so its own message slot: a thread-local string where there is no handle, the
// handle's string where there is one.  A HIP failure reads "<expression>: <error string>".
inline int analysis_fail(std::string& slot, int code, std::string msg, hipError_t e = hipSuccess)
{
    if (e != hipSuccess) msg += std::string(": ") + hipGetErrorString(e);
    slot = std::move(msg);
    return code;
}

#define ANALYSIS_TRY(slot, expr)                                                                   \
    do                                                                                             \
    {                                                                                              \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return mcmcpp::analysis_fail(slot, MCMCPP_HIP_E_HIP, #expr, e_);      \
    } while (0)

// Does [p, p + bytes) lie inside one allocation of device `device`?  `name` is the argument's; `too_short` is what its entry
// point says of a range that ends outside the allocation.
inline int check_device_range(std::string& slot, const char* what, const char* name, const void* p, size_t bytes, int device, const std::string& too_short)
{
    const std::string w(what), a(name);
    const DeviceRange r = probe_device_range(p, device);
    switch (r.kind)
    {
    case DeviceRange::NotDevice: return analysis_fail(slot, MCMCPP_HIP_E_ARG, w + ": " + a + " is not device memory");
    case DeviceRange::OtherDevice:
        return analysis_fail(slot, MCMCPP_HIP_E_ARG, w + ": " + a + " is memory of device " + std::to_string(r.device) + ", not of device " + std::to_string(device));
    case DeviceRange::NoAllocation: return analysis_fail(slot, MCMCPP_HIP_E_ARG, w + ": the runtime does not know the allocation " + a + " lies in");
    case DeviceRange::Found: break;
    }
    if (bytes > r.room) return analysis_fail(slot, MCMCPP_HIP_E_ARG, w + ": " + too_short);
    return MCMCPP_HIP_OK;
}

// The same of stored steps.  (As the samplers ask before run_device launches anything.)
inline int check_device_steps(std::string& slot, const char* what, const void* p, size_t bytes, int device)
{
    return check_device_range(slot, what, "device_steps", p, bytes, device, "n_steps steps do not end inside the allocation around device_steps");
}

// For a function that works on its caller's stream: declared behind the function's buffers, as a Stream of its own would be,
// so that the stream is idle when they go
struct IdleOnReturn
{
    hipStream_t stream;
    ~IdleOnReturn() { (void)hipStreamSynchronize(stream); }
};

// Steps [k0, k0 + now) into dst, one behind the other; src_of(k) is the address of step k.  Steps that follow each other in
// memory go in one copy.
template <class SrcOf>
hipError_t copy_steps(void* dst, SrcOf&& src_of, long long k0, long long now, size_t step_bytes, hipMemcpyKind kind, hipStream_t stream)
{
    for (long long k = k0; k < k0 + now;)
    {
        const long long run = contiguous_run(src_of, k, k0 + now, step_bytes);
        if (const hipError_t e = hipMemcpyAsync((char*)dst + step_bytes * (size_t)(k - k0), src_of(k), step_bytes * (size_t)run, kind, stream)) return e;
        k += run;
    }
    return hipSuccess;
}

// Selected samples as a kernel reads them: n_steps steps of W*P elements, step k at base + k * step_stride (elements)
template <class T>
struct StepSpan
{
    const T* base;
    long long step_stride;
    long long n_steps;
};

// One call's source of steps: `used` host pointers, uploaded a chunk at a time into *chunk (which the caller has made
// upload_bytes(per) large), or every slice-th of the steps behind device_steps, read where they lie.
template <class T>
struct StepSource
{
    const void* const* host_steps;
    const T* device_steps;
    long long used, slice;
    int W, P;
    hipStream_t stream;
    const DeviceBuffer<>* chunk;
    std::string* error;     // the family's message slot
    bool resident = false;  // a host selection of one chunk, uploaded already: a further pass uploads nothing

    size_t upload_bytes(long long per) const { return device_steps ? 0 : sizeof(T) * (size_t)W * P * (size_t)(used < per ? used : per); }

    // f(span) for every chunk of `per` steps of the selection, in order (none if used == 0); stops at the first failure
    template <class F>
    int for_each_chunk(long long per, F&& f)
    {
        const size_t step_elems = (size_t)W * P;
        return for_each_step_chunk(used, per, [&](long long k0, long long now) -> int {
            if (device_steps) return f(StepSpan<T>{device_steps + (size_t)(k0 * slice) * step_elems, (long long)(slice * (long long)step_elems), now});
            if (!resident)
            {
                ANALYSIS_TRY(*error, hipStreamSynchronize(stream));  // the previous chunk's kernels have read the buffer
                ANALYSIS_TRY(*error, copy_steps(chunk->get(), [&](long long k) { return host_steps[k]; }, k0, now, sizeof(T) * step_elems, hipMemcpyHostToDevice, stream));
            }
            resident = used <= per;
            return f(StepSpan<T>{(const T*)chunk->get(), (long long)step_elems, now});
        });
    }
};
}  // namespace mcmcpp
