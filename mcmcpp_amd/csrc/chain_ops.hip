// chain_ops.hip -- what a device-resident Chain of the C++ facade (include/MCMCpp/Chain/Chain.h, MCMCPP_CHAIN_MEMORY=device)
// needs from the library besides the samplers and the *_device analysis entry points: its one allocation
// (mcmcpp_hip_device_alloc / _free), copies to, from and inside it (mcmcpp_hip_device_copy), and sliceAndBurnChain in place
// (mcmcpp_hip_device_chain_compact, chain_compact_kernel).  Which steps are kept and which launches move them is
// chain_compact_plan.hpp's; this file holds no selection rule of its own.
#include <string>
#include <type_traits>

#include "analysis_host.hpp"
#include "chain_compact_plan.hpp"

namespace
{
constexpr int kCompactThreads = 256;
constexpr long long kCompactBlocks = 2048;  // 256 CUs x 8 blocks: the grid of a memory-bound launch, the rest is strided over
constexpr int kCompactUnroll = 4;           // pieces a thread has in flight before its first store

// One wave of the compaction: destination steps [first, first + count) <- source steps burn_in + j * interval, `per_step` pieces
// of 16 bytes (Vec) or of one element each.  The plan guarantees first + count <= source(first): no block of this launch
// writes a piece another block reads, which is also what makes src and dst of one step distinct objects (__restrict__).
// Plain loads and stores; consecutive lanes move consecutive pieces (one 1 KiB wave-instruction per 64 lanes in the 16-byte
// form); kCompactUnroll independent loads are issued ahead of the stores.  blockIdx.y strides over the steps, blockIdx.x over a step.
template <class T, bool Vec>
__global__ void __launch_bounds__(kCompactThreads) chain_compact_kernel(T* steps, long long per_step, long long step_elems, long long burn_in,
                                                                        long long interval, long long first, long long count)
{
    using Piece = std::conditional_t<Vec, uint4, T>;
    const long long stride = (long long)gridDim.x * kCompactThreads;
    for (long long k = blockIdx.y; k < count; k += gridDim.y)
    {
        const long long j = first + k;
        const Piece* __restrict__ src = reinterpret_cast<const Piece*>(steps + (burn_in + j * interval) * step_elems);
        Piece* __restrict__ dst = reinterpret_cast<Piece*>(steps + j * step_elems);
        long long v = (long long)blockIdx.x * kCompactThreads + threadIdx.x;
        for (; v + (kCompactUnroll - 1) * stride < per_step; v += kCompactUnroll * stride)
        {
            Piece held[kCompactUnroll];
#pragma unroll
            for (int u = 0; u < kCompactUnroll; ++u) held[u] = src[v + u * stride];
#pragma unroll
            for (int u = 0; u < kCompactUnroll; ++u) dst[v + u * stride] = held[u];
        }
        for (; v < per_step; v += stride) dst[v] = src[v];
    }
}

thread_local std::string g_chain_error;

int chain_fail(int code, const std::string& msg) { return mcmcpp::analysis_fail(g_chain_error, code, msg); }

template <class T>
int compact(T* steps, int64_t step_elems, int64_t burn_in, int64_t interval, int64_t kept)
{
    const bool vec = (sizeof(T) * (size_t)step_elems) % 16 == 0 && ((uintptr_t)steps & 15) == 0;
    const long long per_step = vec ? (long long)(sizeof(T) * (size_t)step_elems / 16) : (long long)step_elems;
    mcmcpp::Stream stream;
    ANALYSIS_TRY(g_chain_error, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    // blocks along a step: one per kCompactUnroll * kCompactThreads pieces, so that a thread holds kCompactUnroll pieces at once
    const long long per_block = (long long)kCompactUnroll * kCompactThreads;
    long long gx = (per_step + per_block - 1) / per_block;
    if (gx > kCompactBlocks) gx = kCompactBlocks;
    mcmcpp::ChainCompactWave wave;
    for (int64_t done = 0; mcmcpp::chain_compact_wave(done, kept, burn_in, interval, &wave); done = wave.first + wave.count)
    {
        long long gy = kCompactBlocks / gx;
        if (gy > wave.count) gy = wave.count;
        if (gy < 1) gy = 1;
        const dim3 grid((unsigned)gx, (unsigned)gy);
        if (vec)
            hipLaunchKernelGGL((chain_compact_kernel<T, true>), grid, dim3(kCompactThreads), 0, stream, steps, per_step, (long long)step_elems,
                               (long long)burn_in, (long long)interval, (long long)wave.first, (long long)wave.count);
        else
            hipLaunchKernelGGL((chain_compact_kernel<T, false>), grid, dim3(kCompactThreads), 0, stream, steps, per_step, (long long)step_elems,
                               (long long)burn_in, (long long)interval, (long long)wave.first, (long long)wave.count);
        ANALYSIS_TRY(g_chain_error, hipGetLastError());
    }
    ANALYSIS_TRY(g_chain_error, hipStreamSynchronize(stream));
    return MCMCPP_HIP_OK;
}
}  // namespace

extern "C"
{
const char* mcmcpp_hip_device_chain_last_error(void) { return g_chain_error.c_str(); }

void* mcmcpp_hip_device_alloc(int32_t device, uint64_t bytes)
{
    hipDeviceProp_t prop;
    std::string why;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why))
    {
        chain_fail(rc, "device_alloc: " + why);
        return nullptr;
    }
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes ? (size_t)bytes : 64);
    if (e != hipSuccess)
    {
        (void)hipGetLastError();
        chain_fail(MCMCPP_HIP_E_NOMEM, std::string("device_alloc: hipMalloc: ") + hipGetErrorString(e));
        return nullptr;
    }
    return p;
}

void mcmcpp_hip_device_free(void* p) { mcmcpp::free_device(p); }

int mcmcpp_hip_device_copy(void* dst, const void* src, uint64_t bytes)
{
    if (bytes == 0) return MCMCPP_HIP_OK;
    if (!dst || !src) return chain_fail(MCMCPP_HIP_E_ARG, "device_copy: dst and src must not be NULL");
    ANALYSIS_TRY(g_chain_error, hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDefault));
    ANALYSIS_TRY(g_chain_error, hipStreamSynchronize(nullptr));  // (a copy inside device memory may return before it is done)
    return MCMCPP_HIP_OK;
}

int mcmcpp_hip_device_chain_compact(int32_t dtype, int32_t device, void* device_steps, int64_t n_steps, int64_t step_elems, int64_t burn_in,
                                    int64_t interval, int64_t* kept)
{
    if (dtype != MCMCPP_HIP_F64 && dtype != MCMCPP_HIP_F32) return chain_fail(MCMCPP_HIP_E_ARG, "device_chain_compact: dtype must be F64 or F32");
    if (n_steps < 0 || step_elems < 1 || burn_in < 0 || interval < 1)
        return chain_fail(MCMCPP_HIP_E_ARG, "device_chain_compact: n_steps >= 0, step_elems >= 1, burn_in >= 0 and interval >= 1");
    const size_t elem = dtype == MCMCPP_HIP_F64 ? sizeof(double) : sizeof(float);
    if (n_steps > 0 && ((uint64_t)step_elems > (((uint64_t)1 << 62) / elem) / (uint64_t)n_steps || (uint64_t)interval > ((uint64_t)1 << 62) / (uint64_t)n_steps))
        return chain_fail(MCMCPP_HIP_E_ARG, "device_chain_compact: n_steps * step_elems bytes and n_steps * interval must stay below 2^62");
    const int64_t left = mcmcpp::chain_compact_kept(n_steps, burn_in, interval);
    if (kept) *kept = left;
    if (left == 0 || (burn_in == 0 && interval == 1)) return MCMCPP_HIP_OK;  // nothing moves
    if (!device_steps) return chain_fail(MCMCPP_HIP_E_ARG, "device_chain_compact: device_steps must not be NULL");
    if (((uintptr_t)device_steps & (elem - 1)) != 0) return chain_fail(MCMCPP_HIP_E_ARG, "device_chain_compact: device_steps must be aligned to its element type");
    hipDeviceProp_t prop;
    std::string why;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return chain_fail(rc, "device_chain_compact: " + why);
    // every source lies below n_steps (the plan's rule) and every destination below its source: nothing outside these bytes is touched
    if (int rc = mcmcpp::check_device_steps(g_chain_error, "device_chain_compact", device_steps, elem * (size_t)step_elems * (size_t)n_steps, device)) return rc;
    if (dtype == MCMCPP_HIP_F64) return compact(static_cast<double*>(device_steps), step_elems, burn_in, interval, left);
    return compact(static_cast<float*>(device_steps), step_elems, burn_in, interval, left);
}
}
