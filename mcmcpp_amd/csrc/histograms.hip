// histograms.hip -- 1-D histograms of every parameter and 2-D histograms of every parameter pair of stored chain steps:
// the device side of Analysis::CornerHistograms and Analysis::PercentileAndMaximumFinder (reference:
// MCMCpp/Analysis/CornerHistograms.h, PercentileAndMaximumFinder.h).
//
// Both reference classes bin the same way: per parameter the minimum and maximum of the samples used (start values
// numeric_limits<T>::max() / ::min(), strict comparisons), a small tweak of the two bounds, width = (hi - lo) / bins,
// and bin = int((x - lo) / width), all in T.  Here:
//   * bounds pass: per-block minimum / maximum of every parameter (strict comparisons, the reference's start values),
//     combined on the host; min and max are exact in any order.  A NaN sample fails the call.
//   * the tweak and the width are computed on the host in T (this file is built with -ffp-contract=off);
//   * bin pass: every selected sample's bin of every parameter, (x - lo) / width as a correctly rounded division in T,
//     truncated toward zero, written as a column-major index array [P][n] of u8 / u16 / u32.  A bin outside [0, bins)
//     (the reference's upper-bound tweak puts every positive maximum above the range; its behaviour there is undefined)
//     is clamped into bin 0 or bins - 1 and counted per parameter;
//   * 1-D histograms: one block per (slice of samples, parameter), counters privatised in LDS (u32), flushed with
//     64-bit integer atomics; global 64-bit atomics where the bins do not fit;
//   * 2-D histograms: one block per (slice of samples, tile of pairs), the tile's pair histograms privatised in LDS,
//     fed from the two index columns of each pair, flushed with 64-bit integer atomics; global 64-bit atomics where one
//     pair histogram does not fit.
// Every count is an integer sum: results are bit-reproducible and independent of scheduling and chunking.
// Host chains are uploaded in chunks of MCMCPP_HIP_HIST_CHUNK_MB (read at create, default 1024); a selection that fits
// in one chunk is uploaded once and serves both passes, a larger one is uploaded twice.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/mcmcpp_hip.h"
#include "analysis_host.hpp"
#include "hist_plan.hpp"

namespace
{
constexpr int kHistThreads = 256;
static_assert(kHistThreads == mcmcpp::kHistPlanThreads, "hist_plan.hpp plans for the block size of these kernels");

template <class T>
__device__ __forceinline__ const T* sample_row(const T* base, long long step_stride, unsigned W, int P, unsigned s)
{
    return base + (size_t)(s / W) * (size_t)step_stride + (size_t)(s % W) * (size_t)P;
}

// per-block minimum / maximum of every parameter over samples [blockIdx.x * per, ...): part[block][P][2]
template <class T>
__global__ void __launch_bounds__(kHistThreads)
hist_bounds_kernel(const T* base, long long step_stride, unsigned W, int P, unsigned n, unsigned per, T* part, int* nan_flag)
{
    __shared__ T s_lo[kHistThreads], s_hi[kHistThreads];
    const unsigned s0 = blockIdx.x * per;
    const unsigned s1 = (n - s0 < per) ? n : s0 + per;
    const int tid = threadIdx.x;
    bool nan = false;
    for (int p0 = 0; p0 < P; p0 += kHistThreads)
    {
        const int pt = (P - p0 < kHistThreads) ? P - p0 : kHistThreads;
        const int rows = kHistThreads / pt;
        T lo = std::numeric_limits<T>::max(), hi = std::numeric_limits<T>::min();
        if (tid < rows * pt)
        {
            const int p = p0 + tid % pt;
            for (unsigned s = s0 + tid / pt; s < s1; s += rows)
            {
                const T x = sample_row(base, step_stride, W, P, s)[p];
                nan |= (x != x);
                if (x < lo) lo = x;
                if (x > hi) hi = x;
            }
        }
        __syncthreads();
        s_lo[tid] = lo;
        s_hi[tid] = hi;
        __syncthreads();
        if (tid < pt)
        {
            for (int r = 1; r < rows; ++r)
            {
                if (s_lo[r * pt + tid] < lo) lo = s_lo[r * pt + tid];
                if (s_hi[r * pt + tid] > hi) hi = s_hi[r * pt + tid];
            }
            T* o = part + ((size_t)blockIdx.x * P + p0 + tid) * 2;
            o[0] = lo;
            o[1] = hi;
        }
    }
    if (nan) atomicOr(nan_flag, 1);
}

// bin of every (sample, parameter): idx[p * col + s]; out-of-range bins clamped and counted
template <class T, class I>
__global__ void __launch_bounds__(kHistThreads)
hist_bin_kernel(const T* base, long long step_stride, unsigned W, int P, unsigned n, const T* edges, int bins, I* idx, size_t col,
                unsigned long long* clamped)
{
    const double top = (double)bins;
    for (unsigned s = blockIdx.x * kHistThreads + threadIdx.x; s < n; s += gridDim.x * kHistThreads)
    {
        const T* row = sample_row(base, step_stride, W, P, s);
        for (int p = 0; p < P; ++p)
        {
            const T q = (row[p] - edges[2 * p]) / edges[2 * p + 1];
            const double qd = (double)q;
            int b;
            if (qd >= top)
                b = bins - 1;
            else if (!(qd > -1.0))
                b = 0;
            else
                b = -1;
            if (b >= 0)
                atomicAdd(&clamped[p], 1ull);
            else
                b = (int)q;  // in (-1, bins): truncation toward zero lands in [0, bins)
            idx[(size_t)p * col + s] = (I)b;
        }
    }
}

// 1-D histograms: block (slice, p); LDS counters when `lds` (dynamic size bins * 4), else global atomics
template <class I>
__global__ void __launch_bounds__(kHistThreads)
hist_single_kernel(const I* idx, size_t col, unsigned n, unsigned per, int bins, int lds, unsigned long long* single)
{
    extern __shared__ unsigned s_cnt[];
    const int p = blockIdx.y;
    const unsigned s0 = blockIdx.x * per;
    const unsigned s1 = (n - s0 < per) ? n : s0 + per;
    const I* c = idx + (size_t)p * col;
    unsigned long long* out = single + (size_t)p * bins;
    if (lds)
    {
        for (int b = threadIdx.x; b < bins; b += kHistThreads) s_cnt[b] = 0;
        __syncthreads();
        for (unsigned s = s0 + threadIdx.x; s < s1; s += kHistThreads) atomicAdd(&s_cnt[c[s]], 1u);
        __syncthreads();
        for (int b = threadIdx.x; b < bins; b += kHistThreads)
            if (s_cnt[b]) atomicAdd(&out[b], (unsigned long long)s_cnt[b]);
    }
    else
        for (unsigned s = s0 + threadIdx.x; s < s1; s += kHistThreads) atomicAdd(&out[c[s]], 1ull);
}

// 2-D histograms: block (slice, tile of `tile` pairs); pair q = (i, j) from ij[2q], ij[2q+1]; element [bin_i][bin_j]
template <class I>
__global__ void __launch_bounds__(kHistThreads)
hist_pairs_kernel(const I* idx, size_t col, unsigned n, unsigned per, int bins, const int* ij, long long npairs, int tile, int lds,
                  unsigned long long* pairs)
{
    extern __shared__ unsigned s_cnt[];
    const unsigned s0 = blockIdx.x * per;
    const unsigned s1 = (n - s0 < per) ? n : s0 + per;
    const long long q0 = (long long)blockIdx.y * tile;
    const int count = (npairs - q0 < tile) ? (int)(npairs - q0) : tile;
    const size_t b2 = (size_t)bins * bins;
    if (lds)
    {
        const int cells = count * (int)b2;
        for (int e = threadIdx.x; e < cells; e += kHistThreads) s_cnt[e] = 0;
        __syncthreads();
        for (int k = 0; k < count; ++k)
        {
            const I* ci = idx + (size_t)ij[2 * (q0 + k)] * col;
            const I* cj = idx + (size_t)ij[2 * (q0 + k) + 1] * col;
            unsigned* h = s_cnt + (size_t)k * b2;
            for (unsigned s = s0 + threadIdx.x; s < s1; s += kHistThreads) atomicAdd(&h[(unsigned)ci[s] * bins + cj[s]], 1u);
        }
        __syncthreads();
        unsigned long long* out = pairs + (size_t)q0 * b2;
        for (int e = threadIdx.x; e < cells; e += kHistThreads)
            if (s_cnt[e]) atomicAdd(&out[e], (unsigned long long)s_cnt[e]);
    }
    else
        for (int k = 0; k < count; ++k)
        {
            const I* ci = idx + (size_t)ij[2 * (q0 + k)] * col;
            const I* cj = idx + (size_t)ij[2 * (q0 + k) + 1] * col;
            unsigned long long* out = pairs + (size_t)(q0 + k) * b2;
            for (unsigned s = s0 + threadIdx.x; s < s1; s += kHistThreads) atomicAdd(&out[(size_t)ci[s] * bins + cj[s]], 1ull);
        }
}
}  // namespace

struct mcmcpp_hip_histograms
{
    std::string error;
    int dtype = 0, device = 0, W = 0, P = 0, bins = 0, cus = 0;
    bool with_pairs = false;
    long long npairs = 0;
    size_t chunk_bytes = 0;        // MCMCPP_HIP_HIST_CHUNK_MB
    size_t lds_limit = 0;          // dynamic LDS per block for the counters
    int idx_bytes = 1;             // 1 / 2 / 4 (hist_plan.hpp)
    mcmcpp::DeviceBuffer<unsigned long long> d_single, d_pairs, d_clamped;
    mcmcpp::DeviceBuffer<int> d_ij;      // [npairs][2]
    mcmcpp::DeviceBuffer<int> d_nan;
    mcmcpp::DeviceBuffer<> d_edges;      // [P][2] (low edge, width) in T
    mcmcpp::DeviceBuffer<> d_part;       // bounds partials
    mcmcpp::DeviceBuffer<> d_chunk;      // host path upload buffer
    mcmcpp::DeviceBuffer<> d_idx;        // bin indices [P][col]
    bool have_result = false;
    long long points = 0;
    std::vector<unsigned char> bounds;  // [P][2] in T
    // LAST: destroyed first, and idle by then -- nothing it enqueued still uses a buffer above when that frees itself
    mcmcpp::Stream stream;
};

namespace
{
thread_local std::string g_hist_error;

int fail(mcmcpp_hip_histograms* h, int code, const std::string& msg) { return mcmcpp::analysis_fail(h ? h->error : g_hist_error, code, msg); }

int ensure(mcmcpp_hip_histograms* h, mcmcpp::DeviceBuffer<>& buf, size_t bytes, const char* what)
{
    if (mcmcpp::grow(buf, bytes, h->stream))
        return fail(h, MCMCPP_HIP_E_NOMEM, std::string("histograms: cannot allocate ") + what + " (" + std::to_string(bytes) + " bytes)");
    return MCMCPP_HIP_OK;
}

using mcmcpp::StepSpan;

template <class T>
int bounds_pass(mcmcpp_hip_histograms* h, const StepSpan<T>& sp, std::vector<T>& lo, std::vector<T>& hi)
{
    const unsigned n = (unsigned)(sp.n_steps * h->W);
    if (n == 0) return MCMCPP_HIP_OK;
    const mcmcpp::HistPlan plan = mcmcpp::hist_plan(n, h->P, h->bins, h->with_pairs, h->cus, h->lds_limit);
    const unsigned blocks = plan.bounds_blocks, per = plan.bounds_per;
    const size_t pbytes = sizeof(T) * 2 * (size_t)blocks * h->P;
    int rc = ensure(h, h->d_part, pbytes, "the bounds partials");
    if (rc) return rc;
    hipLaunchKernelGGL((hist_bounds_kernel<T>), dim3(blocks), dim3(kHistThreads), 0, h->stream, sp.base, sp.step_stride, (unsigned)h->W, h->P,
                       n, per, (T*)h->d_part.get(), h->d_nan);
    ANALYSIS_TRY(h->error, hipGetLastError());
    std::vector<T> part(2 * (size_t)blocks * h->P);
    ANALYSIS_TRY(h->error, hipMemcpyAsync(part.data(), h->d_part, pbytes, hipMemcpyDeviceToHost, h->stream));
    ANALYSIS_TRY(h->error, hipStreamSynchronize(h->stream));
    for (unsigned b = 0; b < blocks; ++b)
        for (int p = 0; p < h->P; ++p)
        {
            const T l = part[((size_t)b * h->P + p) * 2], u = part[((size_t)b * h->P + p) * 2 + 1];
            if (l < lo[p]) lo[p] = l;
            if (u > hi[p]) hi[p] = u;
        }
    return MCMCPP_HIP_OK;
}

template <class T, class I>
int count_pass_t(mcmcpp_hip_histograms* h, const StepSpan<T>& sp)
{
    const unsigned n = (unsigned)(sp.n_steps * h->W);
    if (n == 0) return MCMCPP_HIP_OK;
    const mcmcpp::HistPlan plan = mcmcpp::hist_plan(n, h->P, h->bins, h->with_pairs, h->cus, h->lds_limit);
    const size_t col = plan.col;
    int rc = ensure(h, h->d_idx, sizeof(I) * col * h->P, "the bin index buffer");
    if (rc) return rc;
    I* idx = (I*)h->d_idx.get();
    const int bins = h->bins;
    hipLaunchKernelGGL((hist_bin_kernel<T, I>), dim3(plan.bin_blocks), dim3(kHistThreads), 0, h->stream, sp.base, sp.step_stride, (unsigned)h->W, h->P, n,
                       (const T*)h->d_edges.get(), bins, idx, col, h->d_clamped);
    ANALYSIS_TRY(h->error, hipGetLastError());
    hipLaunchKernelGGL((hist_single_kernel<I>), dim3(plan.single_blocks, h->P), dim3(kHistThreads), plan.single_lds_bytes, h->stream, idx, col, n,
                       plan.single_per, bins, plan.single_lds, h->d_single);
    ANALYSIS_TRY(h->error, hipGetLastError());
    const size_t b2 = (size_t)bins * bins;
    for (long long i = 0; i < plan.pair_launches; ++i)  // (none without pairs; more than one past the grid.y limit)
    {
        const mcmcpp::HistPairLaunch l = plan.pair_launch(i);
        hipLaunchKernelGGL((hist_pairs_kernel<I>), dim3(plan.pair_blocks, (unsigned)l.now), dim3(kHistThreads), plan.pair_lds_bytes, h->stream, idx, col, n,
                           plan.pair_per, bins, h->d_ij + 2 * l.q0, plan.npairs - l.q0, plan.tile, plan.pair_lds, h->d_pairs + (size_t)l.q0 * b2);
        ANALYSIS_TRY(h->error, hipGetLastError());
    }
    return MCMCPP_HIP_OK;
}

template <class T>
int count_pass(mcmcpp_hip_histograms* h, const StepSpan<T>& sp)
{
    switch (h->idx_bytes)
    {
    case 1: return count_pass_t<T, uint8_t>(h, sp);
    case 2: return count_pass_t<T, uint16_t>(h, sp);
    default: return count_pass_t<T, uint32_t>(h, sp);
    }
}

template <class T>
int sign_of(T v)
{
    return (T(0) < v) - (v < T(0));
}

// the reference's findBinning after its extremum search (CornerHistograms.h / PercentileAndMaximumFinder.h): bound tweak,
// then the width; in T, operation for operation
template <class T>
void finish_bounds(mcmcpp_hip_histograms* h, const std::vector<T>& lo_in, const std::vector<T>& hi_in)
{
    const T expand = static_cast<T>(1.001), contract = static_cast<T>(0.999), minSize = static_cast<T>(0.001);
    h->bounds.assign(sizeof(T) * 2 * (size_t)h->P, 0);
    T* b = (T*)h->bounds.data();
    for (int p = 0; p < h->P; ++p)
    {
        T lo = lo_in[p], hi = hi_in[p];
        if (lo == hi)
        {
            if (lo != T(0))
            {
                if (sign_of(lo) == 1)
                {
                    lo *= contract;
                    hi *= expand;
                }
                else
                {
                    lo *= expand;
                    hi *= contract;
                }
            }
            else
            {
                lo = -minSize;
                hi = minSize;
            }
        }
        else
        {
            int s = sign_of(lo);
            if (s == -1)
                lo *= expand;
            else if (s == 0)
                lo = -minSize;
            else
                lo *= contract;
            s = sign_of(hi);
            if (s == -1)
                hi *= expand;
            else if (s == 0)
                hi = minSize;
            else
                hi *= contract;
        }
        b[2 * p] = lo;
        b[2 * p + 1] = (hi - lo) / static_cast<T>(h->bins);
    }
}

int reset_counts(mcmcpp_hip_histograms* h)
{
    h->have_result = false;
    ANALYSIS_TRY(h->error, hipMemsetAsync(h->d_single, 0, sizeof(unsigned long long) * (size_t)h->P * h->bins, h->stream));
    if (h->d_pairs) ANALYSIS_TRY(h->error, hipMemsetAsync(h->d_pairs, 0, sizeof(unsigned long long) * (size_t)h->npairs * h->bins * h->bins, h->stream));
    ANALYSIS_TRY(h->error, hipMemsetAsync(h->d_clamped, 0, sizeof(unsigned long long) * h->P, h->stream));
    ANALYSIS_TRY(h->error, hipMemsetAsync(h->d_nan, 0, sizeof(int), h->stream));
    return MCMCPP_HIP_OK;
}

template <class T>
int after_bounds(mcmcpp_hip_histograms* h, const std::vector<T>& lo, const std::vector<T>& hi)
{
    int nan = 0;
    ANALYSIS_TRY(h->error, hipMemcpyAsync(&nan, h->d_nan, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ANALYSIS_TRY(h->error, hipStreamSynchronize(h->stream));
    if (nan) return fail(h, MCMCPP_HIP_E_ARG, "histograms: the selected samples contain a NaN (the reference would index with int(NaN))");
    finish_bounds<T>(h, lo, hi);
    ANALYSIS_TRY(h->error, hipMemcpyAsync(h->d_edges, h->bounds.data(), h->bounds.size(), hipMemcpyHostToDevice, h->stream));
    return MCMCPP_HIP_OK;
}

// the bounds pass, the binning and the count pass over the source's chunks (a host selection of one chunk is uploaded once)
template <class T>
int compute(mcmcpp_hip_histograms* h, mcmcpp::StepSource<T> src)
{
    const long long per = mcmcpp::hist_steps_per_chunk(h->chunk_bytes, sizeof(T) * (size_t)h->W * h->P, h->W);
    int rc = ensure(h, h->d_chunk, src.upload_bytes(per), "the upload buffer");
    if (rc) return rc;
    std::vector<T> lo(h->P, std::numeric_limits<T>::max()), hi(h->P, std::numeric_limits<T>::min());
    if ((rc = src.for_each_chunk(per, [&](const StepSpan<T>& sp) { return bounds_pass<T>(h, sp, lo, hi); }))) return rc;
    if ((rc = after_bounds<T>(h, lo, hi))) return rc;
    if ((rc = src.for_each_chunk(per, [&](const StepSpan<T>& sp) { return count_pass<T>(h, sp); }))) return rc;
    ANALYSIS_TRY(h->error, hipStreamSynchronize(h->stream));
    h->points = src.used * h->W;
    h->have_result = true;
    return MCMCPP_HIP_OK;
}

// reset, then compute<T> of the handle's type: `used` host pointers, or every slice-th step behind device_steps
int compute_entry(mcmcpp_hip_histograms* h, const void* const* steps, const void* device_steps, long long used, long long slice)
{
    ANALYSIS_TRY(h->error, hipSetDevice(h->device));
    if (int rc = reset_counts(h)) return rc;
    if (h->dtype == MCMCPP_HIP_F64)
        return compute<double>(h, {steps, static_cast<const double*>(device_steps), used, slice, h->W, h->P, h->stream, &h->d_chunk, &h->error});
    return compute<float>(h, {steps, static_cast<const float*>(device_steps), used, slice, h->W, h->P, h->stream, &h->d_chunk, &h->error});
}
}  // namespace

extern "C"
{
const char* mcmcpp_hip_histograms_last_error(const mcmcpp_hip_histograms* h) { return h ? h->error.c_str() : g_hist_error.c_str(); }

int mcmcpp_hip_histograms_create(int32_t dtype, int32_t device, int32_t num_walkers, int32_t num_params, int32_t bins, int32_t with_pairs,
                                 mcmcpp_hip_histograms** out)
{
    mcmcpp_hip_histograms* h = nullptr;
    if (!out) return fail(h, MCMCPP_HIP_E_ARG, "histograms_create: out is NULL");
    *out = nullptr;
    if ((dtype != MCMCPP_HIP_F64 && dtype != MCMCPP_HIP_F32) || num_walkers < 1 || num_params < 1 || num_params > 65535 || bins < 2)
        return fail(h, MCMCPP_HIP_E_ARG, "histograms_create: dtype must be F64/F32, num_walkers >= 1, 1 <= num_params <= 65535, bins >= 2");
    hipDeviceProp_t prop;
    std::string why;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return fail(h, rc, "histograms_create: " + why);
    const long long npairs = mcmcpp::hist_npairs(num_params, with_pairs != 0);
    // the 64-bit result arrays; refuse what cannot be addressed before asking the allocator
    const double pair_bytes = (double)npairs * (double)bins * (double)bins * 8.0;
    const double single_bytes = (double)num_params * (double)bins * 8.0;
    if (pair_bytes > (double)((size_t)1 << 50) || single_bytes > (double)((size_t)1 << 50))
    {
        char msg[200];
        std::snprintf(msg, sizeof msg, "histograms_create: the 64-bit result arrays would take %.3g bytes", pair_bytes + single_bytes);
        return fail(h, MCMCPP_HIP_E_NOMEM, msg);
    }
    h = new (std::nothrow) mcmcpp_hip_histograms();
    if (!h) return fail(nullptr, MCMCPP_HIP_E_NOMEM, "histograms_create: out of host memory");
    h->dtype = dtype;
    h->device = device;
    h->W = num_walkers;
    h->P = num_params;
    h->bins = bins;
    h->with_pairs = with_pairs != 0;
    h->npairs = npairs;
    h->cus = prop.multiProcessorCount;
    h->lds_limit = mcmcpp::hist_lds_limit(prop.sharedMemPerBlock);
    h->idx_bytes = mcmcpp::hist_index_bytes(bins);
    h->chunk_bytes = mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_HIST_CHUNK_MB", 1024);
    const size_t esize = dtype == MCMCPP_HIP_F64 ? 8 : 4;
    auto bad = [&](int code, const std::string& what) {
        g_hist_error = what;
        mcmcpp_hip_histograms_destroy(h);
        return code;
    };
    if (hipStreamCreateWithFlags(h->stream.replace(), hipStreamNonBlocking) != hipSuccess) return bad(MCMCPP_HIP_E_HIP, "histograms_create: cannot create a stream");
    if (h->d_single.alloc((size_t)single_bytes) != hipSuccess || h->d_clamped.alloc(8 * (size_t)num_params) != hipSuccess ||
        h->d_nan.alloc(sizeof(int)) != hipSuccess || h->d_edges.alloc(2 * esize * (size_t)num_params) != hipSuccess)
        return bad(MCMCPP_HIP_E_NOMEM, "histograms_create: cannot allocate device memory");
    if (npairs > 0)
    {
        if (h->d_pairs.alloc((size_t)pair_bytes) != hipSuccess)
            return bad(MCMCPP_HIP_E_NOMEM, "histograms_create: cannot allocate the " + std::to_string((size_t)pair_bytes) +
                                               "-byte 64-bit pair histograms (" + std::to_string(npairs) + " pairs of " + std::to_string(bins) +
                                               " x " + std::to_string(bins) + " bins)");
        std::vector<int> ij(2 * (size_t)npairs);
        size_t q = 0;
        for (int i = 1; i < num_params; ++i)
            for (int j = 0; j < i; ++j, ++q)
            {
                ij[2 * q] = i;
                ij[2 * q + 1] = j;
            }
        if (h->d_ij.alloc(sizeof(int) * ij.size()) != hipSuccess) return bad(MCMCPP_HIP_E_NOMEM, "histograms_create: cannot allocate the pair table");
        if (hipMemcpy(h->d_ij, ij.data(), sizeof(int) * ij.size(), hipMemcpyHostToDevice) != hipSuccess)
            return bad(MCMCPP_HIP_E_HIP, "histograms_create: cannot upload the pair table");
    }
    *out = h;
    return MCMCPP_HIP_OK;
}

void mcmcpp_hip_histograms_destroy(mcmcpp_hip_histograms* h)
{
    if (!h) return;
    hipSetDevice(h->device);
    delete h;  // (the stream goes idle and away, then the buffers free themselves)
}

int mcmcpp_hip_histograms_compute(mcmcpp_hip_histograms* h, const void* const* steps, int64_t n_steps)
{
    if (!h) return MCMCPP_HIP_E_ARG;
    h->have_result = false;
    if (n_steps < 0 || (n_steps > 0 && !steps)) return fail(h, MCMCPP_HIP_E_ARG, "histograms_compute: bad arguments");
    for (int64_t k = 0; k < n_steps; ++k)
        if (!steps[k]) return fail(h, MCMCPP_HIP_E_ARG, "histograms_compute: a step pointer is NULL");
    return compute_entry(h, steps, nullptr, n_steps, 1);
}

int mcmcpp_hip_histograms_compute_device(mcmcpp_hip_histograms* h, const void* device_steps, int64_t n_steps, int64_t slice_interval)
{
    if (!h) return MCMCPP_HIP_E_ARG;
    h->have_result = false;
    if (n_steps < 0 || slice_interval < 1 || (n_steps > 0 && !device_steps))
        return fail(h, MCMCPP_HIP_E_ARG, "histograms_compute_device: bad arguments");
    return compute_entry(h, nullptr, device_steps, (n_steps + slice_interval - 1) / slice_interval, slice_interval);
}

int mcmcpp_hip_histograms_result(const mcmcpp_hip_histograms* hc, int64_t* num_points, void* bounds, int64_t* single, int64_t* pairs,
                                 int64_t* clamped)
{
    mcmcpp_hip_histograms* h = const_cast<mcmcpp_hip_histograms*>(hc);
    if (!h) return MCMCPP_HIP_E_ARG;
    if (!h->have_result) return fail(h, MCMCPP_HIP_E_STATE, "histograms_result: no successful compute since creation or the last failure");
    if (pairs && !h->with_pairs) return fail(h, MCMCPP_HIP_E_ARG, "histograms_result: this handle was created without pair histograms");
    ANALYSIS_TRY(h->error, hipSetDevice(h->device));
    if (single) ANALYSIS_TRY(h->error, hipMemcpyAsync(single, h->d_single, 8 * (size_t)h->P * h->bins, hipMemcpyDeviceToHost, h->stream));
    if (pairs && h->npairs > 0)
        ANALYSIS_TRY(h->error, hipMemcpyAsync(pairs, h->d_pairs, 8 * (size_t)h->npairs * h->bins * h->bins, hipMemcpyDeviceToHost, h->stream));
    if (clamped) ANALYSIS_TRY(h->error, hipMemcpyAsync(clamped, h->d_clamped, 8 * (size_t)h->P, hipMemcpyDeviceToHost, h->stream));
    ANALYSIS_TRY(h->error, hipStreamSynchronize(h->stream));
    if (bounds) std::memcpy(bounds, h->bounds.data(), h->bounds.size());
    if (num_points) *num_points = h->points;
    return MCMCPP_HIP_OK;
}
}
