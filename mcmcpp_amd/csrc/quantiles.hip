// quantiles.hip -- exact order statistics of every parameter over stored chain steps, and the exact rank of given values: what a
// user reports from a chain (the median, the 16/84 or 2.5/97.5 bounds) without sorting it and without bringing it to the host.
// An extension: the reference has only the binned Analysis::PercentileAndMaximumFinder (histograms.hip), which stays as it is.
//
// Selection, not sorting: most-significant-digit radix select on order-preserving integer keys.
//   * key of a sample of type T (u32 for float, u64 for double): its bit pattern with all bits flipped if the sign bit is set,
//     else with the sign bit flipped: -inf < ... < -0 < +0 < ... < +inf as unsigned integers.  A NaN fails the call.
//   * state per parameter p and requested rank: a key prefix and the rank that remains among the samples with that prefix.
//     Ranks of one parameter whose prefixes coincide form one rank group and share one set of counters (all of them in the
//     first pass).
//   * one pass takes the next digit (quantile_plan.hpp: 8 bits): quant_count_kernel counts, for every (p, group), the samples
//     of p whose key starts with the group's prefix, by that digit; the host takes the digit whose cumulative count first
//     exceeds the remaining rank, subtracts the count in front of it and appends the digit to the prefix.
//   * after the last pass the prefix is the key of the order statistic, and the inverse map gives back a sample's bits.
// The kernels read the rows where they lie, lanes along the parameters: a block takes a slice of the
// samples and a tile of consecutive parameters; its counters are privatised in LDS as u32 and flushed with 64-bit integer
// atomics, or are global 64-bit atomics where the plan finds that they do not fit.  The scan between two passes runs on the
// host, on P x groups x 256 downloaded counters.  Rank counts are one streaming pass of comparisons with 64-bit sums.
// Every count is an integer sum: results are exact and independent of scheduling, slicing and chunking.
// A device chain is read in place; host chains are uploaded in chunks of MCMCPP_HIP_QUANTILE_CHUNK_MB (read per call, default
// 1024): a selection that fits one chunk is uploaded once and serves every pass, a larger one is streamed once per pass.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mcmcpp_hip.h"
#include "analysis_host.hpp"
#include "quantile_plan.hpp"

namespace
{
constexpr int kQuantThreads = 256;
static_assert(kQuantThreads == mcmcpp::kQuantPlanThreads, "quantile_plan.hpp plans for the block size of these kernels");
constexpr int kQuantUnroll = 8;  // loads a thread has in flight
constexpr int kQueryTile = mcmcpp::kQuantQueryTile;

template <class T>
struct KeyOf
{
    typedef uint64_t type;
};
template <>
struct KeyOf<float>
{
    typedef uint32_t type;
};

template <class T>
__host__ __device__ __forceinline__ typename KeyOf<T>::type to_key(T x)
{
    typedef typename KeyOf<T>::type K;
    K b;
    __builtin_memcpy(&b, &x, sizeof b);
    const K sign = K(1) << (8 * sizeof(K) - 1);
    return (b & sign) ? (K)~b : (K)(b ^ sign);
}

template <class T>
T from_key(typename KeyOf<T>::type k)
{
    typedef typename KeyOf<T>::type K;
    const K sign = K(1) << (8 * sizeof(K) - 1);
    const K b = (k & sign) ? (K)(k ^ sign) : (K)~k;
    T x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

template <class T>
__device__ __forceinline__ const T* sample_row(const T* base, long long step_stride, unsigned W, int P, unsigned s)
{
    return base + (size_t)(s / W) * (size_t)step_stride + (size_t)(s % W) * (size_t)P;
}

// One pass of the selection.  Block (slice, tile of parameters): samples [blockIdx.x * per, ...), parameters
// [blockIdx.y * tile, ...), pt of them; thread tid reads parameter tid % pt of every (256 / pt)-th row.  pref[p][groups] holds
// the prefixes (all ones: no group), cnt[p][groups][cells] the counters.  `lds`: dynamic LDS of tile * groups * (cells * 4 +
// sizeof(K)) bytes, the counters first; without it the counters are the global ones.
template <class T, bool lds>
__global__ void __launch_bounds__(kQuantThreads)
quant_count_kernel(const T* base, long long step_stride, unsigned W, int P, unsigned n, unsigned per, int tile, int groups, int shift, int bits,
                   int has_prefix, const typename KeyOf<T>::type* __restrict__ pref, unsigned long long* __restrict__ cnt, int* nan_flag)
{
    typedef typename KeyOf<T>::type K;
    extern __shared__ __align__(16) unsigned s_cnt[];
    const int cells = 1 << bits;
    const int tid = threadIdx.x;
    const int p0 = blockIdx.y * tile;
    const int pt = (P - p0 < tile) ? P - p0 : tile;
    const int rows = kQuantThreads / pt;
    const unsigned s0 = blockIdx.x * per;
    const unsigned s1 = (n - s0 < per) ? n : s0 + per;
    const int sets = pt * groups;
    K* s_pref = reinterpret_cast<K*>(s_cnt + (size_t)tile * groups * cells);  // [groups][pt]
    if (lds)
    {
        for (int e = tid; e < sets * cells; e += kQuantThreads) s_cnt[e] = 0;
        for (int e = tid; e < sets; e += kQuantThreads) s_pref[(e % groups) * pt + e / groups] = pref[(size_t)p0 * groups + e];
        __syncthreads();
    }
    if (tid < rows * pt)
    {
        const int pl = tid % pt, p = p0 + pl;
        const K* gp = pref + (size_t)p * groups;
        unsigned long long* gc = cnt + (size_t)p * groups * cells;
        unsigned* lc = s_cnt + (size_t)pl * groups * cells;
        bool nan = false;
        for (unsigned s = s0 + tid / pt; s < s1; s += rows * kQuantUnroll)
        {
            T x[kQuantUnroll];
#pragma unroll
            for (int u = 0; u < kQuantUnroll; ++u)
            {
                const unsigned su = s + u * rows;
                x[u] = su < s1 ? sample_row(base, step_stride, W, P, su)[p] : T(0);
            }
#pragma unroll
            for (int u = 0; u < kQuantUnroll; ++u)
            {
                if (s + u * rows >= s1) break;
                nan |= (x[u] != x[u]);
                const K key = to_key<T>(x[u]);
                const K hi = has_prefix ? (K)(key >> (shift + bits)) : K(0);
                const int d = (int)((key >> shift) & (K)(cells - 1));
                int mine = -1;  // (the prefixes of a parameter's groups differ: at most one matches)
                for (int g = 0; g < groups; ++g)
                    if ((lds ? s_pref[g * pt + pl] : gp[g]) == hi) mine = g;
                if (mine >= 0)
                {
                    if (lds)
                        atomicAdd(&lc[mine * cells + d], 1u);
                    else
                        atomicAdd(&gc[(size_t)mine * cells + d], 1ull);
                }
            }
        }
        if (nan) atomicOr(nan_flag, 1);
    }
    if (lds)
    {
        __syncthreads();
        unsigned long long* out = cnt + (size_t)p0 * groups * cells;  // the block's sets lie as the global ones do: [pl][g][d]
        for (int e = tid; e < sets * cells; e += kQuantThreads)
            if (s_cnt[e]) atomicAdd(&out[e], (unsigned long long)s_cnt[e]);
    }
}

// Rank counts.  Block as above; a thread takes kQueryTile queries of its parameter at a time and streams its rows once for each
// such tile: below[p][q] += #(x < v), not_above[p][q] += #(x <= v).
template <class T>
__global__ void __launch_bounds__(kQuantThreads)
quant_rank_kernel(const T* base, long long step_stride, unsigned W, int P, unsigned n, unsigned per, int tile, const T* query, int Q,
                  unsigned long long* below, unsigned long long* not_above, int* nan_flag)
{
    const int tid = threadIdx.x;
    const int p0 = blockIdx.y * tile;
    const int pt = (P - p0 < tile) ? P - p0 : tile;
    const int rows = kQuantThreads / pt;
    const unsigned s0 = blockIdx.x * per;
    const unsigned s1 = (n - s0 < per) ? n : s0 + per;
    if (tid >= rows * pt) return;
    const int p = p0 + tid % pt;
    bool nan = false;
    for (int q0 = 0; q0 < Q; q0 += kQueryTile)
    {
        T v[kQueryTile];
        unsigned lt[kQueryTile], le[kQueryTile];  // (a slice holds fewer than 2^32 samples)
#pragma unroll
        for (int j = 0; j < kQueryTile; ++j)
        {
            v[j] = q0 + j < Q ? query[(size_t)p * Q + q0 + j] : T(0);
            lt[j] = le[j] = 0;
        }
#pragma unroll 4
        for (unsigned s = s0 + tid / pt; s < s1; s += rows)
        {
            const T x = sample_row(base, step_stride, W, P, s)[p];
            nan |= (x != x);
#pragma unroll
            for (int j = 0; j < kQueryTile; ++j)
            {
                lt[j] += x < v[j];
                le[j] += x <= v[j];
            }
        }
#pragma unroll
        for (int j = 0; j < kQueryTile; ++j)
            if (q0 + j < Q)
            {
                if (lt[j]) atomicAdd(&below[(size_t)p * Q + q0 + j], (unsigned long long)lt[j]);
                if (le[j]) atomicAdd(&not_above[(size_t)p * Q + q0 + j], (unsigned long long)le[j]);
            }
    }
    if (nan) atomicOr(nan_flag, 1);
}

thread_local std::string g_quant_error;

int quant_fail(int code, const std::string& msg) { return mcmcpp::analysis_fail(g_quant_error, code, msg); }

using mcmcpp::StepSpan;

// One call's steps, how many of them make a chunk, and what the plans ask about the device
template <class T>
struct Source : mcmcpp::StepSource<T>
{
    long long per;
    int cus;
    size_t lds_limit;

    template <class F>
    int for_each_chunk(F&& f)
    {
        return mcmcpp::StepSource<T>::for_each_chunk(per, f);
    }
};

template <class T>
int order_statistics(Source<T>& src, const int64_t* ranks, int R, T* values)
{
    typedef typename KeyOf<T>::type K;
    const int key_bits = 8 * (int)sizeof(K), P = src.P;
    const int passes = mcmcpp::quantile_passes(key_bits);
    std::vector<K> prefix((size_t)P * R, K(0));
    std::vector<long long> rem((size_t)P * R);
    std::vector<int> group((size_t)P * R, 0);
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < R; ++k) rem[(size_t)p * R + k] = ranks[k];
    int groups = 1;  // the most rank groups of a parameter
    mcmcpp::DeviceBuffer<> d_pref;
    mcmcpp::DeviceBuffer<unsigned long long> d_cnt;
    mcmcpp::DeviceBuffer<int> d_nan;
    if (d_nan.alloc(sizeof(int)) != hipSuccess) return quant_fail(MCMCPP_HIP_E_NOMEM, "order_statistics: cannot allocate device memory");
    ANALYSIS_TRY(g_quant_error, hipMemsetAsync(d_nan, 0, sizeof(int), src.stream));
    std::vector<K> table;
    std::vector<unsigned long long> cnt;
    for (int pass = 0; pass < passes; ++pass)
    {
        const mcmcpp::QuantDigit dg = mcmcpp::quantile_digit(key_bits, pass);
        const int cells = 1 << dg.bits;
        const size_t sets = (size_t)P * groups;
        table.assign(sets, (K)~K(0));
        for (int p = 0; p < P; ++p)
            for (int k = 0; k < R; ++k) table[(size_t)p * groups + group[(size_t)p * R + k]] = prefix[(size_t)p * R + k];
        if (mcmcpp::grow(d_pref, sizeof(K) * sets, src.stream) != hipSuccess || mcmcpp::grow(d_cnt, 8 * sets * cells, src.stream) != hipSuccess)
            return quant_fail(MCMCPP_HIP_E_NOMEM, "order_statistics: cannot allocate the " + std::to_string(8 * sets * cells) + "-byte counters");
        ANALYSIS_TRY(g_quant_error, hipMemcpyAsync(d_pref, table.data(), sizeof(K) * sets, hipMemcpyHostToDevice, src.stream));
        ANALYSIS_TRY(g_quant_error, hipMemsetAsync(d_cnt, 0, 8 * sets * cells, src.stream));
        int rc = src.for_each_chunk([&](const StepSpan<T>& sp) -> int {
            const unsigned n = (unsigned)(sp.n_steps * src.W);
            const mcmcpp::QuantPlan plan = mcmcpp::quantile_plan(n, P, groups, key_bits, dg.bits, src.cus, src.lds_limit);
            const auto kernel = plan.lds ? quant_count_kernel<T, true> : quant_count_kernel<T, false>;
            hipLaunchKernelGGL(kernel, dim3(plan.blocks, (unsigned)plan.ptiles), dim3(kQuantThreads), plan.lds_bytes, src.stream, sp.base, sp.step_stride,
                               (unsigned)src.W, P, n, plan.per, plan.tile, groups, dg.shift, dg.bits, pass > 0 ? 1 : 0, (const K*)d_pref.get(), d_cnt.get(),
                               d_nan.get());
            ANALYSIS_TRY(g_quant_error, hipGetLastError());
            return MCMCPP_HIP_OK;
        });
        if (rc) return rc;
        cnt.resize(sets * cells);
        ANALYSIS_TRY(g_quant_error, hipMemcpyAsync(cnt.data(), d_cnt, 8 * sets * cells, hipMemcpyDeviceToHost, src.stream));
        int nan = 0;
        if (pass == 0) ANALYSIS_TRY(g_quant_error, hipMemcpyAsync(&nan, d_nan, sizeof(int), hipMemcpyDeviceToHost, src.stream));
        ANALYSIS_TRY(g_quant_error, hipStreamSynchronize(src.stream));
        if (nan) return quant_fail(MCMCPP_HIP_E_ARG, "order_statistics: the selected samples contain a NaN (it has no place in the order)");
        // the scan: the digit whose cumulative count first exceeds the remaining rank
        for (int p = 0; p < P; ++p)
            for (int k = 0; k < R; ++k)
            {
                const size_t at = (size_t)p * R + k;
                const unsigned long long* h = &cnt[((size_t)p * groups + group[at]) * cells];
                int d = 0;
                while (d < cells && (unsigned long long)rem[at] >= h[d]) rem[at] -= (long long)h[d++];
                if (d == cells) return quant_fail(MCMCPP_HIP_E_HIP, "order_statistics: the counters of a pass do not add up to the samples used");
                prefix[at] = (K)((prefix[at] << dg.bits) | (K)d);
            }
        // ranks of a parameter whose prefixes coincide share the next pass's counters
        groups = 1;
        for (int p = 0; p < P; ++p)
        {
            int count = 0;
            for (int k = 0; k < R; ++k)
            {
                int g = 0;
                while (g < k && prefix[(size_t)p * R + g] != prefix[(size_t)p * R + k]) ++g;
                group[(size_t)p * R + k] = g < k ? group[(size_t)p * R + g] : count++;
            }
            if (count > groups) groups = count;
        }
    }
    for (size_t at = 0; at < prefix.size(); ++at) values[at] = from_key<T>(prefix[at]);
    return MCMCPP_HIP_OK;
}

template <class T>
int rank_counts(Source<T>& src, const T* query, int Q, int64_t* below, int64_t* not_above)
{
    const int P = src.P;
    const size_t cells = (size_t)P * Q;
    mcmcpp::DeviceBuffer<> d_query;
    mcmcpp::DeviceBuffer<unsigned long long> d_cnt;  // below, then not_above
    mcmcpp::DeviceBuffer<int> d_nan;
    if (d_query.alloc(sizeof(T) * cells) != hipSuccess || d_cnt.alloc(16 * cells) != hipSuccess || d_nan.alloc(sizeof(int)) != hipSuccess)
        return quant_fail(MCMCPP_HIP_E_NOMEM, "rank_counts: cannot allocate device memory");
    ANALYSIS_TRY(g_quant_error, hipMemcpyAsync(d_query, query, sizeof(T) * cells, hipMemcpyHostToDevice, src.stream));
    ANALYSIS_TRY(g_quant_error, hipMemsetAsync(d_cnt, 0, 16 * cells, src.stream));
    ANALYSIS_TRY(g_quant_error, hipMemsetAsync(d_nan, 0, sizeof(int), src.stream));
    int rc = src.for_each_chunk([&](const StepSpan<T>& sp) -> int {
        const unsigned n = (unsigned)(sp.n_steps * src.W);
        const mcmcpp::QuantRankPlan plan = mcmcpp::quantile_rank_plan(n, P, src.cus);
        hipLaunchKernelGGL((quant_rank_kernel<T>), dim3(plan.blocks, (unsigned)plan.ptiles), dim3(kQuantThreads), 0, src.stream, sp.base, sp.step_stride,
                           (unsigned)src.W, P, n, plan.per, plan.tile, (const T*)d_query.get(), Q, d_cnt.get(), d_cnt.get() + cells, d_nan.get());
        ANALYSIS_TRY(g_quant_error, hipGetLastError());
        return MCMCPP_HIP_OK;
    });
    if (rc) return rc;
    std::vector<int64_t> cnt(2 * cells);
    int nan = 0;
    ANALYSIS_TRY(g_quant_error, hipMemcpyAsync(cnt.data(), d_cnt, 16 * cells, hipMemcpyDeviceToHost, src.stream));
    ANALYSIS_TRY(g_quant_error, hipMemcpyAsync(&nan, d_nan, sizeof(int), hipMemcpyDeviceToHost, src.stream));
    ANALYSIS_TRY(g_quant_error, hipStreamSynchronize(src.stream));
    if (nan) return quant_fail(MCMCPP_HIP_E_ARG, "rank_counts: the selected samples contain a NaN (it is neither below nor above a value)");
    if (below) std::memcpy(below, cnt.data(), 8 * cells);
    if (not_above) std::memcpy(not_above, cnt.data() + cells, 8 * cells);
    return MCMCPP_HIP_OK;
}

struct Request
{
    const char* what;
    int32_t dtype, device;
    const void* const* steps;
    const void* device_steps;
    bool on_device;
    int64_t n_steps, slice;
    int32_t W, P;
    const int64_t* ranks;  // order statistics
    int32_t n_ranks;
    void* values;
    const void* query;  // rank counts
    int32_t n_query;
    int64_t *below, *not_above;
};

template <class T>
bool any_nan(const void* v, size_t count)
{
    const T* x = static_cast<const T*>(v);
    for (size_t i = 0; i < count; ++i)
        if (x[i] != x[i]) return true;
    return false;
}

template <class T>
int run_request(const Request& r, int device, const hipDeviceProp_t& prop, long long used)
{
    const size_t step_bytes = sizeof(T) * (size_t)r.W * r.P;
    if (r.on_device)
        if (int rc = mcmcpp::check_device_steps(g_quant_error, r.what, r.device_steps, step_bytes * (size_t)r.n_steps, device)) return rc;
    mcmcpp::DeviceBuffer<> d_chunk;
    mcmcpp::Stream stream;  // (behind the upload buffer: the stream is idle and gone when the buffer goes)
    ANALYSIS_TRY(g_quant_error, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    // (a device chain is read in place: 32-bit sample indexing alone bounds its chunks)
    const size_t chunk_bytes = r.on_device ? std::numeric_limits<size_t>::max() : mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_QUANTILE_CHUNK_MB", 1024);
    Source<T> src{{r.steps, static_cast<const T*>(r.device_steps), used, r.slice, r.W, r.P, stream, &d_chunk, &g_quant_error},
                  mcmcpp::quantile_steps_per_chunk(chunk_bytes, step_bytes, r.W), prop.multiProcessorCount, mcmcpp::hist_lds_limit(prop.sharedMemPerBlock)};
    if (mcmcpp::grow(d_chunk, src.upload_bytes(src.per), stream) != hipSuccess)
        return quant_fail(MCMCPP_HIP_E_NOMEM, std::string(r.what) + ": cannot allocate the upload buffer");
    return r.ranks ? order_statistics<T>(src, r.ranks, r.n_ranks, static_cast<T*>(r.values))
                   : rank_counts<T>(src, static_cast<const T*>(r.query), r.n_query, r.below, r.not_above);
}

int quant_entry(const Request& r)
{
    const std::string w(r.what);
    if (r.dtype != MCMCPP_HIP_F64 && r.dtype != MCMCPP_HIP_F32) return quant_fail(MCMCPP_HIP_E_ARG, w + ": dtype must be MCMCPP_HIP_F64 or MCMCPP_HIP_F32");
    if (r.P < 1 || r.P > mcmcpp::kQuantMaxParams) return quant_fail(MCMCPP_HIP_E_ARG, w + ": 1 <= num_params <= " + std::to_string(mcmcpp::kQuantMaxParams));
    if (r.W < 1) return quant_fail(MCMCPP_HIP_E_ARG, w + ": num_walkers >= 1");
    if (r.on_device ? !r.device_steps : !r.steps) return quant_fail(MCMCPP_HIP_E_ARG, w + ": the steps must not be NULL");
    if (r.slice < 1) return quant_fail(MCMCPP_HIP_E_ARG, w + ": slice_interval >= 1");
    if (r.n_steps < 1) return quant_fail(MCMCPP_HIP_E_ARG, w + ": no samples (N == 0): n_steps >= 1");
    const long long used = (r.n_steps + r.slice - 1) / r.slice;
    const long long N = used * r.W;
    const size_t esize = r.dtype == MCMCPP_HIP_F64 ? 8 : 4;
    if (r.ranks)  // order statistics
    {
        if (r.n_ranks < 1 || r.n_ranks > mcmcpp::kQuantMaxRanks) return quant_fail(MCMCPP_HIP_E_ARG, w + ": 1 <= n_ranks <= " + std::to_string(mcmcpp::kQuantMaxRanks));
        if (!r.ranks || !r.values) return quant_fail(MCMCPP_HIP_E_ARG, w + ": ranks and values must not be NULL");
        for (int k = 0; k < r.n_ranks; ++k)
            if (r.ranks[k] < 0 || r.ranks[k] >= N)
                return quant_fail(MCMCPP_HIP_E_ARG, w + ": rank " + std::to_string(r.ranks[k]) + " is outside [0, N) with N = " + std::to_string(N) + " samples");
    }
    else
    {
        if (r.n_query < 1) return quant_fail(MCMCPP_HIP_E_ARG, w + ": n_query >= 1");
        if (!r.query) return quant_fail(MCMCPP_HIP_E_ARG, w + ": query must not be NULL");
        const size_t count = (size_t)r.P * r.n_query;
        if (esize == 8 ? any_nan<double>(r.query, count) : any_nan<float>(r.query, count))
            return quant_fail(MCMCPP_HIP_E_ARG, w + ": a query is NaN (it is neither below nor above a sample)");
    }
    if (!r.on_device)
        for (int64_t k = 0; k < r.n_steps; ++k)
            if (!r.steps[k]) return quant_fail(MCMCPP_HIP_E_ARG, w + ": a step pointer is NULL");
    hipDeviceProp_t prop;
    std::string why;
    int device = r.device;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return quant_fail(rc, w + ": " + why);
    return esize == 8 ? run_request<double>(r, device, prop, used) : run_request<float>(r, device, prop, used);
}
}  // namespace

extern "C"
{
const char* mcmcpp_hip_order_statistics_last_error(void) { return g_quant_error.c_str(); }

int mcmcpp_hip_order_statistics(int32_t dtype, int32_t device, const void* const* steps, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                                const int64_t* ranks, int32_t n_ranks, void* values)
{
    if (!ranks || !values) return quant_fail(MCMCPP_HIP_E_ARG, "order_statistics: ranks and values must not be NULL");
    return quant_entry(Request{"order_statistics", dtype, device, steps, nullptr, false, n_steps, 1, num_walkers, num_params, ranks, n_ranks, values, nullptr, 0,
                               nullptr, nullptr});
}

int mcmcpp_hip_order_statistics_device(int32_t dtype, int32_t device, const void* device_steps, int64_t n_steps, int64_t slice_interval, int32_t num_walkers,
                                       int32_t num_params, const int64_t* ranks, int32_t n_ranks, void* values)
{
    if (!ranks || !values) return quant_fail(MCMCPP_HIP_E_ARG, "order_statistics_device: ranks and values must not be NULL");
    return quant_entry(Request{"order_statistics_device", dtype, device, nullptr, device_steps, true, n_steps, slice_interval, num_walkers, num_params, ranks,
                               n_ranks, values, nullptr, 0, nullptr, nullptr});
}

int mcmcpp_hip_rank_counts(int32_t dtype, int32_t device, const void* const* steps, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                           const void* query, int32_t n_query, int64_t* below, int64_t* not_above)
{
    return quant_entry(Request{"rank_counts", dtype, device, steps, nullptr, false, n_steps, 1, num_walkers, num_params, nullptr, 0, nullptr, query, n_query, below,
                               not_above});
}

int mcmcpp_hip_rank_counts_device(int32_t dtype, int32_t device, const void* device_steps, int64_t n_steps, int64_t slice_interval, int32_t num_walkers,
                                  int32_t num_params, const void* query, int32_t n_query, int64_t* below, int64_t* not_above)
{
    return quant_entry(Request{"rank_counts_device", dtype, device, nullptr, device_steps, true, n_steps, slice_interval, num_walkers, num_params, nullptr, 0, nullptr,
                               query, n_query, below, not_above});
}
}
