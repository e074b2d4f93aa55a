// rank_kernels.hpp -- what rank.hip and summary.hip share: the order-preserving keys, where the draws of the sequences lie, the
// NaN, gather, sort, score, pick and indicator kernels, and the Ranker that sorts a tile of parameters.  The kernels are
// described at the head of rank.hip; the plan of a sort is rank_plan.hpp's.  Everything lies in an unnamed namespace: each of
// the two translation units has its own instances.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mcmcpp_hip.h"
#include "analysis_host.hpp"
#include "normal_score.hpp"
#include "rank_plan.hpp"
#include "rhat_state.hpp"

namespace
{
constexpr int kThreads = mcmcpp::kRankThreads;
constexpr int kDigits = mcmcpp::kRankDigits;
constexpr int kWaves = mcmcpp::kRankWaves;
constexpr int kRounds = mcmcpp::kRankItemsPerThread;

// -inf < ... < -0 < +0 < ... < +inf as unsigned integers (quantiles.hip's order)
__device__ __forceinline__ uint32_t to_key(float x)
{
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ uint64_t to_key(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    return (b & 0x8000000000000000ULL) ? ~b : (b ^ 0x8000000000000000ULL);
}
__device__ __forceinline__ double key_value(uint32_t k)
{
    const uint32_t b = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float x;
    __builtin_memcpy(&x, &b, 4);
    return (double)x;
}
__device__ __forceinline__ double key_value(uint64_t k)
{
    const uint64_t b = (k & 0x8000000000000000ULL) ? (k ^ 0x8000000000000000ULL) : ~k;
    double x;
    __builtin_memcpy(&x, &b, 8);
    return x;
}
// the keys of -0 and +0 are neighbours: [lo, hi] is the run of keys that equal k as numbers
template <class K>
__device__ __forceinline__ void numeric_run(K k, K* lo, K* hi)
{
    const K pos0 = K(1) << (8 * sizeof(K) - 1), neg0 = pos0 - 1;
    *lo = k == pos0 ? neg0 : k;
    *hi = k == neg0 ? pos0 : k;
}

// Where the draws lie: draw j = (k HL + t) W + w; step t of a chain's sequences is its used step t (t < L) or n - L + (t - L)
template <class T>
struct Draws
{
    const T* base;
    long long step_stride, chain_stride;  // elements
    long long n, L, HL;
    int W, P;
    unsigned S;
};
template <class T>
__device__ __forceinline__ const T* draw_row(const Draws<T>& d, unsigned j)
{
    const long long per_chain = d.HL * d.W;
    const long long k = j / per_chain, rem = j % per_chain;
    const long long t = rem / d.W, w = rem % d.W;
    const long long g = t < d.L ? t : d.n - d.L + (t - d.L);
    return d.base + k * d.chain_stride + g * d.step_stride + w * d.P;
}

// thread (draw j, parameter p) over all S x P draws: a NaN raises the flag
template <class T>
__global__ void __launch_bounds__(kThreads) rank_nan_kernel(Draws<T> d, int* nan_flag)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)d.S * d.P) return;
    const T x = draw_row(d, (unsigned)(id / d.P))[id % d.P];
    if (x != x) atomicOr(nan_flag, 1);
}

template <class T, class K, bool Fold>
__global__ void __launch_bounds__(kThreads) rank_gather_kernel(Draws<T> d, int p0, const double* __restrict__ median, K* __restrict__ keys, unsigned* __restrict__ idx)
{
    const unsigned j = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (j >= d.S) return;
    const int p = p0 + (int)blockIdx.y;
    const T x = draw_row(d, j)[p];
    const size_t at = (size_t)blockIdx.y * d.S + j;
    if (Fold)
        keys[at] = (K)to_key(fabs((double)x - median[p]));
    else if (sizeof(K) == 4)
        keys[at] = (K)to_key((float)x);
    else
        keys[at] = (K)to_key((double)x);
    idx[at] = j;
}

// table [parameter][digit][block]
template <class K>
__global__ void __launch_bounds__(kThreads) rank_histogram_kernel(const K* __restrict__ keys, unsigned S, int shift, unsigned* __restrict__ table)
{
    __shared__ unsigned s_hist[kDigits];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const K* k = keys + (size_t)blockIdx.y * S;
    long long first, count;
    mcmcpp::rank_block_span(S, blockIdx.x, &first, &count);
#pragma unroll
    for (int i = 0; i < kRounds; ++i)
    {
        const long long at = i * kThreads + threadIdx.x;
        if (at < count) atomicAdd(&s_hist[(unsigned)(k[first + at] >> shift) & (kDigits - 1)], 1u);
    }
    __syncthreads();
    table[((size_t)blockIdx.y * kDigits + threadIdx.x) * gridDim.x + blockIdx.x] = s_hist[threadIdx.x];
}

// the exclusive scan of the 256 values the threads of a block hold (s_scan: 256 words); *total: their sum
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* s_scan, unsigned* total)
{
    const unsigned t = threadIdx.x;
    s_scan[t] = v;
    __syncthreads();
    unsigned sum = v;
#pragma unroll
    for (int step = 1; step < kThreads; step <<= 1)
    {
        const unsigned other = t >= (unsigned)step ? s_scan[t - step] : 0u;
        __syncthreads();
        sum += other;
        s_scan[t] = sum;
        __syncthreads();
    }
    *total = s_scan[kThreads - 1];
    __syncthreads();
    return sum - v;
}

// Block (digit, parameter): row [blocks] of the table -> its exclusive scan in place; totals [parameter][digit]
__global__ void __launch_bounds__(kThreads) rank_scan_kernel(unsigned* __restrict__ table, unsigned blocks, unsigned* __restrict__ totals)
{
    __shared__ unsigned s_scan[kThreads];
    unsigned* row = table + ((size_t)blockIdx.y * kDigits + blockIdx.x) * blocks;
    const unsigned per = (blocks + kThreads - 1) / kThreads;
    const unsigned b0 = threadIdx.x * per < blocks ? threadIdx.x * per : blocks, b1 = b0 + per < blocks ? b0 + per : blocks;
    unsigned mine = 0;
    for (unsigned b = b0; b < b1; ++b) mine += row[b];
    unsigned total;
    unsigned run = block_exclusive_scan(mine, s_scan, &total);
    for (unsigned b = b0; b < b1; ++b)
    {
        const unsigned c = row[b];
        row[b] = run;
        run += c;
    }
    if (threadIdx.x == 0) totals[(size_t)blockIdx.y * kDigits + blockIdx.x] = total;
}

template <class K>
__global__ void __launch_bounds__(kThreads)
rank_scatter_kernel(const K* __restrict__ keys_in, const unsigned* __restrict__ idx_in, K* __restrict__ keys_out, unsigned* __restrict__ idx_out, unsigned S, int shift,
                    const unsigned* __restrict__ table, const unsigned* __restrict__ totals, int* fault)
{
    __shared__ unsigned s_scan[kThreads];
    __shared__ unsigned s_base[kDigits];         // where the block's next draw of a digit goes
    __shared__ unsigned s_wave[kWaves][kDigits];  // a round's counts of the wavefronts, then their offsets
    const unsigned tid = threadIdx.x, wave = tid / mcmcpp::kRankWave;
    const size_t param = blockIdx.y;
    const K* kin = keys_in + param * S;
    const unsigned* iin = idx_in + param * S;
    K* kout = keys_out + param * S;
    unsigned* iout = idx_out + param * S;
    unsigned all;
    const unsigned digit_first = block_exclusive_scan(totals[param * kDigits + tid], s_scan, &all);
    s_base[tid] = digit_first + table[(param * kDigits + tid) * gridDim.x + blockIdx.x];
    long long first, count;
    mcmcpp::rank_block_span(S, blockIdx.x, &first, &count);
    for (int i = 0; i < kRounds; ++i)
    {
        const long long at = i * kThreads + tid;
        const bool valid = at < count;
        const long long j = first + at;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s_wave[w][tid] = 0;
        __syncthreads();
        K key = 0;
        unsigned id = 0, digit = 0;
        if (valid)
        {
            key = kin[j];
            id = iin[j];
            digit = (unsigned)(key >> shift) & (kDigits - 1);
        }
        // the lanes of this wavefront that hold a draw of the same digit
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < mcmcpp::kRankDigitBits; ++b)
        {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long set = __ballot(valid && bit);
            peers &= bit ? set : ~set;
        }
        const unsigned before = __builtin_amdgcn_mbcnt_hi((unsigned)(peers >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)peers, 0u));
        if (valid && before == 0) s_wave[wave][digit] = (unsigned)__popcll(peers);
        __syncthreads();
        {
            unsigned run = s_base[tid];  // thread = digit: the wavefronts in order
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
            {
                const unsigned c = s_wave[w][tid];
                s_wave[w][tid] = run;
                run += c;
            }
            s_base[tid] = run;
        }
        __syncthreads();
        if (valid)
        {
            const unsigned dst = s_wave[wave][digit] + before;
            if (dst < S)  // (it is, by the histogram of the same keys; were it ever not, the call fails and says so)
            {
                kout[dst] = key;
                iout[dst] = id;
            }
            else
                atomicOr(fault, 1);
        }
        __syncthreads();
    }
}

// Thread (sorted position i, parameter): the run of its key -> the score at the draw's place
template <class K>
__global__ void __launch_bounds__(kThreads) rank_score_kernel(const K* __restrict__ keys, const unsigned* __restrict__ idx, unsigned S, int p0, int P, double* __restrict__ scores)
{
    const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (i >= S) return;
    const K* k = keys + (size_t)blockIdx.y * S;
    K lo_key, hi_key;
    numeric_run<K>(k[i], &lo_key, &hi_key);
    unsigned a = 0, b = i;  // first position whose key >= lo_key: in [0, i]
    while (a < b)
    {
        const unsigned m = a + (b - a) / 2;
        if (k[m] < lo_key)
            a = m + 1;
        else
            b = m;
    }
    const unsigned below = a;
    a = i + 1;  // first position whose key > hi_key: in [i + 1, S]
    b = S;
    while (a < b)
    {
        const unsigned m = a + (b - a) / 2;
        if (k[m] <= hi_key)
            a = m + 1;
        else
            b = m;
    }
    const unsigned j = idx[(size_t)blockIdx.y * S + i];
    scores[(size_t)j * P + p0 + blockIdx.y] = mcmcpp::normal_score_of_rank(below, a - below, S);
}

struct PickRanks
{
    unsigned r[6];
};
// thread (one of six ranks, parameter of the tile): picked [parameter][6]
template <class K>
__global__ void rank_pick_kernel(const K* __restrict__ keys, unsigned S, PickRanks ranks, double* __restrict__ picked)
{
    if (threadIdx.x < 6) picked[blockIdx.x * 6 + threadIdx.x] = key_value(keys[(size_t)blockIdx.x * S + ranks.r[threadIdx.x]]);
}

template <class T>
__global__ void __launch_bounds__(kThreads) rank_indicator_kernel(Draws<T> d, const double* __restrict__ q, double* __restrict__ out)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)d.S * d.P) return;
    const int p = (int)(id % d.P);
    out[id] = (double)draw_row(d, (unsigned)(id / d.P))[p] <= q[p] ? 1.0 : 0.0;
}

struct Quantiles
{
    std::vector<double> median, q05, q95;
};

// Everything one call shares: the draws, the stream, the workspace of a tile.  *err is the message slot of the caller's family.
template <class T>
struct Ranker
{
    typedef typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type OwnKey;  // the key of a draw as it is

    Draws<T> d;
    int P = 0, tile = 0;
    long long S = 0;
    hipStream_t stream = nullptr;
    mcmcpp::DeviceBuffer<char> work;
    mcmcpp::DeviceBuffer<double> d_picked, d_median;
    mcmcpp::DeviceBuffer<int> d_fault;  // raised by a scatter whose destination lies outside the draws: never, by construction
    mcmcpp::RankLayout lay;
    std::string what;
    std::string* err = nullptr;

    int fail(int code, const std::string& msg) const { return mcmcpp::analysis_fail(*err, code, msg); }

    // the workspace for keys of key_bits (the widest the call sorts)
    int prepare(int key_bits)
    {
        tile = mcmcpp::rank_param_tile(S, P, key_bits, mcmcpp::rank_work_bytes_from_env());
        lay = mcmcpp::rank_layout(S, key_bits, tile);
        if (work.alloc(lay.bytes) != hipSuccess)
        {
            tile = 1;
            lay = mcmcpp::rank_layout(S, key_bits, 1);
            if (work.alloc(lay.bytes) != hipSuccess)
                return fail(MCMCPP_HIP_E_NOMEM, what + ": cannot allocate the " + std::to_string(lay.bytes) + " bytes of the sort of one parameter");
        }
        if (d_picked.alloc(8 * 6 * (size_t)tile) != hipSuccess || d_median.alloc(8 * (size_t)P) != hipSuccess || d_fault.alloc(sizeof(int)) != hipSuccess)
            return fail(MCMCPP_HIP_E_NOMEM, what + ": cannot allocate the order statistics");
        ANALYSIS_TRY(*err, hipMemsetAsync(d_fault.get(), 0, sizeof(int), stream));
        return MCMCPP_HIP_OK;
    }

    // the sorted keys of the tile rank_tile<K, ...> sorted last: [parameter of the tile][S]
    template <class K>
    const K* sorted_keys() const
    {
        return reinterpret_cast<const K*>(work.get() + lay.keys_a);
    }

    // Parameters [p0, p0 + now): gather, sort; then the order statistics into *quant (if given) and the scores into the chain
    // `scores` (if given).  The stream is idle on return where quant is given.
    template <class K, bool Fold>
    int rank_tile(int p0, int now, Quantiles* quant, double* scores)
    {
        const unsigned n32 = (unsigned)S;
        K* keys[2] = {reinterpret_cast<K*>(work.get() + lay.keys_a), reinterpret_cast<K*>(work.get() + lay.keys_b)};
        unsigned* idx[2] = {reinterpret_cast<unsigned*>(work.get() + lay.idx_a), reinterpret_cast<unsigned*>(work.get() + lay.idx_b)};
        unsigned* table = reinterpret_cast<unsigned*>(work.get() + lay.table);
        unsigned* totals = reinterpret_cast<unsigned*>(work.get() + lay.totals);
        const unsigned draw_blocks = (unsigned)mcmcpp::rank_draw_blocks(S), blocks = (unsigned)mcmcpp::rank_blocks(S);
        hipLaunchKernelGGL((rank_gather_kernel<T, K, Fold>), dim3(draw_blocks, now), dim3(kThreads), 0, stream, d, p0, (const double*)d_median.get(), keys[0], idx[0]);
        ANALYSIS_TRY(*err, hipGetLastError());
        const int passes = mcmcpp::rank_passes(8 * (int)sizeof(K));
        for (int pass = 0; pass < passes; ++pass)
        {
            const int from = pass & 1, to = from ^ 1, shift = mcmcpp::rank_digit_shift(pass);
            hipLaunchKernelGGL(rank_histogram_kernel<K>, dim3(blocks, now), dim3(kThreads), 0, stream, (const K*)keys[from], n32, shift, table);
            ANALYSIS_TRY(*err, hipGetLastError());
            hipLaunchKernelGGL(rank_scan_kernel, dim3(kDigits, now), dim3(kThreads), 0, stream, table, blocks, totals);
            ANALYSIS_TRY(*err, hipGetLastError());
            hipLaunchKernelGGL(rank_scatter_kernel<K>, dim3(blocks, now), dim3(kThreads), 0, stream, (const K*)keys[from], (const unsigned*)idx[from], keys[to], idx[to], n32,
                               shift, (const unsigned*)table, (const unsigned*)totals, d_fault.get());
            ANALYSIS_TRY(*err, hipGetLastError());
        }
        // (an even number of passes: the sorted keys are in keys[0])
        if (scores)
        {
            hipLaunchKernelGGL(rank_score_kernel<K>, dim3(draw_blocks, now), dim3(kThreads), 0, stream, (const K*)keys[0], (const unsigned*)idx[0], n32, p0, P, scores);
            ANALYSIS_TRY(*err, hipGetLastError());
        }
        if (quant)
        {
            const double qs[3] = {0.5, 0.05, 0.95};
            mcmcpp::RankQuantile rq[3];
            PickRanks ranks;
            for (int i = 0; i < 3; ++i)
            {
                rq[i] = mcmcpp::rank_quantile(qs[i], S);
                ranks.r[2 * i] = (unsigned)rq[i].lo;
                ranks.r[2 * i + 1] = (unsigned)rq[i].hi;
            }
            hipLaunchKernelGGL(rank_pick_kernel<K>, dim3(now), dim3(64), 0, stream, (const K*)keys[0], n32, ranks, d_picked.get());
            ANALYSIS_TRY(*err, hipGetLastError());
            std::vector<double> picked(6 * (size_t)now);
            ANALYSIS_TRY(*err, hipMemcpyAsync(picked.data(), d_picked.get(), 8 * picked.size(), hipMemcpyDeviceToHost, stream));
            ANALYSIS_TRY(*err, hipStreamSynchronize(stream));
            for (int i = 0; i < now; ++i)
            {
                const double* x = picked.data() + 6 * (size_t)i;
                quant->median[p0 + i] = mcmcpp::rank_quantile_value(x[0], x[1], rq[0]);
                quant->q05[p0 + i] = mcmcpp::rank_quantile_value(x[2], x[3], rq[1]);
                quant->q95[p0 + i] = mcmcpp::rank_quantile_value(x[4], x[5], rq[2]);
            }
        }
        return MCMCPP_HIP_OK;
    }

    // the call fails where a sort pass has raised the fault flag
    int check_fault()
    {
        int fault = 0;
        ANALYSIS_TRY(*err, hipMemcpyAsync(&fault, d_fault.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(*err, hipStreamSynchronize(stream));
        if (fault) return fail(MCMCPP_HIP_E_UNSUPPORTED, what + ": internal error: a sort pass placed a draw outside the draws (histogram and scatter disagree)");
        return MCMCPP_HIP_OK;
    }

    // every parameter, tile by tile: the draws as they are (quant and / or scores), or folded about d_median (scores)
    int rank_all(bool fold, Quantiles* quant, double* scores)
    {
        for (int t = 0; t < mcmcpp::rank_tiles(P, tile); ++t)
        {
            const int p0 = t * tile, now = P - p0 < tile ? P - p0 : tile;
            const int rc = fold ? rank_tile<uint64_t, true>(p0, now, quant, scores) : rank_tile<OwnKey, false>(p0, now, quant, scores);
            if (rc) return rc;
        }
        return check_fault();
    }

    // the medians the fold is about; a fold about a median that is not finite has NaN values, which have no place in the order
    int set_fold_center(const Quantiles& quant)
    {
        for (int p = 0; p < P; ++p)
            if (!std::isfinite(quant.median[p]))
                return fail(MCMCPP_HIP_E_ARG, what + ": the median of parameter " + std::to_string(p) + " is not finite: a folded draw is NaN (it has no place in the order)");
        ANALYSIS_TRY(*err, hipMemcpyAsync(d_median.get(), quant.median.data(), 8 * (size_t)P, hipMemcpyHostToDevice, stream));
        return MCMCPP_HIP_OK;
    }

    // Where the draws of request r lie (the caller has checked a device chain's range): a device chain in place; host chains
    // uploaded once into d_up, as the sequences' steps [K][HL][W][P] -- a middle step that belongs to no sequence stays on the
    // host.  Then the NaN check: a NaN fails the call before anything is written.  Sets d, P, S, what.
    int locate_draws(const mcmcpp::RhatRequest& r, long long n, const mcmcpp::RhatShape& shape, mcmcpp::DeviceBuffer<T>& d_up, mcmcpp::DeviceBuffer<int>& d_nan)
    {
        const int K = r.K;
        const long long E = (long long)r.W * r.P, L = shape.L, HL = (long long)shape.H * L;
        const size_t step_bytes = sizeof(T) * (size_t)E, chain_elems = (size_t)K * HL * E;
        P = r.P;
        S = shape.M * L;
        what = r.what;
        d.W = r.W;
        d.P = P;
        d.S = (unsigned)S;
        d.L = L;
        d.HL = HL;
        if (r.on_device)
        {
            d.base = static_cast<const T*>(r.device_steps);
            d.step_stride = r.slice * E;
            d.chain_stride = (r.chain_stride_steps ? r.chain_stride_steps : r.n_steps) * E;
            d.n = n;
        }
        else
        {
            if (d_up.alloc(sizeof(T) * chain_elems) != hipSuccess) return fail(MCMCPP_HIP_E_NOMEM, what + ": cannot allocate the " + std::to_string(sizeof(T) * chain_elems) + " bytes of the uploaded chains");
            const long long per = mcmcpp::rank_steps_per_chunk(mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_RHAT_CHUNK_MB", 1024), step_bytes);
            const long long a1 = mcmcpp::rhat_half_begin(n, L, 1);
            for (int k = 0; k < K; ++k)
            {
                const void* const* src = r.steps + (size_t)k * n;
                const auto src_of = [&](long long t) { return src[t < L ? t : a1 + (t - L)]; };
                for (long long t0 = 0; t0 < HL; t0 += per)
                    ANALYSIS_TRY(*err, mcmcpp::copy_steps(d_up.get() + ((size_t)k * HL + t0) * E, src_of, t0, HL - t0 < per ? HL - t0 : per, step_bytes, hipMemcpyHostToDevice, stream));
            }
            d.base = d_up.get();
            d.step_stride = E;
            d.chain_stride = HL * E;
            d.n = HL;
        }
        if (d_nan.alloc(sizeof(int)) != hipSuccess) return fail(MCMCPP_HIP_E_NOMEM, what + ": cannot allocate device memory");
        ANALYSIS_TRY(*err, hipMemsetAsync(d_nan.get(), 0, sizeof(int), stream));
        hipLaunchKernelGGL(rank_nan_kernel<T>, dim3((unsigned)mcmcpp::rank_element_blocks(S, P)), dim3(kThreads), 0, stream, d, d_nan.get());
        ANALYSIS_TRY(*err, hipGetLastError());
        int nan = 0;
        ANALYSIS_TRY(*err, hipMemcpyAsync(&nan, d_nan.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(*err, hipStreamSynchronize(stream));
        if (nan) return fail(MCMCPP_HIP_E_ARG, what + ": the draws contain a NaN (it has no place in the order)");
        return MCMCPP_HIP_OK;
    }
};

// What every entry point of the two families refuses before a device is opened, beyond the Gelman-Rubin call's own checks
inline int rank_check_draw_counts(std::string& err, const std::string& w, const mcmcpp::RhatShape& shape, int P)
{
    if ((double)shape.M * (double)shape.L > (double)mcmcpp::kRankMaxDraws)
        return mcmcpp::analysis_fail(err, MCMCPP_HIP_E_ARG, w + ": at most 2^31 - 1 draws of a parameter can be ranked (S = M L)");
    if (!mcmcpp::rank_grids_fit(shape.M * shape.L, P))
        return mcmcpp::analysis_fail(err, MCMCPP_HIP_E_ARG, w + ": too many draws in all: S x num_params must not exceed 256 x (2^31 - 1)");
    return MCMCPP_HIP_OK;
}
}  // namespace
