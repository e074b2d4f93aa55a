// rank.hip -- the normal scores of the draws of every parameter, and the rank-normalised diagnostics of Vehtari, Gelman, Simpson,
// Carpenter and Buerkner (2021) that rest on them: rank-normalised split R-hat (bulk and folded), bulk-ESS and tail-ESS, over
// the sequences of rhat.hip / ess.hip.  An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_normal_scores and mcmcpp_hip_rank_diagnostics).  Ranks are
// integers, found exactly; the score of a rank is normal_score.hpp's, one value in bits on device and host.  The diagnostics are
// the existing entry points (mcmcpp_hip_effective_sample_size_device, mcmcpp_hip_gelman_rubin_device) run on fp64 chains this
// file builds in device memory: their bits, by construction.
//
// Per tile of parameters (rank_plan.hpp; blockIdx.y is the parameter of the tile in every kernel):
//   * rank_gather_kernel: draw j = (k HL + t) W + w of parameter p -> order-preserving key (quantiles.hip's to_key) and the
//     draw index j.  Folded: the key of |x - median| in double.
//   * the LSD radix sort, 8-bit digits, stable, key + index; a pass is three launches:
//       rank_histogram_kernel   per-block digit counts in LDS (integer LDS atomics) -> table [digit][block]
//       rank_scan_kernel        one workgroup a digit: the exclusive scan of its row of the table, and the digit's total
//       rank_scatter_kernel     digit bases from the totals; a block walks its span in rounds of 256 draws: lanes of equal
//                               digit rank themselves inside their wavefront by eight 64-bit ballots and mbcnt, wavefronts
//                               through LDS; the rounds follow each other in the draws' order, so the pass is stable.
//     No workgroup waits for another: every dependence is a kernel boundary.
//   * rank_score_kernel: sorted position i -> below = first position of its key, equal = length of its run, both by binary
//     search in the sorted keys (-0 and +0 are one run: their keys are neighbours); z = normal_score_of_rank; stored at the
//     draw's place j P + p of the fp64 score chain [K][H L][W][P].
//   * rank_pick_kernel: the six order statistics of median, q05 and q95 from the sorted keys (which keep -0 below +0: the
//     total order of mcmcpp_hip_order_statistics).
//   * rank_indicator_kernel: 1.0 / 0.0 of x <= q[p], compared in double.
// A device chain is read in place.  Host chains are uploaded once, as the sequences' steps [K][H L][W][P], in copy groups of
// MCMCPP_HIP_RHAT_CHUNK_MB.
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

thread_local std::string g_rank_error;

int rank_fail(int code, const std::string& msg) { return mcmcpp::analysis_fail(g_rank_error, code, msg); }

struct Quantiles
{
    std::vector<double> median, q05, q95;
};

// Everything one call shares: the draws, the stream, the workspace of a tile
template <class T>
struct Ranker
{
    Draws<T> d;
    int P = 0, tile = 0;
    long long S = 0;
    hipStream_t stream = nullptr;
    mcmcpp::DeviceBuffer<char> work;
    mcmcpp::DeviceBuffer<double> d_picked, d_median;
    mcmcpp::DeviceBuffer<int> d_fault;  // raised by a scatter whose destination lies outside the draws: never, by construction
    mcmcpp::RankLayout lay;
    std::string what;

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
                return rank_fail(MCMCPP_HIP_E_NOMEM, what + ": cannot allocate the " + std::to_string(lay.bytes) + " bytes of the sort of one parameter");
        }
        if (d_picked.alloc(8 * 6 * (size_t)tile) != hipSuccess || d_median.alloc(8 * (size_t)P) != hipSuccess || d_fault.alloc(sizeof(int)) != hipSuccess)
            return rank_fail(MCMCPP_HIP_E_NOMEM, what + ": cannot allocate the order statistics");
        ANALYSIS_TRY(g_rank_error, hipMemsetAsync(d_fault.get(), 0, sizeof(int), stream));
        return MCMCPP_HIP_OK;
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
        ANALYSIS_TRY(g_rank_error, hipGetLastError());
        const int passes = mcmcpp::rank_passes(8 * (int)sizeof(K));
        for (int pass = 0; pass < passes; ++pass)
        {
            const int from = pass & 1, to = from ^ 1, shift = mcmcpp::rank_digit_shift(pass);
            hipLaunchKernelGGL(rank_histogram_kernel<K>, dim3(blocks, now), dim3(kThreads), 0, stream, (const K*)keys[from], n32, shift, table);
            ANALYSIS_TRY(g_rank_error, hipGetLastError());
            hipLaunchKernelGGL(rank_scan_kernel, dim3(kDigits, now), dim3(kThreads), 0, stream, table, blocks, totals);
            ANALYSIS_TRY(g_rank_error, hipGetLastError());
            hipLaunchKernelGGL(rank_scatter_kernel<K>, dim3(blocks, now), dim3(kThreads), 0, stream, (const K*)keys[from], (const unsigned*)idx[from], keys[to], idx[to], n32,
                               shift, (const unsigned*)table, (const unsigned*)totals, d_fault.get());
            ANALYSIS_TRY(g_rank_error, hipGetLastError());
        }
        // (an even number of passes: the sorted keys are in keys[0])
        if (scores)
        {
            hipLaunchKernelGGL(rank_score_kernel<K>, dim3(draw_blocks, now), dim3(kThreads), 0, stream, (const K*)keys[0], (const unsigned*)idx[0], n32, p0, P, scores);
            ANALYSIS_TRY(g_rank_error, hipGetLastError());
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
            ANALYSIS_TRY(g_rank_error, hipGetLastError());
            std::vector<double> picked(6 * (size_t)now);
            ANALYSIS_TRY(g_rank_error, hipMemcpyAsync(picked.data(), d_picked.get(), 8 * picked.size(), hipMemcpyDeviceToHost, stream));
            ANALYSIS_TRY(g_rank_error, hipStreamSynchronize(stream));
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

    // every parameter, tile by tile: the draws as they are (quant and / or scores), or folded about d_median (scores)
    int rank_all(bool fold, Quantiles* quant, double* scores)
    {
        for (int t = 0; t < mcmcpp::rank_tiles(P, tile); ++t)
        {
            const int p0 = t * tile, now = P - p0 < tile ? P - p0 : tile;
            typedef typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type OwnKey;
            const int rc = fold ? rank_tile<uint64_t, true>(p0, now, quant, scores) : rank_tile<OwnKey, false>(p0, now, quant, scores);
            if (rc) return rc;
        }
        int fault = 0;
        ANALYSIS_TRY(g_rank_error, hipMemcpyAsync(&fault, d_fault.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(g_rank_error, hipStreamSynchronize(stream));
        if (fault) return rank_fail(MCMCPP_HIP_E_UNSUPPORTED, what + ": internal error: a sort pass placed a draw outside the draws (histogram and scatter disagree)");
        return MCMCPP_HIP_OK;
    }

    // the medians the fold is about; a fold about a median that is not finite has NaN values, which have no place in the order
    int set_fold_center(const Quantiles& quant)
    {
        for (int p = 0; p < P; ++p)
            if (!std::isfinite(quant.median[p]))
                return rank_fail(MCMCPP_HIP_E_ARG, what + ": the median of parameter " + std::to_string(p) + " is not finite: a folded draw is NaN (it has no place in the order)");
        ANALYSIS_TRY(g_rank_error, hipMemcpyAsync(d_median.get(), quant.median.data(), 8 * (size_t)P, hipMemcpyHostToDevice, stream));
        return MCMCPP_HIP_OK;
    }
};

struct ScoreOutputs
{
    double *scores, *median, *q05, *q95;
    int64_t *sequence_length, *num_sequences;
};
struct DiagOutputs
{
    double *rhat, *rhat_rank, *rhat_folded, *ess_bulk, *ess_tail, *ess_tail_lower, *ess_tail_upper, *median, *q05, *q95;
    int64_t *closed_bulk, *closed_tail, *sequence_length, *num_sequences;
};
struct Request
{
    mcmcpp::RhatRequest in;
    bool diagnostics;
    int32_t fold;
    int64_t max_lag;
    ScoreOutputs so;
    DiagOutputs dg;
};

// the scores' buffer of the device form: memory of this device, and large enough
int check_scores_buffer(const std::string& w, const void* p, size_t bytes, int device)
{
    const mcmcpp::DeviceRange r = mcmcpp::probe_device_range(p, device);
    switch (r.kind)
    {
    case mcmcpp::DeviceRange::NotDevice: return rank_fail(MCMCPP_HIP_E_ARG, w + ": scores is not device memory");
    case mcmcpp::DeviceRange::OtherDevice:
        return rank_fail(MCMCPP_HIP_E_ARG, w + ": scores is memory of device " + std::to_string(r.device) + ", not of device " + std::to_string(device));
    case mcmcpp::DeviceRange::NoAllocation: return rank_fail(MCMCPP_HIP_E_ARG, w + ": the runtime does not know the allocation scores lies in");
    case mcmcpp::DeviceRange::Found: break;
    }
    if (bytes > r.room) return rank_fail(MCMCPP_HIP_E_ARG, w + ": the " + std::to_string(bytes) + " bytes of the scores do not end inside the allocation around scores");
    return MCMCPP_HIP_OK;
}

template <class T>
int run_request(const Request& q, int device, long long n, const mcmcpp::RhatShape& shape)
{
    const mcmcpp::RhatRequest& r = q.in;
    const std::string w(r.what);
    const int K = r.K, P = r.P, H = shape.H;
    const long long E = (long long)r.W * P, L = shape.L, HL = (long long)H * L, S = shape.M * L;
    const size_t step_bytes = sizeof(T) * (size_t)E, chain_elems = (size_t)K * HL * E;
    const long long chain_stride_steps = r.chain_stride_steps ? r.chain_stride_steps : r.n_steps;
    if (r.on_device)
    {
        if (int rc = mcmcpp::check_device_steps(g_rank_error, r.what, r.device_steps, step_bytes * (size_t)((K - 1) * chain_stride_steps + r.n_steps), device)) return rc;
        if (!q.diagnostics)
            if (int rc = check_scores_buffer(w, q.so.scores, 8 * chain_elems, device)) return rc;
    }
    mcmcpp::DeviceBuffer<T> d_up;
    mcmcpp::DeviceBuffer<double> d_chain, d_q;
    mcmcpp::DeviceBuffer<int> d_nan;
    Ranker<T> rk;
    mcmcpp::Stream stream;  // (behind the buffers: the stream is idle and gone when they go)
    ANALYSIS_TRY(g_rank_error, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    rk.stream = stream;
    rk.P = P;
    rk.S = S;
    rk.what = w;
    Draws<T>& d = rk.d;
    d.W = r.W;
    d.P = P;
    d.S = (unsigned)S;
    d.L = L;
    d.HL = HL;
    if (r.on_device)
    {
        d.base = static_cast<const T*>(r.device_steps);
        d.step_stride = r.slice * E;
        d.chain_stride = chain_stride_steps * E;
        d.n = n;
    }
    else
    {
        // the sequences' steps [K][HL][W][P], uploaded once: a middle step that belongs to no sequence stays on the host
        if (d_up.alloc(sizeof(T) * chain_elems) != hipSuccess) return rank_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(sizeof(T) * chain_elems) + " bytes of the uploaded chains");
        const long long per = mcmcpp::rank_steps_per_chunk(mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_RHAT_CHUNK_MB", 1024), step_bytes);
        const long long a1 = mcmcpp::rhat_half_begin(n, L, 1);
        for (int k = 0; k < K; ++k)
        {
            const void* const* src = r.steps + (size_t)k * n;
            const auto src_of = [&](long long t) { return src[t < L ? t : a1 + (t - L)]; };
            for (long long t0 = 0; t0 < HL; t0 += per)
                ANALYSIS_TRY(g_rank_error, mcmcpp::copy_steps(d_up.get() + ((size_t)k * HL + t0) * E, src_of, t0, HL - t0 < per ? HL - t0 : per, step_bytes, hipMemcpyHostToDevice, stream));
        }
        d.base = d_up.get();
        d.step_stride = E;
        d.chain_stride = HL * E;
        d.n = HL;
    }
    const unsigned all_blocks = (unsigned)mcmcpp::rank_element_blocks(S, P);  // (rank_entry has checked that it fits)
    // a NaN fails the call before anything is written
    {
        if (d_nan.alloc(sizeof(int)) != hipSuccess) return rank_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate device memory");
        ANALYSIS_TRY(g_rank_error, hipMemsetAsync(d_nan.get(), 0, sizeof(int), stream));
        hipLaunchKernelGGL(rank_nan_kernel<T>, dim3(all_blocks), dim3(kThreads), 0, stream, d, d_nan.get());
        ANALYSIS_TRY(g_rank_error, hipGetLastError());
        int nan = 0;
        ANALYSIS_TRY(g_rank_error, hipMemcpyAsync(&nan, d_nan.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(g_rank_error, hipStreamSynchronize(stream));
        if (nan) return rank_fail(MCMCPP_HIP_E_ARG, w + ": the draws contain a NaN (it has no place in the order)");
    }
    const bool folds = q.diagnostics || q.fold != 0;
    if (int rc = rk.prepare(mcmcpp::rank_key_bits(sizeof(T) == 4, folds))) return rc;
    Quantiles quant;
    quant.median.resize(P);
    quant.q05.resize(P);
    quant.q95.resize(P);

    if (!q.diagnostics)
    {
        double* scores = q.so.scores;
        if (!r.on_device)
        {
            if (d_chain.alloc(8 * chain_elems) != hipSuccess) return rank_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * chain_elems) + " bytes of the scores");
            scores = d_chain.get();
        }
        if (q.fold == 0)
        {
            if (int rc = rk.rank_all(false, &quant, scores)) return rc;
        }
        else
        {
            if (int rc = rk.rank_all(false, &quant, nullptr)) return rc;
            if (int rc = rk.set_fold_center(quant)) return rc;
            if (int rc = rk.rank_all(true, nullptr, scores)) return rc;
        }
        ANALYSIS_TRY(g_rank_error, hipStreamSynchronize(stream));
        // the call has succeeded: the outputs
        if (!r.on_device) ANALYSIS_TRY(g_rank_error, hipMemcpy(q.so.scores, scores, 8 * chain_elems, hipMemcpyDeviceToHost));
        if (q.so.median) std::memcpy(q.so.median, quant.median.data(), 8 * (size_t)P);
        if (q.so.q05) std::memcpy(q.so.q05, quant.q05.data(), 8 * (size_t)P);
        if (q.so.q95) std::memcpy(q.so.q95, quant.q95.data(), 8 * (size_t)P);
        if (q.so.sequence_length) *q.so.sequence_length = L;
        if (q.so.num_sequences) *q.so.num_sequences = shape.M;
        return MCMCPP_HIP_OK;
    }

    // the diagnostics: the existing entry points on fp64 chains [K][HL][W][P] built here
    if (d_chain.alloc(8 * chain_elems) != hipSuccess || d_q.alloc(8 * (size_t)P) != hipSuccess)
        return rank_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * chain_elems) + " bytes of the score chain");
    std::vector<double> rhat_rank(P), ess_bulk(P), rhat_folded(P), lower(P), upper(P);
    std::vector<int64_t> closed_bulk(P), closed_lower(P), closed_upper(P);
    int64_t len = 0, count = 0;
    const auto ess_of_chain = [&](double* ess, int64_t* closed, double* rhat) -> int {
        ANALYSIS_TRY(g_rank_error, hipStreamSynchronize(stream));
        const int rc = mcmcpp_hip_effective_sample_size_device(MCMCPP_HIP_F64, device, d_chain.get(), K, 0, HL, 1, r.W, P, r.split, q.max_lag, 0, ess, nullptr, nullptr, closed,
                                                               nullptr, nullptr, rhat, nullptr, nullptr, nullptr, &len, &count);
        return rc ? rank_fail(rc, w + ": " + mcmcpp_hip_effective_sample_size_last_error()) : MCMCPP_HIP_OK;
    };
    if (int rc = rk.rank_all(false, &quant, d_chain.get())) return rc;
    if (int rc = ess_of_chain(ess_bulk.data(), closed_bulk.data(), rhat_rank.data())) return rc;
    if (int rc = rk.set_fold_center(quant)) return rc;
    if (int rc = rk.rank_all(true, nullptr, d_chain.get())) return rc;
    ANALYSIS_TRY(g_rank_error, hipStreamSynchronize(stream));
    if (int rc = mcmcpp_hip_gelman_rubin_device(MCMCPP_HIP_F64, device, d_chain.get(), K, 0, HL, 1, r.W, P, r.split, rhat_folded.data(), nullptr, nullptr, nullptr, nullptr,
                                                nullptr, nullptr, nullptr, nullptr, nullptr))
        return rank_fail(rc, w + ": " + mcmcpp_hip_gelman_rubin_last_error());
    for (int tail = 0; tail < 2; ++tail)
    {
        ANALYSIS_TRY(g_rank_error, hipMemcpyAsync(d_q.get(), (tail ? quant.q95 : quant.q05).data(), 8 * (size_t)P, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(rank_indicator_kernel<T>, dim3(all_blocks), dim3(kThreads), 0, stream, d, (const double*)d_q.get(), d_chain.get());
        ANALYSIS_TRY(g_rank_error, hipGetLastError());
        if (int rc = ess_of_chain((tail ? upper : lower).data(), (tail ? closed_upper : closed_lower).data(), nullptr)) return rc;
    }
    // the call has succeeded: the outputs
    const DiagOutputs& o = q.dg;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int p = 0; p < P; ++p)
    {
        const double a = rhat_rank[p], b = rhat_folded[p], lo = lower[p], up = upper[p];
        if (o.rhat) o.rhat[p] = (a != a || b != b) ? nan : (a > b ? a : b);
        if (o.ess_tail) o.ess_tail[p] = (lo != lo || up != up) ? nan : (lo < up ? lo : up);
        if (o.closed_tail) o.closed_tail[p] = closed_lower[p] && closed_upper[p];
    }
    const auto give = [&](double* out, const std::vector<double>& v) {
        if (out) std::memcpy(out, v.data(), 8 * (size_t)P);
    };
    give(o.rhat_rank, rhat_rank);
    give(o.rhat_folded, rhat_folded);
    give(o.ess_bulk, ess_bulk);
    give(o.ess_tail_lower, lower);
    give(o.ess_tail_upper, upper);
    give(o.median, quant.median);
    give(o.q05, quant.q05);
    give(o.q95, quant.q95);
    if (o.closed_bulk) std::memcpy(o.closed_bulk, closed_bulk.data(), 8 * (size_t)P);
    if (o.sequence_length) *o.sequence_length = L;
    if (o.num_sequences) *o.num_sequences = shape.M;
    return MCMCPP_HIP_OK;
}

int rank_entry(const Request& q)
{
    const std::string w(q.in.what);
    long long n = 0;
    mcmcpp::RhatShape shape;
    if (int rc = mcmcpp::rhat_check_request(g_rank_error, q.in, &n, &shape)) return rc;
    if (q.diagnostics && q.max_lag < 0) return rank_fail(MCMCPP_HIP_E_ARG, w + ": max_lag >= 0 (0: up to L - 1)");
    if ((double)shape.M * (double)shape.L > (double)mcmcpp::kRankMaxDraws)
        return rank_fail(MCMCPP_HIP_E_ARG, w + ": at most 2^31 - 1 draws of a parameter can be ranked (S = M L)");
    if (!mcmcpp::rank_grids_fit(shape.M * shape.L, q.in.P))
        return rank_fail(MCMCPP_HIP_E_ARG, w + ": too many draws in all: S x num_params must not exceed 256 x (2^31 - 1)");
    if (!q.diagnostics && !q.so.scores) return rank_fail(MCMCPP_HIP_E_ARG, w + ": scores must not be NULL");
    hipDeviceProp_t prop;
    std::string why;
    int device = q.in.device;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return rank_fail(rc, w + ": " + why);
    return q.in.dtype == MCMCPP_HIP_F64 ? run_request<double>(q, device, n, shape) : run_request<float>(q, device, n, shape);
}
}  // namespace

extern "C"
{
const char* mcmcpp_hip_rank_diagnostics_last_error(void) { return g_rank_error.c_str(); }

int mcmcpp_hip_normal_scores(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                             int32_t split, int32_t fold, double* scores, double* median, double* q05, double* q95, int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::RhatRequest{"normal_scores", dtype, device, steps, nullptr, false, num_chains, 0, n_steps, 1, num_walkers, num_params, split}, false, fold,
                              0, ScoreOutputs{scores, median, q05, q95, sequence_length, num_sequences}, DiagOutputs{}});
}

int mcmcpp_hip_normal_scores_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains, int64_t chain_stride_steps, int64_t n_steps,
                                    int64_t slice_interval, int32_t num_walkers, int32_t num_params, int32_t split, int32_t fold, double* scores, double* median,
                                    double* q05, double* q95, int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::RhatRequest{"normal_scores_device", dtype, device, nullptr, device_steps, true, num_chains, chain_stride_steps, n_steps, slice_interval,
                                                  num_walkers, num_params, split},
                              false, fold, 0, ScoreOutputs{scores, median, q05, q95, sequence_length, num_sequences}, DiagOutputs{}});
}

int mcmcpp_hip_rank_diagnostics(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                                int32_t split, int64_t max_lag, double* rhat, double* rhat_rank, double* rhat_folded, double* ess_bulk, double* ess_tail,
                                double* ess_tail_lower, double* ess_tail_upper, double* median, double* q05, double* q95, int64_t* closed_bulk, int64_t* closed_tail,
                                int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::RhatRequest{"rank_diagnostics", dtype, device, steps, nullptr, false, num_chains, 0, n_steps, 1, num_walkers, num_params, split}, true, 0,
                              max_lag, ScoreOutputs{},
                              DiagOutputs{rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper, median, q05, q95, closed_bulk, closed_tail,
                                          sequence_length, num_sequences}});
}

int mcmcpp_hip_rank_diagnostics_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains, int64_t chain_stride_steps, int64_t n_steps,
                                       int64_t slice_interval, int32_t num_walkers, int32_t num_params, int32_t split, int64_t max_lag, double* rhat, double* rhat_rank,
                                       double* rhat_folded, double* ess_bulk, double* ess_tail, double* ess_tail_lower, double* ess_tail_upper, double* median,
                                       double* q05, double* q95, int64_t* closed_bulk, int64_t* closed_tail, int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::RhatRequest{"rank_diagnostics_device", dtype, device, nullptr, device_steps, true, num_chains, chain_stride_steps, n_steps,
                                                  slice_interval, num_walkers, num_params, split},
                              true, 0, max_lag, ScoreOutputs{},
                              DiagOutputs{rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper, median, q05, q95, closed_bulk, closed_tail,
                                          sequence_length, num_sequences}});
}
}
