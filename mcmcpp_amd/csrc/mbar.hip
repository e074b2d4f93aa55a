// mbar.hip -- the multistate Bennett acceptance ratio (MBAR: Shirts & Chodera 2008; Tan 2004; Geyer's reverse logistic
// regression) over the rungs of a tempering ladder, from the stored steps of its K chains: one joint solve for all K
// log-normalising constants from every draw of every rung evaluated under every rung's parameters, with their K x K covariance.
// An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_evidence_mbar); mbar_plan.hpp numbers the sums, shapes the
// trees and the buffers, and has the Cholesky solve, the solver, which asks for one pass at a time, and the covariance.
//   * mbar_store_kernel: the calculator's log-posteriors of a chunk of one rung's draws under all K parameter sets (K calculator
//     launches, as mcmcpp_hip_calc_logp_device makes them) widened into l[k], with the counts of non-finite values and of NaN or
//     +inf among them: first in LDS, then one integer atomic each per block.
//   * mbar_pass_kernel: block = a tile of kBridgeTile terms of one tree (grid.z: the joint tree, or a rung's) for one group k
//     (grid.y): lane t takes terms 2t, 2t+1, 2t+512, 2t+513, reads them from the K streams (each coalesced), forms the maximum,
//     the denominator and w_k, then w_l anew for l = k .. K - 1: K + (K - k) evidence_exp a term, and no array a lane indexes at
//     run time.  The group's sums (S_k, then row k of P) go kMbarBatch at a time through LDS in the shape of sum_tree.  Behind the
//     final pass the launch over the rungs' trees also keeps w_r of rung r's own draws: the chain of the effective sample size.
//   * mbar_slice_kernel, mbar_total_kernel: a thread adds the tile sums of a slice of one sum in ascending order, then a thread
//     per sum adds its slice sums in ascending order.  The host reads back Q doubles a pass ((K + 1) Q behind the final one).
// No atomics on doubles, and nothing depends on the CU count, the chunk size or where a chain lies.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "evidence_plan.hpp"
#include "mbar_plan.hpp"
#include "rhat_state.hpp"

namespace
{
using mcmcpp::kBridgeThreads;
using mcmcpp::kBridgeTile;
using mcmcpp::kEvidenceThreads;
using mcmcpp::kMbarBatch;
using mcmcpp::kMbarMaxChains;

// per (rung, chain): the non-finite log-posteriors, the NaN or +inf among them
struct MbarCount
{
    unsigned long long nonfinite, bad;
};
struct MbarZeta
{
    double z[kMbarMaxChains];
};

// lp [K][chunk_draws] of the handle's dtype -> l[k][at + i], i < count: grid (blocks, K)
template <class T>
__global__ void __launch_bounds__(kEvidenceThreads)
mbar_store_kernel(const T* __restrict__ lp, long long chunk_draws, long long count, double* __restrict__ l, long long kn, long long at, MbarCount* __restrict__ counts)
{
    __shared__ unsigned long long s_nonfinite, s_bad;
    const int k = (int)blockIdx.y;
    const long long i = (long long)blockIdx.x * kEvidenceThreads + threadIdx.x;
    if (threadIdx.x == 0) s_nonfinite = 0, s_bad = 0;
    __syncthreads();
    if (i < count)
    {
        const double v = (double)lp[(size_t)k * (size_t)chunk_draws + (size_t)i];
        l[(size_t)k * (size_t)kn + (size_t)(at + i)] = v;
        const bool nan = v != v, pinf = v == __builtin_inf(), ninf = v == -__builtin_inf();
        if (nan || pinf || ninf) atomicAdd(&s_nonfinite, 1ULL);
        if (nan || pinf) atomicAdd(&s_bad, 1ULL);
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        if (s_nonfinite) atomicAdd(&counts[k].nonfinite, s_nonfinite);
        if (s_bad) atomicAdd(&counts[k].bad, s_bad);
    }
}

// One tree per blockIdx.z: `count` terms that begin at term blockIdx.z * set_stride of l[k] (kn doubles each)
template <bool SERIES>
__global__ void __launch_bounds__(kBridgeThreads)
mbar_pass_kernel(const double* __restrict__ l, int K, long long kn, long long set_stride, long long count, long long tiles, MbarZeta zeta, double* __restrict__ tile_sums,
                 double* __restrict__ series)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double s_p[kMbarBatch][kBridgeThreads];
    const int t = (int)threadIdx.x, k = (int)blockIdx.y, set = (int)blockIdx.z;
    const int Q = K + K * (K + 1) / 2;
    const long long first = (long long)set * set_stride, base = (long long)blockIdx.x * kBridgeTile;
    long long at[4];
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const long long i = base + 512 * (j >> 1) + 2 * t + (j & 1);
        live[j] = i < count;
        at[j] = first + (live[j] ? i : 0);  // (a missing term reads the tree's first: a place that exists)
    }
    double m[4], dn[4], ek[4], wk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = l[at[j]] - zeta.z[0];
    for (int c = 1; c < K; ++c)
    {
        const double* __restrict__ lc = l + (size_t)c * (size_t)kn;
        const double z = zeta.z[c];
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            const double a = lc[at[j]] - z;
            if (a > m[j]) m[j] = a;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) dn[j] = 0.0, ek[j] = 0.0;
    for (int c = 0; c < K; ++c)
    {
        const double* __restrict__ lc = l + (size_t)c * (size_t)kn;
        const double z = zeta.z[c];
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            const double e = mcmcpp::evidence_exp((lc[at[j]] - z) - m[j]);
            dn[j] = dn[j] + e;
            if (c == k) ek[j] = e;
        }
    }
    bool none[4];  // a missing term, or a draw whose K entries are all -inf: every w is +0
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        none[j] = !live[j] || m[j] == -__builtin_inf();
        wk[j] = none[j] ? 0.0 : ek[j] / dn[j];
    }
    if (SERIES)
        if (k == set)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live[j]) series[at[j]] = wk[j];

    // the group's sums: number 0 is S_k, number 1 + (c - k) is P_kc
    const int nq = 1 + K - k;
    for (int q0 = 0; q0 < nq; q0 += kMbarBatch)
    {
#pragma unroll
        for (int b = 0; b < kMbarBatch; ++b)
        {
            const int qi = q0 + b;
            double p = 0.0;
            if (qi == 0)
                p = ((wk[0] + wk[1]) + wk[2]) + wk[3];
            else if (qi < nq)
            {
                const int c = k + qi - 1;
                const double* __restrict__ lc = l + (size_t)c * (size_t)kn;
                const double z = zeta.z[c];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                {
                    const double e = mcmcpp::evidence_exp((lc[at[j]] - z) - m[j]);
                    const double v = wk[j] * (none[j] ? 0.0 : e / dn[j]);
                    p = j == 0 ? v : p + v;
                }
            }
            s_p[b][t] = p;
        }
        __syncthreads();
        for (int s = kBridgeThreads / 2; s >= 1; s >>= 1)
        {
            if (t < s)
#pragma unroll
                for (int b = 0; b < kMbarBatch; ++b) s_p[b][t] = s_p[b][t] + s_p[b][t + s];
            __syncthreads();
        }
        if (t < kMbarBatch && q0 + t < nq)
        {
            const int qi = q0 + t, q = qi == 0 ? k : mcmcpp::mbar_index_p(K, k, k + qi - 1);
            tile_sums[((size_t)set * (size_t)Q + (size_t)q) * (size_t)tiles + blockIdx.x] = s_p[t][0];
        }
        __syncthreads();  // (the next batch writes s_p)
    }
}

// tile sums [rows][tiles] -> slice sums [rows][slices]: one thread per (row, slice)
__global__ void __launch_bounds__(kBridgeThreads)
mbar_slice_kernel(const double* __restrict__ tile_sums, long long tiles, int slices, long long rows, double* __restrict__ slice_sums)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const long long item = (long long)blockIdx.x * kBridgeThreads + threadIdx.x;
    if (item >= rows * slices) return;
    const long long row = item / slices;
    const int sl = (int)(item % slices);
    long long first, count;
    mcmcpp::bridge_slice_span(tiles, sl, &first, &count);
    const double* __restrict__ v = tile_sums + (size_t)row * (size_t)tiles + first;
    double acc = 0.0;
    for (long long j = 0; j < count; ++j) acc = acc + v[j];
    slice_sums[(size_t)row * (size_t)slices + sl] = acc;
}
// slice sums [rows][slices] -> out [rows]: one thread per row
__global__ void __launch_bounds__(kBridgeThreads)
mbar_total_kernel(const double* __restrict__ slice_sums, int slices, long long rows, double* __restrict__ out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const long long row = (long long)blockIdx.x * kBridgeThreads + threadIdx.x;
    if (row >= rows) return;
    const double* __restrict__ v = slice_sums + (size_t)row * (size_t)slices;
    double acc = 0.0;
    for (int sl = 0; sl < slices; ++sl) acc = acc + v[sl];
    out[row] = acc;
}

template <class T>
int run_request(mcmcpp_hip_sampler& h, const mcmcpp::MbarRequest& b, long long n)
{
    const mcmcpp::EvidenceRequest& q = b.q;
    std::string& slot = h.error;
    const std::string w(q.what);
    const auto fail = [&](int code, const std::string& msg) { return mcmcpp::analysis_fail(slot, code, msg); };
    const int K = q.K, W = q.W, D = q.D;
    const long long E = (long long)W * D, N = n * W, KN = (long long)K * N;
    const size_t step_bytes = sizeof(T) * (size_t)E;
    const long long chain_stride_steps = q.chain_stride_steps ? q.chain_stride_steps : q.n_steps;
    const double nan = std::numeric_limits<double>::quiet_NaN();

    ANALYSIS_TRY(slot, hipSetDevice(q.device));
    hipDeviceProp_t prop;
    ANALYSIS_TRY(slot, hipGetDeviceProperties(&prop, q.device));
    if (q.on_device)
        if (int rc = mcmcpp::check_device_steps(slot, q.what, q.device_steps, step_bytes * (size_t)((K - 1) * chain_stride_steps + q.n_steps), q.device)) return rc;

    const long long per = mcmcpp::evidence_steps_per_chunk(mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_EVIDENCE_CHUNK_MB", 1024), step_bytes, q.on_device, q.slice);
    const long long chunk_steps = n < per ? n : per, chunk_draws = chunk_steps * W;
    if (!mcmcpp::evidence_grid_fits(chunk_draws)) return fail(MCMCPP_HIP_E_ARG, w + ": too many draws in a chunk for a launch grid (lower MCMCPP_HIP_EVIDENCE_CHUNK_MB)");
    if (!mcmcpp::mbar_grid_fits(K, N)) return fail(MCMCPP_HIP_E_ARG, w + ": too many draws for a launch grid");
    const mcmcpp::MbarPlan plan = mcmcpp::mbar_plan(K, N);
    const int Q = plan.Q;

    mcmcpp::DeviceBuffer<> d_chunk;
    mcmcpp::DeviceBuffer<T> d_lp;
    mcmcpp::DeviceBuffer<double> d_l, d_series, d_tiles, d_slices, d_totals;
    mcmcpp::DeviceBuffer<MbarCount> d_counts;
    mcmcpp::Stream stream;  // (behind the buffers: the stream is idle and gone when they go)
    ANALYSIS_TRY(slot, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    if (!q.on_device && d_chunk.alloc(step_bytes * (size_t)chunk_steps) != hipSuccess) return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the upload buffer");
    if (d_lp.alloc(sizeof(T) * (size_t)K * (size_t)chunk_draws) != hipSuccess || d_counts.alloc(sizeof(MbarCount) * (size_t)K * (size_t)K) != hipSuccess)
        return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the log-posteriors of a chunk");
    if (d_l.alloc(8 * plan.l_doubles) != hipSuccess)
        return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * plan.l_doubles) + " bytes of the log-posteriors of every draw under every chain");
    if (d_series.alloc(8 * plan.series_doubles) != hipSuccess || d_tiles.alloc(8 * plan.tile_sum_doubles) != hipSuccess || d_slices.alloc(8 * plan.slice_sum_doubles) != hipSuccess ||
        d_totals.alloc(8 * plan.total_doubles) != hipSuccess)
        return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the sums of a pass");

    // l: the draws of rung r under every chain's parameters
    ANALYSIS_TRY(slot, hipMemsetAsync(d_counts.get(), 0, sizeof(MbarCount) * (size_t)K * (size_t)K, stream));
    std::vector<const void*> used(q.on_device ? 0 : (size_t)n);  // host steps: the used ones of a rung
    for (int r = 0; r < K; ++r)
    {
        if (!q.on_device)
            for (long long s = 0; s < n; ++s) used[(size_t)s] = q.steps[(size_t)r * (size_t)q.n_steps + (size_t)(s * q.slice)];
        mcmcpp::StepSource<T> src{q.on_device ? nullptr : used.data(),
                                  q.on_device ? static_cast<const T*>(q.device_steps) + (size_t)(r * chain_stride_steps) * (size_t)E : nullptr,
                                  n, q.slice, W, D, stream, &d_chunk, &slot};
        long long done = 0;  // used steps of the rung behind the chunks so far
        const int rc = src.for_each_chunk(per, [&](mcmcpp::StepSpan<T> span) -> int {
            // the upload has arrived, and the store kernel of the chunk before has read the log-posteriors the calculator overwrites
            ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
            const long long count = span.n_steps * W;  // (rows that follow each other: per == 1 where the steps do not)
            for (int k = 0; k < K; ++k)
                if (int crc = h.calc_logp_device(k, span.base, count, d_lp.get() + (size_t)k * (size_t)chunk_draws)) return mcmcpp::nested_result(slot, q.what, crc);
            hipLaunchKernelGGL(mbar_store_kernel<T>, dim3((unsigned)mcmcpp::evidence_diff_blocks(count), (unsigned)K), dim3(kEvidenceThreads), 0, stream, (const T*)d_lp.get(),
                               chunk_draws, count, d_l.get(), KN, (long long)r * N + done * W, d_counts.get() + (size_t)r * (size_t)K);
            ANALYSIS_TRY(slot, hipGetLastError());
            done += span.n_steps;
            return MCMCPP_HIP_OK;
        });
        if (rc) return rc;
    }
    std::vector<MbarCount> counts((size_t)K * (size_t)K);
    ANALYSIS_TRY(slot, hipMemcpyAsync(counts.data(), d_counts.get(), sizeof(MbarCount) * counts.size(), hipMemcpyDeviceToHost, stream));
    ANALYSIS_TRY(slot, hipStreamSynchronize(stream));

    std::vector<double> log_z((size_t)K, nan), cov((size_t)K * (size_t)K, nan), log_ratio((size_t)(K - 1), nan), mcse((size_t)(K - 1), nan), ess((size_t)K, nan);
    std::vector<int64_t> nonfinite((size_t)K * (size_t)K, 0);
    double log_ratio_total = nan, mcse_total = nan;
    int64_t passes = 0, converged = 0;
    bool bad = false;  // a NaN or +inf anywhere: every figure stays NaN
    for (size_t i = 0; i < counts.size(); ++i) nonfinite[i] = (int64_t)counts[i].nonfinite, bad = bad || counts[i].bad != 0;

    if (!bad)
    {
        const dim3 block(kBridgeThreads);
        // the sums of `sets` trees of `tree`'s shape into totals[at ..): the pass kernel, then the two that close it
        const auto sums = [&](const mcmcpp::MbarTree& tree, int sets, long long set_stride, const MbarZeta& zeta, bool series, size_t at) -> int {
            const dim3 grid((unsigned)tree.tiles, (unsigned)K, (unsigned)sets);
            if (series)
                hipLaunchKernelGGL(mbar_pass_kernel<true>, grid, block, 0, stream, (const double*)d_l.get(), K, KN, set_stride, tree.terms, tree.tiles, zeta, d_tiles.get(), d_series.get());
            else
                hipLaunchKernelGGL(mbar_pass_kernel<false>, grid, block, 0, stream, (const double*)d_l.get(), K, KN, set_stride, tree.terms, tree.tiles, zeta, d_tiles.get(),
                                   (double*)nullptr);
            const long long rows = (long long)sets * Q;
            hipLaunchKernelGGL(mbar_slice_kernel, dim3(mcmcpp::mbar_close_blocks(rows * tree.slices)), block, 0, stream, (const double*)d_tiles.get(), tree.tiles, tree.slices, rows,
                               d_slices.get());
            hipLaunchKernelGGL(mbar_total_kernel, dim3(mcmcpp::mbar_close_blocks(rows)), block, 0, stream, (const double*)d_slices.get(), tree.slices, rows, d_totals.get() + at);
            ANALYSIS_TRY(slot, hipGetLastError());
            return MCMCPP_HIP_OK;
        };
        const auto eval = [&](const double* at, bool final, mcmcpp::MbarSums* s) -> int {
            MbarZeta zeta{};
            for (int k = 0; k < K; ++k) zeta.z[k] = at[k];
            s->joint.assign((size_t)Q, 0.0);
            if (int rc = sums(plan.joint, 1, 0, zeta, false, 0)) return rc;
            ANALYSIS_TRY(slot, hipMemcpyAsync(s->joint.data(), d_totals.get(), 8 * (size_t)Q, hipMemcpyDeviceToHost, stream));
            if (final)
            {
                s->rung.assign((size_t)K * (size_t)Q, 0.0);
                if (int rc = sums(plan.rung, K, N, zeta, true, (size_t)Q)) return rc;
                ANALYSIS_TRY(slot, hipMemcpyAsync(s->rung.data(), d_totals.get() + Q, 8 * (size_t)K * (size_t)Q, hipMemcpyDeviceToHost, stream));
            }
            ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
            return MCMCPP_HIP_OK;
        };
        mcmcpp::MbarRoot root;
        if (int rc = mcmcpp::mbar_solve(K, N, eval, &root)) return rc;
        passes = root.passes, converged = root.converged;
        if (!root.failed)
        {
            // w_r of rung r's own draws as the ESS call sees it: a chain of one rung, n steps of W walkers of one parameter, split
            const mcmcpp::RhatRequest ess_request = mcmcpp::rhat_device_request("effective_sample_size_device", MCMCPP_HIP_F64, q.device, nullptr, 1, 0, n, 1, W, 1, 1);
            const mcmcpp::RhatShape ess_shape = mcmcpp::rhat_shape(1, n, W, 1);
            for (int r = 0; r < K; ++r)
            {
                mcmcpp::RhatRequest chain = ess_request;
                chain.device_steps = d_series.get() + (size_t)r * (size_t)N;
                mcmcpp::EssOutputs eo{};
                eo.ess = &ess[(size_t)r];
                if (int erc = mcmcpp::nested_result(slot, q.what, mcmcpp::ess_compute(slot, chain, 0, 0, prop, n, ess_shape, stream, eo))) return erc;
            }
            log_z = root.zeta;
            mcmcpp::mbar_covariance(K, N, root.L.data(), root.at.rung.data(), ess.data(), cov.data());
            mcmcpp::mbar_figures(K, log_z.data(), cov.data(), log_ratio.data(), mcse.data(), &log_ratio_total, &mcse_total);
        }
    }

    // the call has succeeded: the outputs
    const mcmcpp::MbarOutputs& o = b.out;
    const auto give = [&](double* out, const std::vector<double>& v) {
        if (out) std::memcpy(out, v.data(), 8 * v.size());
    };
    give(o.log_z, log_z);
    give(o.cov, cov);
    give(o.log_ratio, log_ratio);
    give(o.mcse, mcse);
    give(o.ess, ess);
    if (o.nonfinite) std::memcpy(o.nonfinite, nonfinite.data(), 8 * nonfinite.size());
    if (o.log_ratio_total) *o.log_ratio_total = log_ratio_total;
    if (o.mcse_total) *o.mcse_total = mcse_total;
    if (o.passes) *o.passes = passes;
    if (o.converged) *o.converged = converged;
    if (o.num_draws) *o.num_draws = N;
    return MCMCPP_HIP_OK;
}
}  // namespace

namespace mcmcpp
{
int mbar_compute(mcmcpp_hip_sampler& h, const MbarRequest& m)
{
    long long n = 0;  // every check that needs no device: those of the ratios
    if (int rc = evidence_check(h, m.q, &n)) return rc;
    return m.q.dtype == MCMCPP_HIP_F64 ? run_request<double>(h, m, n) : run_request<float>(h, m, n);
}
}  // namespace mcmcpp
