// bridge.hip -- the bridge estimate (Bennett's acceptance ratio; Meng & Wong 1996) of the ratios of normalising constants
// between the rungs of a tempering ladder, from the stored steps of its K chains: one estimate per pair of neighbours from the
// draws of both rungs, the root c* of g(c) = S_0(c) - S_1(c).  An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_evidence_bridge).  The differences u are those of
// mcmcpp_hip_evidence_ratios, made the same way (evidence_plan.hpp: at most three calculator launches per chunk of a rung;
// evidence_kernels.hpp: evidence_diff_kernel), but kept raw: bridge_plan.hpp says which of three buffers holds which u, and has
// the solver, which asks for one pass at a time.
//   * bridge_pass_kernel: block = a tile of kBridgeTile draws of one direction (grid.y): lane t loads terms 2t, 2t+1 and 2t+512,
//     2t+513 with two 16-byte loads, forms h = sigma(u -+ c), h (1 - h) and, on the final pass, h h, adds its four terms left to
//     right and reduces the 256 partial sums through LDS in the shape of sum_tree; thread q writes the tile's sum of quantity q.
//     The final pass writes h over u: the chain the effective sample size is computed on.
//   * bridge_close_kernel: one block: a thread adds the tile sums of a slice of one quantity in ascending order, then one thread
//     per quantity adds its slice sums in ascending order.  The host reads back four doubles (six behind the final pass).
// One pair, from its two u arrays to its figures (the solve, the final sums, the two ESS calls, the edges), is
// bridge_pair_compute (bridge_pair.hpp): this file calls it per pair of rungs, gaussian_bridge.hip on (target, fitted Gaussian).
// No atomics on doubles, and nothing depends on the CU count, the chunk size or where a chain lies.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bridge_pair.hpp"
#include "bridge_plan.hpp"
#include "evidence_kernels.hpp"
#include "evidence_plan.hpp"
#include "rhat_state.hpp"

namespace
{
using mcmcpp::evidence_diff_kernel;
using mcmcpp::EvidenceState;
using mcmcpp::kBridgeThreads;
using mcmcpp::kBridgeTile;
using mcmcpp::kEvidenceThreads;

template <bool FINAL>
__global__ void __launch_bounds__(kBridgeThreads)
bridge_pass_kernel(double* __restrict__ u0, double* __restrict__ u1, long long N, long long tiles, double c, double* __restrict__ tile_sums)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    constexpr int kQ = FINAL ? 3 : 2;
    __shared__ double s_p[kQ][kBridgeThreads];
    const int d = (int)blockIdx.y, t = (int)threadIdx.x;
    double* __restrict__ u = d ? u1 : u0;
    const long long base = (long long)blockIdx.x * kBridgeTile;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int half = 0; half < 2; ++half)
    {
        const long long i = base + 512 * half + 2 * t;  // (even, and u is a whole allocation: a 16-byte boundary)
        if (i + 1 < N)
        {
            const double2 v = *reinterpret_cast<const double2*>(u + i);
            x[2 * half] = v.x, x[2 * half + 1] = v.y;
        }
        else if (i < N)
            x[2 * half] = u[i];
    }
    double p[kQ];
    for (int q = 0; q < kQ; ++q) p[q] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
        const long long i = base + 512 * (j >> 1) + 2 * t + (j & 1);
        const double h = i < N ? mcmcpp::bridge_sigma(d ? x[j] + c : x[j] - c) : 0.0;  // a missing term is +0
        x[j] = h;
        const double v[3] = {h, h * (1.0 - h), h * h};
        for (int q = 0; q < kQ; ++q) p[q] = j == 0 ? v[q] : p[q] + v[q];
    }
    if (FINAL)
#pragma unroll
        for (int half = 0; half < 2; ++half)
        {
            const long long i = base + 512 * half + 2 * t;
            if (i + 1 < N)
                *reinterpret_cast<double2*>(u + i) = make_double2(x[2 * half], x[2 * half + 1]);
            else if (i < N)
                u[i] = x[2 * half];
        }
    for (int q = 0; q < kQ; ++q) s_p[q][t] = p[q];
    __syncthreads();
    for (int s = kBridgeThreads / 2; s >= 1; s >>= 1)
    {
        if (t < s)
            for (int q = 0; q < kQ; ++q) s_p[q][t] = s_p[q][t] + s_p[q][t + s];
        __syncthreads();
    }
    if (t < kQ) tile_sums[(size_t)(d * 3 + t) * (size_t)tiles + blockIdx.x] = s_p[t][0];
}

// tile sums [2][3][tiles] -> slice sums [2][3][slices] -> out [3][2]: S_0, S_1, Q_0, Q_1 and, where nq == 3, H_0, H_1
__global__ void __launch_bounds__(kBridgeThreads)
bridge_close_kernel(const double* __restrict__ tile_sums, long long tiles, int slices, int nq, double* __restrict__ slice_sums, double* __restrict__ out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const long long items = 2LL * nq * slices;
    for (long long item = threadIdx.x; item < items; item += kBridgeThreads)
    {
        const int sl = (int)(item % slices), dq = (int)(item / slices), d = dq / nq, q = dq % nq;
        long long first, count;
        mcmcpp::bridge_slice_span(tiles, sl, &first, &count);
        const double* __restrict__ v = tile_sums + (size_t)(d * 3 + q) * (size_t)tiles + first;
        double acc = 0.0;
        for (long long j = 0; j < count; ++j) acc = acc + v[j];
        slice_sums[(size_t)(d * 3 + q) * (size_t)slices + sl] = acc;
    }
    __syncthreads();  // (one block: the slice sums are its own writes)
    if ((int)threadIdx.x < 2 * nq)
    {
        const int d = (int)threadIdx.x / nq, q = (int)threadIdx.x % nq;
        const double* __restrict__ v = slice_sums + (size_t)(d * 3 + q) * (size_t)slices;
        double acc = 0.0;
        for (int sl = 0; sl < slices; ++sl) acc = acc + v[sl];
        out[2 * q + d] = acc;
    }
}

template <class T>
int run_request(mcmcpp_hip_sampler& h, const mcmcpp::BridgeRequest& b, long long n)
{
    const mcmcpp::EvidenceRequest& q = b.q;
    std::string& slot = h.error;
    const std::string w(q.what);
    const auto fail = [&](int code, const std::string& msg) { return mcmcpp::analysis_fail(slot, code, msg); };
    const int K = q.K, W = q.W, D = q.D, pairs = mcmcpp::evidence_pairs(K);
    const long long E = (long long)W * D, N = n * W;
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
    if (!mcmcpp::bridge_grid_fits(N)) return fail(MCMCPP_HIP_E_ARG, w + ": too many draws of a rung for a launch grid");

    mcmcpp::DeviceBuffer<> d_chunk;
    mcmcpp::DeviceBuffer<T> d_lp;
    mcmcpp::DeviceBuffer<double> d_u[3];
    mcmcpp::BridgePairScratch scratch;
    mcmcpp::DeviceBuffer<EvidenceState> d_state;
    mcmcpp::Stream stream;  // (behind the buffers: the stream is idle and gone when they go)
    ANALYSIS_TRY(slot, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    if (!q.on_device && d_chunk.alloc(step_bytes * (size_t)chunk_steps) != hipSuccess) return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the upload buffer");
    if (d_lp.alloc(sizeof(T) * 3 * (size_t)chunk_draws) != hipSuccess || scratch.alloc(N) != hipSuccess || d_state.alloc(2 * sizeof(EvidenceState)) != hipSuccess)
        return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the log-posteriors of a chunk");
    for (int j = 0; j < mcmcpp::bridge_buffers(K); ++j)
        if (d_u[j].alloc(8 * (size_t)N) != hipSuccess)
            return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * (size_t)N) + " bytes of the differences of a pair and direction");

    std::vector<double> log_ratio((size_t)pairs, nan), mcse((size_t)pairs, nan), overlap((size_t)pairs, nan), ess(2 * (size_t)pairs, nan);
    std::vector<int64_t> passes((size_t)pairs, 0), converged((size_t)pairs, 0), nonfinite(2 * (size_t)pairs, 0);
    std::vector<unsigned long long> bad(2 * (size_t)pairs, 0);
    std::vector<const void*> used(q.on_device ? 0 : (size_t)n);  // host steps: the used ones of a rung

    for (int k = 0; k < K; ++k)
    {
        const mcmcpp::EvidenceRung rung = mcmcpp::evidence_rung(K, k);
        ANALYSIS_TRY(slot, hipMemsetAsync(d_state.get(), 0, 2 * sizeof(EvidenceState), stream));
        if (!q.on_device)
            for (long long s = 0; s < n; ++s) used[(size_t)s] = q.steps[(size_t)k * (size_t)q.n_steps + (size_t)(s * q.slice)];
        mcmcpp::StepSource<T> src{q.on_device ? nullptr : used.data(),
                                  q.on_device ? static_cast<const T*>(q.device_steps) + (size_t)(k * chain_stride_steps) * (size_t)E : nullptr,
                                  n, q.slice, W, D, stream, &d_chunk, &slot};
        long long done = 0;  // used steps of the rung behind the chunks so far
        const int rc = src.for_each_chunk(per, [&](mcmcpp::StepSpan<T> span) -> int {
            // the upload has arrived, and the kernels of the chunk before have read the log-posteriors the calculator overwrites
            ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
            const long long count = span.n_steps * W;  // (rows that follow each other: per == 1 where the steps do not)
            for (int j = 0; j < rung.n_evals; ++j)
                if (int crc = h.calc_logp_device(rung.evals[j], span.base, count, d_lp.get() + (size_t)j * chunk_draws)) return mcmcpp::nested_result(slot, q.what, crc);
            for (int j = 0; j < rung.n_uses; ++j)
                hipLaunchKernelGGL(evidence_diff_kernel<T>, dim3((unsigned)mcmcpp::evidence_diff_blocks(count)), dim3(kEvidenceThreads), 0, stream,
                                   (const T*)(d_lp.get() + (size_t)(1 + j) * chunk_draws), (const T*)d_lp.get(), count,
                                   d_u[mcmcpp::bridge_buffer_of(rung.use_d[j], rung.use_p[j])].get() + (size_t)(done * W), d_state.get() + j);
            ANALYSIS_TRY(slot, hipGetLastError());
            done += span.n_steps;
            return MCMCPP_HIP_OK;
        });
        if (rc) return rc;
        EvidenceState st[2];
        ANALYSIS_TRY(slot, hipMemcpyAsync(st, d_state.get(), sizeof st, hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
        for (int j = 0; j < rung.n_uses; ++j)
        {
            const size_t at = (size_t)mcmcpp::evidence_index(K, rung.use_d[j], rung.use_p[j]);
            nonfinite[at] = (int64_t)st[j].nonfinite;
            bad[at] = st[j].bad;
        }
        if (k == 0) continue;

        // pair p = k - 1 is complete
        const int p = k - 1;
        const size_t at0 = (size_t)mcmcpp::evidence_index(K, 0, p), at1 = (size_t)mcmcpp::evidence_index(K, 1, p);
        if (bad[at0] || bad[at1]) continue;  // a NaN or +inf u: the figures of this pair stay NaN
        double* const u[2] = {d_u[mcmcpp::bridge_buffer_of(0, p)].get(), d_u[mcmcpp::bridge_buffer_of(1, p)].get()};
        mcmcpp::BridgePairFigures f;
        if (int prc = mcmcpp::bridge_pair_compute(slot, q.what, q.device, prop, stream, scratch, u, n, W, &f)) return prc;
        log_ratio[(size_t)p] = f.log_ratio, mcse[(size_t)p] = f.mcse, overlap[(size_t)p] = f.overlap;
        ess[at0] = f.ess[0], ess[at1] = f.ess[1];
        passes[(size_t)p] = f.passes, converged[(size_t)p] = f.converged;
    }

    // the call has succeeded: the outputs
    const mcmcpp::BridgeOutputs& o = b.out;
    const auto give = [&](double* out, const std::vector<double>& v) {
        if (out) std::memcpy(out, v.data(), 8 * v.size());
    };
    const auto give_counts = [&](int64_t* out, const std::vector<int64_t>& v) {
        if (out) std::memcpy(out, v.data(), 8 * v.size());
    };
    give(o.log_ratio, log_ratio);
    give(o.mcse, mcse);
    give(o.overlap, overlap);
    give(o.ess, ess);
    give_counts(o.passes, passes);
    give_counts(o.converged, converged);
    give_counts(o.nonfinite, nonfinite);
    double total = 0.0, squares = 0.0;
    for (int p = 0; p < pairs; ++p)
    {
        total = total + log_ratio[(size_t)p];
        squares = squares + mcse[(size_t)p] * mcse[(size_t)p];
    }
    if (o.log_ratio_total) *o.log_ratio_total = total;
    if (o.mcse_total) *o.mcse_total = std::sqrt(squares);
    if (o.num_draws) *o.num_draws = N;
    return MCMCPP_HIP_OK;
}
}  // namespace

namespace mcmcpp
{
int bridge_pair_compute(std::string& slot, const char* what, int device, const hipDeviceProp_t& prop, hipStream_t stream, const BridgePairScratch& scratch,
                        double* const u[2], long long n, int W, BridgePairFigures* out)
{
    const BridgePlan& plan = scratch.plan;
    const long long N = n * W;
    // h_d(c*) as the ESS call sees it: a chain of one rung, n steps of W walkers of one parameter, split
    const RhatRequest ess_request = rhat_device_request("effective_sample_size_device", MCMCPP_HIP_F64, device, nullptr, 1, 0, n, 1, W, 1, 1);
    const RhatShape ess_shape = rhat_shape(1, n, W, 1);
    const auto eval = [&](double c, bool final, BridgeSums* s) -> int {
        const dim3 grid(plan.grid_x, plan.grid_y), block(kBridgeThreads);
        if (final)
            hipLaunchKernelGGL(bridge_pass_kernel<true>, grid, block, 0, stream, u[0], u[1], N, plan.tiles, c, scratch.tiles.get());
        else
            hipLaunchKernelGGL(bridge_pass_kernel<false>, grid, block, 0, stream, u[0], u[1], N, plan.tiles, c, scratch.tiles.get());
        hipLaunchKernelGGL(bridge_close_kernel, dim3(1), block, 0, stream, (const double*)scratch.tiles.get(), plan.tiles, plan.slices, final ? 3 : 2, scratch.slices.get(),
                           scratch.out.get());
        ANALYSIS_TRY(slot, hipGetLastError());
        double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        ANALYSIS_TRY(slot, hipMemcpyAsync(r, scratch.out.get(), 8 * (final ? 6 : 4), hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
        for (int d = 0; d < 2; ++d) s->S[d] = r[d], s->Q[d] = r[2 + d], s->H[d] = r[4 + d];
        return MCMCPP_HIP_OK;
    };
    BridgePairFigures f;
    BridgeRoot root;
    if (int rc = bridge_solve(eval, &root)) return rc;
    f.passes = root.passes;
    f.converged = root.converged;
    if (root.at.S[0] == 0.0 || root.at.S[1] == 0.0)  // no mass is shared at double precision
    {
        f.overlap = 0.0;
        *out = f;
        return MCMCPP_HIP_OK;
    }
    const double Nd = (double)N;
    double sum = 0.0;
    for (int d = 0; d < 2; ++d)
    {
        const double mean = root.at.S[d] / Nd, var = root.at.H[d] / Nd - mean * mean;
        const double rel2 = (var > 0.0 ? var : 0.0) / (mean * mean);
        RhatRequest chain = ess_request;
        chain.device_steps = u[d];
        EssOutputs eo{};
        double ess_value = std::numeric_limits<double>::quiet_NaN();
        eo.ess = &ess_value;
        if (int erc = nested_result(slot, what, ess_compute(slot, chain, 0, 0, prop, n, ess_shape, stream, eo))) return erc;
        f.ess[d] = ess_value;
        sum = sum + (rel2 == 0.0 ? 0.0 : rel2 / ess_value);
    }
    f.log_ratio = root.c;
    f.overlap = (root.at.S[0] + root.at.S[1]) / Nd;
    f.mcse = std::sqrt(sum);
    *out = f;
    return MCMCPP_HIP_OK;
}

int bridge_compute(mcmcpp_hip_sampler& h, const BridgeRequest& b)
{
    long long n = 0;  // every check that needs no device: those of the ratios
    if (int rc = evidence_check(h, b.q, &n)) return rc;
    return b.q.dtype == MCMCPP_HIP_F64 ? run_request<double>(h, b, n) : run_request<float>(h, b, n);
}
}  // namespace mcmcpp
