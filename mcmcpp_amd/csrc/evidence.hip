// evidence.hip -- the ratios of normalising constants between the rungs of a tempering ladder, from the stored steps of its K
// chains: importance weights between neighbouring rungs in both directions, each with its standard error, its effective sample
// size and its Kish size.  An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_evidence_ratios).  The log-posteriors are those of the
// handle's own calc_logp_device, called with each rung's parameters on the rows of a chunk (evidence_plan.hpp has the host's
// decisions: at most three calls per chunk of a rung); the effective sample size is that of the existing entry point's body
// (rhat_state.hpp: ess_compute of mcmcpp_hip_effective_sample_size_device, on this call's stream and into the handle's message
// slot) on the weights, a chain of one rung in device memory.
//   * evidence_diff_kernel (evidence_kernels.hpp, shared with bridge.hip): thread = a draw of the chunk: u = (double)logp_other -
//     (double)logp_own, stored at the draw's place of the weights buffer [N]; the largest u that is neither NaN nor +inf and the
//     counts of non-finite u and of NaN or +inf among them, by integer atomics, which no order of arrival changes.
//   * evidence_weights_kernel: block = slice t of sum_fixed over the N draws: e = evidence_exp(u - m) written over u, a tile of
//     kEvidenceTile draws at a time through LDS, from which thread 0 adds e and thread 1 adds e e in ascending order from +0.
//     The slice sums [slices][2] are added in ascending order by the host.
// Nothing depends on the CU count, the chunk size or where a chain lies: a chunk boundary decides which launch writes a u.
// Host steps are uploaded a chunk at a time (MCMCPP_HIP_EVIDENCE_CHUNK_MB, read per call, default 1024); a device chain is read
// where it lies, in chunks of the same size (a step at a time where only every slice-th step is used: the calculator reads
// rows that follow each other).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "evidence_exp.hpp"
#include "evidence_kernels.hpp"
#include "evidence_plan.hpp"
#include "normal_score.hpp"
#include "rhat_state.hpp"

namespace
{
using mcmcpp::evidence_diff_kernel;
using mcmcpp::evidence_key_value;
using mcmcpp::EvidenceState;
using mcmcpp::kEvidenceThreads;
using mcmcpp::kEvidenceTile;

__global__ void __launch_bounds__(kEvidenceThreads) evidence_weights_kernel(double* __restrict__ w, long long N, long long slen, double m, double* __restrict__ part)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double s_e[kEvidenceTile];
    long long first, count;
    mcmcpp::evidence_slice_span(N, slen, (int)blockIdx.x, &first, &count);
    double acc = 0.0;
    for (long long t0 = 0; t0 < count; t0 += kEvidenceTile)
    {
        const int now = (int)(count - t0 < kEvidenceTile ? count - t0 : kEvidenceTile);
        for (int j = threadIdx.x; j < now; j += kEvidenceThreads)
        {
            const double e = mcmcpp::evidence_exp(w[first + t0 + j] - m);
            w[first + t0 + j] = e;
            s_e[j] = e;
        }
        __syncthreads();
        if (threadIdx.x < 2)
            for (int j = 0; j < now; ++j)
            {
                const double e = s_e[j];
                acc = acc + (threadIdx.x == 0 ? e : e * e);
            }
        __syncthreads();
    }
    if (threadIdx.x < 2) part[2 * (size_t)blockIdx.x + threadIdx.x] = acc;
}

template <class T>
int run_request(mcmcpp_hip_sampler& h, const mcmcpp::EvidenceRequest& q, long long n)
{
    std::string& slot = h.error;
    const std::string w(q.what);
    const auto fail = [&](int code, const std::string& msg) { return mcmcpp::analysis_fail(slot, code, msg); };
    const int K = q.K, W = q.W, D = q.D, pairs = mcmcpp::evidence_pairs(K);
    const long long E = (long long)W * D, N = n * W;
    const size_t step_bytes = sizeof(T) * (size_t)E;
    const long long chain_stride_steps = q.chain_stride_steps ? q.chain_stride_steps : q.n_steps;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    ANALYSIS_TRY(slot, hipSetDevice(q.device));
    hipDeviceProp_t prop;
    ANALYSIS_TRY(slot, hipGetDeviceProperties(&prop, q.device));
    if (q.on_device)
        if (int rc = mcmcpp::check_device_steps(slot, q.what, q.device_steps, step_bytes * (size_t)((K - 1) * chain_stride_steps + q.n_steps), q.device)) return rc;

    // the weights as the ESS call sees them: a chain of one rung, n steps of W walkers of one parameter, split
    const mcmcpp::RhatRequest ess_request = mcmcpp::rhat_device_request("effective_sample_size_device", MCMCPP_HIP_F64, q.device, nullptr, 1, 0, n, 1, W, 1, 1);
    const long long ess_n = n;  // (n >= 4 and the W >= 2 walkers of a handle: what the call's own check asks of the halves, L >= 2 and M >= 2)
    const mcmcpp::RhatShape ess_shape = mcmcpp::rhat_shape(1, n, W, 1);

    const long long per = mcmcpp::evidence_steps_per_chunk(mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_EVIDENCE_CHUNK_MB", 1024), step_bytes, q.on_device, q.slice);
    const long long chunk_steps = n < per ? n : per, chunk_draws = chunk_steps * W;
    const mcmcpp::EvidenceWeightsPlan plan = mcmcpp::evidence_weights_plan(N);
    if (!mcmcpp::evidence_grid_fits(chunk_draws)) return fail(MCMCPP_HIP_E_ARG, w + ": too many draws in a chunk for a launch grid (lower MCMCPP_HIP_EVIDENCE_CHUNK_MB)");

    mcmcpp::DeviceBuffer<> d_chunk;
    mcmcpp::DeviceBuffer<T> d_lp;
    mcmcpp::DeviceBuffer<double> d_w[2], d_part;
    mcmcpp::DeviceBuffer<EvidenceState> d_state;
    mcmcpp::Stream stream;  // (behind the buffers: the stream is idle and gone when they go)
    ANALYSIS_TRY(slot, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    if (!q.on_device && d_chunk.alloc(step_bytes * (size_t)chunk_steps) != hipSuccess) return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the upload buffer");
    if (d_lp.alloc(sizeof(T) * 3 * (size_t)chunk_draws) != hipSuccess || d_part.alloc(8 * 2 * 2 * (size_t)plan.slices) != hipSuccess ||
        d_state.alloc(2 * sizeof(EvidenceState)) != hipSuccess)
        return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the log-posteriors of a chunk");
    for (int j = 0; j < (K > 2 ? 2 : 1); ++j)  // (a rung of a ladder of two belongs to one pair)
        if (d_w[j].alloc(8 * (size_t)N) != hipSuccess)
            return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * (size_t)N) + " bytes of the weights of a pair and direction");

    const size_t outs = 2 * (size_t)pairs;
    std::vector<double> log_ratio(outs, nan), mcse(outs, nan), ess(outs, nan), kish(outs, nan), max_u(outs, nan);
    std::vector<int64_t> nonfinite(outs, 0);
    std::vector<double> part(2 * (size_t)plan.slices);
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
                                   (const T*)(d_lp.get() + (size_t)(1 + j) * chunk_draws), (const T*)d_lp.get(), count, d_w[j].get() + (size_t)(done * W),
                                   d_state.get() + j);
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
            if (st[j].bad) continue;  // a NaN or +inf u: the figures of this (d, p) stay NaN
            const double m = evidence_key_value(st[j].max_key);
            max_u[at] = m;
            if (m == -inf)  // no draw inside the other rung's support
            {
                log_ratio[at] = -inf;
                continue;
            }
            hipLaunchKernelGGL(evidence_weights_kernel, dim3(plan.blocks), dim3(kEvidenceThreads), 0, stream, d_w[j].get(), N, plan.slen, m, d_part.get() + 2 * (size_t)plan.slices * j);
            ANALYSIS_TRY(slot, hipGetLastError());
            ANALYSIS_TRY(slot, hipMemcpyAsync(part.data(), d_part.get() + 2 * (size_t)plan.slices * j, 8 * part.size(), hipMemcpyDeviceToHost, stream));
            ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
            double S1 = part[0], S2 = part[1];
            for (int t = 1; t < plan.slices; ++t)
            {
                S1 = S1 + part[2 * (size_t)t];
                S2 = S2 + part[2 * (size_t)t + 1];
            }
            const double Nd = (double)N, wbar = S1 / Nd;
            const double lme = m + mcmcpp::normal_score_log(wbar);
            const double var = S2 / Nd - wbar * wbar;
            const double rel2 = (var > 0.0 ? var : 0.0) / (wbar * wbar);
            mcmcpp::RhatRequest chain = ess_request;
            chain.device_steps = d_w[j].get();
            mcmcpp::EssOutputs eo{};
            double ess_value = nan;
            eo.ess = &ess_value;
            if (int erc = mcmcpp::nested_result(slot, q.what, mcmcpp::ess_compute(slot, chain, 0, 0, prop, ess_n, ess_shape, stream, eo))) return erc;
            log_ratio[at] = lme;
            kish[at] = (S1 * S1) / S2;
            ess[at] = ess_value;
            mcse[at] = rel2 == 0.0 ? 0.0 : std::sqrt(rel2 / ess_value);
        }
    }
    // both directions estimate log(Z_p / Z_{p+1}): the reverse one's lme is the logarithm of the inverse ratio
    for (int p = 0; p < pairs; ++p) log_ratio[(size_t)mcmcpp::evidence_index(K, 1, p)] = -log_ratio[(size_t)mcmcpp::evidence_index(K, 1, p)];

    // the call has succeeded: the outputs
    const mcmcpp::EvidenceOutputs& o = q.out;
    const auto give = [&](double* out, const std::vector<double>& v) {
        if (out) std::memcpy(out, v.data(), 8 * v.size());
    };
    give(o.log_ratio, log_ratio);
    give(o.mcse, mcse);
    give(o.ess, ess);
    give(o.kish, kish);
    give(o.max_u, max_u);
    if (o.nonfinite) std::memcpy(o.nonfinite, nonfinite.data(), 8 * nonfinite.size());
    for (int d = 0; d < 2; ++d)
    {
        double total = 0.0, squares = 0.0;
        for (int p = 0; p < pairs; ++p)
        {
            const size_t at = (size_t)mcmcpp::evidence_index(K, d, p);
            total = total + log_ratio[at];
            squares = squares + mcse[at] * mcse[at];
        }
        if (o.log_ratio_total) o.log_ratio_total[d] = total;
        if (o.mcse_total) o.mcse_total[d] = std::sqrt(squares);
    }
    if (o.num_draws) *o.num_draws = N;
    return MCMCPP_HIP_OK;
}
}  // namespace

namespace mcmcpp
{
int evidence_check(mcmcpp_hip_sampler& h, const EvidenceRequest& q, long long* used_steps)
{
    const std::string w(q.what);
    const auto fail = [&](const std::string& msg) { return analysis_fail(h.error, MCMCPP_HIP_E_ARG, w + ": " + msg); };
    if (q.slice < 1) return fail("slice_interval >= 1");
    const long long n = q.n_steps < 1 ? 0 : (q.n_steps + q.slice - 1) / q.slice;
    if (n < 4) return fail("the effective sample size needs four used steps of a rung (n >= 4): there are " + std::to_string(n));
    if (q.chain_stride_steps < 0 || (q.chain_stride_steps > 0 && q.chain_stride_steps < q.n_steps))
        return fail("chain_stride_steps must be 0 (the chains follow each other) or at least n_steps");
    if (q.on_device ? !q.device_steps : !q.steps) return fail("the steps must not be NULL");
    if (!q.on_device)
        for (int64_t k = 0; k < q.K; ++k)
            for (int64_t s = 0; s < q.n_steps; s += q.slice)
                if (!q.steps[k * q.n_steps + s]) return fail("a step pointer is NULL");
    *used_steps = n;
    return MCMCPP_HIP_OK;
}

int evidence_compute(mcmcpp_hip_sampler& h, const EvidenceRequest& q)
{
    // every check that needs no device
    long long n = 0;
    if (int rc = evidence_check(h, q, &n)) return rc;
    return q.dtype == MCMCPP_HIP_F64 ? run_request<double>(h, q, n) : run_request<float>(h, q, n);
}
}  // namespace mcmcpp
