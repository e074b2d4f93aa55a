// gaussian_bridge.hip -- the evidence of one chain's target from an ordinary run: the bridge estimate between the target and a
// Gaussian q = N(mean, L L^T) fitted to its draws (Overstall & Forster 2010; Gronau et al. 2017).  q is normalised, so the
// bridge's log-ratio is log Z itself.  An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_evidence_gaussian).  gaussian_bridge_plan.hpp has the host's
// decisions and the arithmetic of a row and of log q, one text for host and device; the log-posteriors are the handle's own
// calc_logp_device; the pair's figures are bridge.hip's (bridge_pair.hpp).  Three kernels are this file's:
//   * gaussian_rows_kernel: thread = a proposal.  It reaches the row's place j D of the caller's pcg64 stream through the jump
//     table (one entry per set bit of j), steps D times, turns each raw draw into a normal score, keeps the scores in its column
//     of LDS and forms x = mean + L z there, from the last coordinate up.  L and the mean are in LDS, read by all lanes at one
//     address.  The block then writes its rows in the order they lie in memory, rounded once to the handle's dtype.  It writes
//     rows and nothing else.
//   * gaussian_log_q_kernel: the block loads its rows in the order they lie in memory, widened, into the columns; thread = a
//     row: forward substitution in its column, z_i over x_i, and log q = (-0.5 s) + k.  The same kernel evaluates the rounded
//     proposals and the draws.
//   * gaussian_diff_kernel: thread = a row: u = logp - log q (proposals) or log q - logp (draws), with evidence_kernels.hpp's
//     counts of what is not finite.
// No atomics on doubles, and nothing depends on the CU count, the chunk size or where the chain lies.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bridge_pair.hpp"
#include "evidence_kernels.hpp"
#include "evidence_plan.hpp"
#include "gaussian_bridge_plan.hpp"
#include "pcg128.hpp"
#include "rhat_state.hpp"

namespace
{
using mcmcpp::Affine128;
using mcmcpp::EvidenceState;
using mcmcpp::kGaussianDiffThreads;
using mcmcpp::U128;

// a thread's column of the block's rows in LDS: element d at col[d * stride]
struct LdsColumn
{
    double* col;
    int stride;
    __device__ __forceinline__ double& operator()(int d) const { return col[d * stride]; }
};

// the block's part of dynamic LDS: the Gaussian's parameters, then the columns [D][rows + 1]
__device__ __forceinline__ double* stage_params(double* lds, const double* __restrict__ prm, int D)
{
    const int len = D + D * (D + 1) / 2;
    for (int e = (int)threadIdx.x; e < len; e += (int)blockDim.x) lds[e] = prm[e];
    return lds + len;
}

// The block's elements in the order they lie in memory, e = t, t + rows, ...: element e is coordinate e % D of the block's row
// e / D.  One division per thread; from there the pair is stepped.
struct ElementWalk
{
    int row, d, row_step, d_step, D;
    __device__ __forceinline__ ElementWalk(int t, int rows, int dims) : row(t / dims), d(t % dims), row_step(rows / dims), d_step(rows % dims), D(dims) {}
    __device__ __forceinline__ void next()
    {
        row += row_step, d += d_step;
        if (d >= D) d -= D, ++row;
    }
};

template <class T>
__global__ void __launch_bounds__(256)
gaussian_rows_kernel(T* __restrict__ rows_out, long long j0, long long count, int D, const double* __restrict__ prm, U128 state0, U128 inc,
                     const Affine128* __restrict__ jump, int entries)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    extern __shared__ double lds[];
    const int rows = (int)blockDim.x, stride = rows + 1, t = (int)threadIdx.x;
    double* const s_col = stage_params(lds, prm, D);
    __syncthreads();
    const long long first = (long long)blockIdx.x * rows, local = first + t;
    if (local < count)
    {
        const unsigned long long j = (unsigned long long)(j0 + local);
        U128 s = state0;
        for (int b = 0; b < entries; ++b)
            if ((j >> b) & 1ULL) s = mcmcpp::apply(jump[b], s);
        const LdsColumn z{s_col + t, stride};
        for (int d = 0; d < D; ++d)
        {
            s = mcmcpp::pcg_step(s, inc);
            z(d) = mcmcpp::normal_score(mcmcpp::gaussian_p(mcmcpp::pcg_output(s)));
        }
        mcmcpp::gaussian_row_core(D, lds, z);
    }
    __syncthreads();
    const long long here = count - first < rows ? count - first : rows;
    const int total = (int)here * D;
    T* __restrict__ dst = rows_out + (size_t)first * (size_t)D;
    ElementWalk at(t, rows, D);
    for (int e = t; e < total; e += rows, at.next()) dst[e] = (T)s_col[at.d * stride + at.row];
}

template <class T>
__global__ void __launch_bounds__(256)
gaussian_log_q_kernel(const T* __restrict__ rows_in, long long count, int D, const double* __restrict__ prm, double k, double* __restrict__ log_q_out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    extern __shared__ double lds[];
    const int rows = (int)blockDim.x, stride = rows + 1, t = (int)threadIdx.x;
    double* const s_col = stage_params(lds, prm, D);
    const long long first = (long long)blockIdx.x * rows, local = first + t;
    const long long here = count - first < rows ? count - first : rows;
    const int total = (int)here * D;
    const T* __restrict__ src = rows_in + (size_t)first * (size_t)D;
    ElementWalk at(t, rows, D);
    for (int e = t; e < total; e += rows, at.next()) s_col[at.d * stride + at.row] = (double)src[e];
    __syncthreads();
    if (local < count) log_q_out[local] = mcmcpp::gaussian_log_q_core(D, lds, k, LdsColumn{s_col + t, stride});
}

// target_first: u = logp - log q (on the proposals); else u = log q - logp (on the draws)
template <class T>
__global__ void __launch_bounds__(kGaussianDiffThreads)
gaussian_diff_kernel(const T* __restrict__ lp, const double* __restrict__ lq, long long count, int target_first, double* __restrict__ u_out, EvidenceState* __restrict__ state)
{
    const long long i = (long long)blockIdx.x * kGaussianDiffThreads + threadIdx.x;
    double u = 0.0;
    if (i < count)
    {
        const double a = (double)lp[i], b = lq[i];
        u = target_first ? a - b : b - a;
        u_out[i] = u;
    }
    mcmcpp::evidence_note_u(u, i < count, state);
}

// GPU time of one kernel over the launches of a call, between two events around each launch on the call's stream
// (mcmcpp_hip_evidence_gaussian_last_timing).  collect() is called behind a synchronisation of the stream, before the next begin().
struct KernelClock
{
    mcmcpp::Event first, last;
    bool pending = false;
    double ms = 0.0;
    hipError_t create()
    {
        if (const hipError_t e = hipEventCreate(first.replace())) return e;
        return hipEventCreate(last.replace());
    }
    void begin(hipStream_t stream) { (void)hipEventRecord(first, stream); }
    void end(hipStream_t stream)
    {
        (void)hipEventRecord(last, stream);
        pending = true;
    }
    void collect()
    {
        float one = 0.0f;
        if (pending && hipEventElapsedTime(&one, first, last) == hipSuccess) ms += (double)one;
        pending = false;
    }
};
thread_local double g_last_rows_ms = 0.0, g_last_log_q_ms = 0.0;  // of this thread's last successful call

template <class T>
int run_request(mcmcpp_hip_sampler& h, const mcmcpp::GaussianBridgeRequest& g, long long n)
{
    const mcmcpp::EvidenceRequest& q = g.q;
    std::string& slot = h.error;
    const std::string w(q.what);
    const auto fail = [&](int code, const std::string& msg) { return mcmcpp::analysis_fail(slot, code, msg); };
    const int W = q.W, D = q.D;
    const long long E = (long long)W * D, N = n * W;
    const size_t step_bytes = sizeof(T) * (size_t)E;

    ANALYSIS_TRY(slot, hipSetDevice(q.device));
    hipDeviceProp_t prop;
    ANALYSIS_TRY(slot, hipGetDeviceProperties(&prop, q.device));
    if (q.on_device)
        if (int rc = mcmcpp::check_device_steps(slot, q.what, q.device_steps, step_bytes * (size_t)q.n_steps, q.device)) return rc;

    // the draws go a chunk of steps at a time, as in the other two evidence calls; the proposals in chunks of as many rows as a
    // chunk of steps that follow each other holds
    const size_t chunk_bytes = mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_EVIDENCE_CHUNK_MB", 1024);
    const long long per = mcmcpp::evidence_steps_per_chunk(chunk_bytes, step_bytes, q.on_device, q.slice);
    const long long per_made = mcmcpp::evidence_steps_per_chunk(chunk_bytes, step_bytes, false, 1);
    const long long chunk_steps = n < per ? n : per, made_rows = (n < per_made ? n : per_made) * W;
    const int rows = mcmcpp::gaussian_rows_per_block(D);
    const size_t lds_bytes = mcmcpp::gaussian_lds_bytes(D, rows);
    if (!mcmcpp::evidence_grid_fits(made_rows) || !mcmcpp::gaussian_grid_fits(made_rows, D))
        return fail(MCMCPP_HIP_E_ARG, w + ": too many draws in a chunk for a launch grid (lower MCMCPP_HIP_EVIDENCE_CHUNK_MB)");
    if (!mcmcpp::bridge_grid_fits(N)) return fail(MCMCPP_HIP_E_ARG, w + ": too many draws for a launch grid");

    // the Gaussian as the kernels read it, k, and the jump table of the caller's stream
    std::vector<double> prm(mcmcpp::gaussian_param_doubles(D));
    mcmcpp::gaussian_pack(D, g.mean, g.chol, prm.data());
    const double k = mcmcpp::gaussian_log_norm(D, prm.data());
    U128 state0, inc;
    mcmcpp::pcg_seed(g.seed, g.stream, &state0, &inc);
    std::vector<Affine128> jump((size_t)mcmcpp::gaussian_jump_entries(N));  // entry b: from row j's place to row (j + 2^b)'s
    for (size_t b = 0; b < jump.size(); ++b) jump[b] = mcmcpp::pcg_jump(inc, mcmcpp::gaussian_position(1LL << b, D, 0));

    mcmcpp::DeviceBuffer<> d_chunk;
    mcmcpp::DeviceBuffer<T> d_made, d_lp;
    mcmcpp::DeviceBuffer<double> d_prm, d_lq, d_u[2];
    mcmcpp::DeviceBuffer<Affine128> d_jump;
    mcmcpp::BridgePairScratch scratch;
    mcmcpp::DeviceBuffer<EvidenceState> d_state;
    KernelClock rows_clock, log_q_clock;
    mcmcpp::Stream stream;  // (behind the buffers and the events: the stream is idle and gone when they go)
    ANALYSIS_TRY(slot, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    ANALYSIS_TRY(slot, rows_clock.create());
    ANALYSIS_TRY(slot, log_q_clock.create());
    if (!q.on_device && d_chunk.alloc(step_bytes * (size_t)chunk_steps) != hipSuccess) return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the upload buffer");
    if (d_made.alloc(sizeof(T) * (size_t)made_rows * (size_t)D) != hipSuccess)
        return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(sizeof(T) * (size_t)made_rows * (size_t)D) + " bytes of the proposals of a chunk");
    if (d_lp.alloc(sizeof(T) * (size_t)made_rows) != hipSuccess || d_lq.alloc(8 * (size_t)made_rows) != hipSuccess || d_prm.alloc(8 * prm.size()) != hipSuccess ||
        d_jump.alloc(sizeof(Affine128) * jump.size()) != hipSuccess || scratch.alloc(N) != hipSuccess || d_state.alloc(2 * sizeof(EvidenceState)) != hipSuccess)
        return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the log-posteriors of a chunk");
    for (int d = 0; d < 2; ++d)
        if (d_u[d].alloc(8 * (size_t)N) != hipSuccess)
            return fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * (size_t)N) + " bytes of the differences of a direction");
    ANALYSIS_TRY(slot, hipMemcpyAsync(d_prm.get(), prm.data(), 8 * prm.size(), hipMemcpyHostToDevice, stream));
    ANALYSIS_TRY(slot, hipMemcpyAsync(d_jump.get(), jump.data(), sizeof(Affine128) * jump.size(), hipMemcpyHostToDevice, stream));
    ANALYSIS_TRY(slot, hipMemsetAsync(d_state.get(), 0, 2 * sizeof(EvidenceState), stream));

    // what the caller asked to see, kept here until the call has succeeded
    const mcmcpp::GaussianBridgeOutputs& o = g.out;
    std::vector<T> made(o.proposals ? (size_t)N * (size_t)D : 0);
    std::vector<double> log_q(o.log_q ? 2 * (size_t)N : 0);

    // log q and u of `count` rows that follow each other from `base`, which are rows [at, at + count) of direction d
    // (its caller has synchronised the stream: the log q kernel of the chunk before is over)
    const auto evaluate = [&](int d, const T* base, long long at, long long count) -> int {
        log_q_clock.collect();
        if (int crc = h.calc_logp_device(g.chain, base, count, d_lp.get())) return mcmcpp::nested_result(slot, q.what, crc);
        log_q_clock.begin(stream);
        hipLaunchKernelGGL(gaussian_log_q_kernel<T>, dim3((unsigned)mcmcpp::gaussian_blocks(count, rows)), dim3((unsigned)rows), lds_bytes, stream, base, count, D,
                           (const double*)d_prm.get(), k, d_lq.get());
        log_q_clock.end(stream);
        hipLaunchKernelGGL(gaussian_diff_kernel<T>, dim3((unsigned)mcmcpp::gaussian_diff_blocks(count)), dim3(kGaussianDiffThreads), 0, stream, (const T*)d_lp.get(),
                           (const double*)d_lq.get(), count, d == 0 ? 1 : 0, d_u[d].get() + (size_t)at, d_state.get() + d);
        ANALYSIS_TRY(slot, hipGetLastError());
        if (o.log_q) ANALYSIS_TRY(slot, hipMemcpyAsync(log_q.data() + (size_t)d * (size_t)N + (size_t)at, d_lq.get(), 8 * (size_t)count, hipMemcpyDeviceToHost, stream));
        return MCMCPP_HIP_OK;
    };

    // direction 1: the draws
    std::vector<const void*> used(q.on_device ? 0 : (size_t)n);
    if (!q.on_device)
        for (long long s = 0; s < n; ++s) used[(size_t)s] = q.steps[(size_t)(s * q.slice)];
    mcmcpp::StepSource<T> src{q.on_device ? nullptr : used.data(), q.on_device ? static_cast<const T*>(q.device_steps) : nullptr, n, q.slice, W, D, stream, &d_chunk, &slot};
    long long done = 0;  // used steps behind the chunks so far
    const int rc = src.for_each_chunk(per, [&](mcmcpp::StepSpan<T> span) -> int {
        // the upload has arrived, and the kernels of the chunk before have read the log-posteriors the calculator overwrites
        ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
        if (int erc = evaluate(1, span.base, done * W, span.n_steps * W)) return erc;  // (rows that follow each other: per == 1 where the steps do not)
        done += span.n_steps;
        return MCMCPP_HIP_OK;
    });
    if (rc) return rc;

    // direction 0: the proposals, made where the calculator reads them
    for (long long j0 = 0; j0 < N; j0 += made_rows)
    {
        const long long count = N - j0 < made_rows ? N - j0 : made_rows;
        ANALYSIS_TRY(slot, hipStreamSynchronize(stream));  // the chunk before is done with the rows and the log-posteriors
        rows_clock.begin(stream);
        hipLaunchKernelGGL(gaussian_rows_kernel<T>, dim3((unsigned)mcmcpp::gaussian_blocks(count, rows)), dim3((unsigned)rows), lds_bytes, stream, d_made.get(), j0, count, D,
                           (const double*)d_prm.get(), state0, inc, (const Affine128*)d_jump.get(), (int)jump.size());
        rows_clock.end(stream);
        ANALYSIS_TRY(slot, hipGetLastError());
        ANALYSIS_TRY(slot, hipStreamSynchronize(stream));  // the calculator works on the handle's stream
        rows_clock.collect();
        if (int erc = evaluate(0, d_made.get(), j0, count)) return erc;
        if (o.proposals)
            ANALYSIS_TRY(slot, hipMemcpyAsync(made.data() + (size_t)j0 * (size_t)D, d_made.get(), sizeof(T) * (size_t)count * (size_t)D, hipMemcpyDeviceToHost, stream));
    }
    EvidenceState st[2];
    ANALYSIS_TRY(slot, hipMemcpyAsync(st, d_state.get(), sizeof st, hipMemcpyDeviceToHost, stream));
    ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
    log_q_clock.collect();

    mcmcpp::BridgePairFigures f;  // a NaN or +inf u: the figures stay NaN
    if (!st[0].bad && !st[1].bad)
    {
        double* const u[2] = {d_u[0].get(), d_u[1].get()};
        if (int prc = mcmcpp::bridge_pair_compute(slot, q.what, q.device, prop, stream, scratch, u, n, W, &f)) return prc;
    }

    // the call has succeeded: the outputs
    if (o.log_evidence) *o.log_evidence = f.log_ratio;
    if (o.mcse) *o.mcse = f.mcse;
    if (o.overlap) *o.overlap = f.overlap;
    if (o.ess) o.ess[0] = f.ess[0], o.ess[1] = f.ess[1];
    if (o.passes) *o.passes = f.passes;
    if (o.converged) *o.converged = f.converged;
    if (o.nonfinite) o.nonfinite[0] = (int64_t)st[0].nonfinite, o.nonfinite[1] = (int64_t)st[1].nonfinite;
    if (o.num_draws) *o.num_draws = N;
    if (o.proposals) std::memcpy(o.proposals, made.data(), sizeof(T) * made.size());
    if (o.log_q) std::memcpy(o.log_q, log_q.data(), 8 * log_q.size());
    g_last_rows_ms = rows_clock.ms, g_last_log_q_ms = log_q_clock.ms;
    return MCMCPP_HIP_OK;
}
}  // namespace

extern "C" void mcmcpp_hip_evidence_gaussian_last_timing(double* rows_ms, double* log_q_ms)
{
    if (rows_ms) *rows_ms = g_last_rows_ms;
    if (log_q_ms) *log_q_ms = g_last_log_q_ms;
}

namespace mcmcpp
{
int gaussian_bridge_compute(mcmcpp_hip_sampler& h, const GaussianBridgeRequest& g)
{
    // every check that needs no device: those of the ratios on the steps of one chain, then the Gaussian
    long long n = 0;
    if (int rc = evidence_check(h, g.q, &n)) return rc;
    const std::string w(g.q.what);
    if (!g.mean || !g.chol) return analysis_fail(h.error, MCMCPP_HIP_E_ARG, w + ": mean and chol must not be NULL");
    int i = 0, d = 0;
    switch (gaussian_check(g.q.D, g.mean, g.chol, &i, &d))
    {
    case kGaussianOk: break;
    case kGaussianTooWide:
        return analysis_fail(h.error, MCMCPP_HIP_E_UNSUPPORTED, w + ": a Gaussian of " + std::to_string(g.q.D) + " parameters; " + std::to_string(kGaussianMaxD) + " at the most");
    case kGaussianMeanNotFinite: return analysis_fail(h.error, MCMCPP_HIP_E_ARG, w + ": mean[" + std::to_string(i) + "] is not finite");
    case kGaussianFactorNotFinite:
        return analysis_fail(h.error, MCMCPP_HIP_E_ARG, w + ": chol[" + std::to_string(i) + "][" + std::to_string(d) + "] is not finite");
    case kGaussianDiagonal:
        return analysis_fail(h.error, MCMCPP_HIP_E_ARG, w + ": chol[" + std::to_string(i) + "][" + std::to_string(i) + "] is not a positive normal number");
    }
    return g.q.dtype == MCMCPP_HIP_F64 ? run_request<double>(h, g, n) : run_request<float>(h, g, n);
}
}  // namespace mcmcpp
