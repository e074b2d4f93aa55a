// ess.hip -- the effective sample size and integrated autocorrelation time of every parameter over the walkers of K chains:
// the multi-sequence estimator of BDA3 / Stan that goes with the split R-hat of rhat.hip, over the same M = K H W sequences.
// An extension: the reference's AutoCorrCalc (autocorr.hip) takes one pooled chain and knows no between-chain variance.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_effective_sample_size): all arithmetic fp64, every operation
// rounded on its own, every sum of one fixed shape, nothing added atomically.  A result is a function of the data alone.
//
//   * Phase 1 is the R-hat state (rhat_state.hpp): sequence means in device memory, within and between on the host.
//   * ess_lag_kernel: A_m[t] = sum over s of e_s e_{s+t}, e = x - sequence_mean, in ascending s.  Lanes lie along the W*P
//     contiguous elements of a step row, one element a lane; block z takes one (chain, half); the four wavefronts of a
//     workgroup take four consecutive lag blocks of kEssLagBlock lags of the same 64 series, so that their rereads of a row
//     are served by the CU's cache.  A lane keeps its block's accumulators and a ring of the next kEssLagBlock converted
//     samples in registers; the loop over s is unrolled by the block so that the ring is indexed statically, kEssRowsInFlight
//     rows' loads of both streams in flight.  The block of lag 0 takes its leading sample from the ring: one stream.
//   * ess_slice_sums_kernel / ess_slice_join_kernel: sum_fixed over m of A_m[t], per (lag, parameter): [lags][P] sums.
//   * The host divides, forms rho, walks the windows (ess_plan.hpp) and decides whether another round of lags is needed.
// A device chain is read in place.  Of host chains one (chain, half) is the unit of upload; the units stay in device memory
// across the rounds where they all fit and are uploaded again in every round where they do not.
// The entry points check, open the device, probe a device chain's range and make a stream; their body is ess_compute
// (rhat_state.hpp), which rank.hip and summary.hip call on chains of their own, on their stream and into their message slot.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mcmcpp_hip.h"
#include "analysis_host.hpp"
#include "ess_plan.hpp"
#include "rhat_state.hpp"

namespace
{
constexpr int B = mcmcpp::kEssLagBlock;
constexpr int R = mcmcpp::kEssRowsInFlight;
constexpr int kThreads = mcmcpp::kEssThreads;

// Steps [s0, s0 + B) of one series against the lags [t0, t0 + B), all of whose products exist.  rows: the wavefront's first element in
// step 0 of its half (a lane reads element `lane` behind it); step s is `stride` elements further.  ring[q % B] holds e_{t0 + q}: on entry for q in [s0, s0 + B - 1);
// step s brings e_{s + t0 + B - 1} in, in place of e_{s + t0 - 1}.  s0 is a multiple of B: the ring is indexed statically.
template <class T, bool First>
__device__ __forceinline__ void ess_group(const T* rows, unsigned lane, long long stride, long long s0, long long t0, double mu, double (&ring)[B], double (&acc)[B])
{
    const T* lead_at = rows + s0 * stride;
    const T* ring_at = lead_at + (t0 + (B - 1)) * stride;
#pragma unroll
    for (int c = 0; c < B / R; ++c)
    {
        double nx[R], ld[R];
#pragma unroll
        for (int u = 0; u < R; ++u)
        {
            nx[u] = (double)(ring_at + u * stride)[lane];
            if (!First) ld[u] = (double)(lead_at + u * stride)[lane];
        }
        lead_at += R * stride;
        ring_at += R * stride;
#pragma unroll
        for (int u = 0; u < R; ++u)
        {
            const int i = c * R + u;
            ring[(i + B - 1) % B] = nx[u] - mu;
            const double lead = First ? ring[i % B] : ld[u] - mu;
#pragma unroll
            for (int j = 0; j < B; ++j) acc[j] = acc[j] + lead * ring[(i + j) % B];
        }
        __builtin_amdgcn_sched_barrier(0);  // (the next rows' loads stay behind these products: their registers are the ring's)
    }
}

// Steps [s0, s_end) at the end of the sequence, R at a time: ring[j] holds e_{s + t0 + j} and moves down one slot a step; a
// product whose second sample lies past the sequence is left out (s + t0 + j < L), a sample past it is not read.
template <class T, bool First>
__device__ __forceinline__ void ess_tail(const T* rows, unsigned lane, long long stride, long long s0, long long s_end, long long t0, long long L, double mu, double (&ring)[B],
                                         double (&acc)[B])
{
    for (long long sc = s0; sc < s_end; sc += R)
    {
        double nx[R], ld[R];
#pragma unroll
        for (int u = 0; u < R; ++u)
        {
            const long long s = sc + u;
            nx[u] = s + t0 + (B - 1) < L ? (double)(rows + (s + t0 + (B - 1)) * stride)[lane] : 0.0;
            if (!First) ld[u] = s + t0 < L ? (double)(rows + s * stride)[lane] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < R; ++u)
        {
            const long long left = L - t0 - (sc + u);  // products of this step: j < left
            ring[B - 1] = nx[u] - mu;
            const double lead = First ? ring[0] : ld[u] - mu;
#pragma unroll
            for (int j = 0; j < B; ++j)
                if (j < left) acc[j] = acc[j] + lead * ring[j];
#pragma unroll
            for (int j = 0; j < B - 1; ++j) ring[j] = ring[j + 1];
        }
    }
}

template <class T, bool First>
__device__ __forceinline__ void ess_series(const T* rows, unsigned lane, long long stride, long long t0, long long L, double mu, double (&acc)[B])
{
    double ring[B];
#pragma unroll
    for (int q = 0; q < B - 1; ++q) ring[q] = (t0 + q < L ? (double)(rows + (t0 + q) * stride)[lane] : 0.0) - mu;
    ring[B - 1] = 0.0;
    const mcmcpp::EssWalk w = mcmcpp::ess_block_walk(L, t0);
    long long s0 = 0;
    for (; s0 < w.full_end; s0 += B) ess_group<T, First>(rows, lane, stride, s0, t0, mu, ring, acc);
    ess_tail<T, First>(rows, lane, stride, s0, w.lead_end, t0, L, mu, ring, acc);
}

// Block (x, y, z): elements [64 x, 64 x + 64); wavefront v takes lag block 4 y + v of the round's `blocks`, lags
// [t_first + 32 (4 y + v), ...); z = kl * H + h, (chain, half) z_first + z of the sequences.  Step s of that half is at
// base + kl * chain_stride + h * half_offset + s * step_stride (elements).  A: [lag of the round][series].
template <class T>
__global__ void __launch_bounds__(kThreads)
ess_lag_kernel(const T* base, long long step_stride, long long chain_stride, long long half_offset, int H, long long E, long long L, long long t_first, long long blocks,
               int z_first, const double* __restrict__ seq_mean, double* __restrict__ A, long long series)
{
    const unsigned lane = threadIdx.x % mcmcpp::kEssWave;
    const long long e0 = (long long)blockIdx.x * mcmcpp::kEssWave, e = e0 + lane;
    const long long b = (long long)blockIdx.y * mcmcpp::kEssBlocksPerGroup + threadIdx.x / mcmcpp::kEssWave;
    if (e >= E || b >= blocks) return;
    const int kl = (int)blockIdx.z / H, h = (int)blockIdx.z % H;
    const long long i = ((long long)z_first + blockIdx.z) * E + e;
    const long long t0 = t_first + b * B;
    const T* rows = base + (long long)kl * chain_stride + (long long)h * half_offset + e0;  // (the same for every lane: a lane reads element `lane` of it)
    const double mu = seq_mean[i];
    double acc[B];
#pragma unroll
    for (int j = 0; j < B; ++j) acc[j] = 0.0;
    if (t0 == 0)
        ess_series<T, true>(rows, lane, step_stride, t0, L, mu, acc);
    else
        ess_series<T, false>(rows, lane, step_stride, t0, L, mu, acc);
    double* out = A + (b * B) * series + i;
#pragma unroll
    for (int j = 0; j < B; ++j) out[j * series] = acc[j];
}

// Thread (slice j, parameter p) of lag blockIdx.y of the round: its slice of A[lag][m P + p] over m, in ascending order from
// +0.  part: [lag][slices][P]
__global__ void __launch_bounds__(kThreads)
ess_slice_sums_kernel(const double* __restrict__ A, int P, long long M, long long slen, int slices, long long lag_first, double* __restrict__ part)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)slices * P) return;
    const int j = (int)(id / P), p = (int)(id % P);
    const long long lag = lag_first + blockIdx.y;
    const double* a = A + lag * M * P + p;
    const long long m0 = (long long)j * slen, m1 = (j + 1) * slen < M ? (j + 1) * slen : M;
    double sum = 0.0;
    long long m = m0;
    for (; m + R <= m1; m += R)
    {
        double x[R];
#pragma unroll
        for (int u = 0; u < R; ++u) x[u] = a[(m + u) * P];
#pragma unroll
        for (int u = 0; u < R; ++u) sum = sum + x[u];
    }
    for (; m < m1; ++m) sum = sum + a[m * P];
    part[(lag * slices + j) * P + p] = sum;
}

// Thread (lag, parameter): the slice sums in ascending order.  part [lags][slices][P] -> S [lags][P]
__global__ void __launch_bounds__(kThreads)
ess_slice_join_kernel(const double* __restrict__ part, int P, long long lags, int slices, double* __restrict__ S)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= lags * P) return;
    const long long lag = id / P;
    const int p = (int)(id % P);
    const double* a = part + (lag * slices) * P + p;
    double s = a[0];
    for (int j = 1; j < slices; ++j) s = s + a[(long long)j * P];
    S[id] = s;
}

thread_local std::string g_ess_error;

using mcmcpp::EssOutputs;

template <class T>
int run_request(std::string& slot, const mcmcpp::RhatRequest& r, int64_t max_lag, int64_t n_functions, const hipDeviceProp_t& prop, long long n,
                const mcmcpp::RhatShape& shape, hipStream_t stream, const EssOutputs& out)
{
    const auto ess_fail = [&](int code, const std::string& msg) { return mcmcpp::analysis_fail(slot, code, msg); };
    const std::string w(r.what);
    const int K = r.K, P = r.P, H = shape.H;
    const long long E = (long long)r.W * P, L = shape.L, M = shape.M, series = M * P;
    const size_t step_bytes = sizeof(T) * (size_t)E;
    mcmcpp::RhatState st;
    mcmcpp::DeviceBuffer<T> d_units;
    mcmcpp::DeviceBuffer<double> d_A, d_part, d_S;
    std::vector<double> S;              // [lags done][P]
    mcmcpp::IdleOnReturn idle{stream};  // (behind the buffers: the stream is idle when they go)
    if (int rc = mcmcpp::rhat_sequences_state(slot, r, prop, n, shape, stream, st)) return rc;
    ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
    st.chunk.reset();  // (phase 1's upload buffer and slice state have done their work)
    st.first.reset();
    st.state.reset();
    const double* seq_mean = st.seq.get();
    const double *h_mean = st.h_res.data(), *h_within = h_mean + P, *h_between = h_within + P;

    const long long cap = mcmcpp::ess_cap(L, max_lag), kmax = mcmcpp::ess_kmax(cap), F = mcmcpp::ess_function_lags(n_functions, cap);
    mcmcpp::EssKnobs knobs = mcmcpp::ess_knobs_from_env();
    const mcmcpp::RhatSumPlan sum = mcmcpp::rhat_sum_plan(M, P, 1);

    // where the lag kernel finds step s of (chain, half) z
    const int units = K * H;
    const long long a1 = mcmcpp::rhat_half_begin(n, L, 1);
    bool resident = true;
    const T* base = static_cast<const T*>(r.device_steps);
    long long step_stride = r.slice * E, chain_stride = (r.chain_stride_steps ? r.chain_stride_steps : r.n_steps) * E, half_offset = a1 * r.slice * E;
    if (!r.on_device)
    {
        if (d_units.alloc(step_bytes * (size_t)L * units) != hipSuccess)
        {
            resident = false;
            if (d_units.alloc(step_bytes * (size_t)L) != hipSuccess)
                return ess_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(step_bytes * (size_t)L) + " bytes of one (chain, half)");
        }
        base = d_units.get();
        step_stride = E;
        half_offset = L * E;
        chain_stride = (long long)H * L * E;
    }
    const auto upload = [&](int u, T* dst) -> hipError_t {
        const void* const* src = r.steps + (size_t)(u / H) * n + (u % H ? a1 : 0);
        return mcmcpp::copy_steps(dst, [&](long long s) { return src[s]; }, 0, L, step_bytes, hipMemcpyHostToDevice, stream);
    };
    if (!r.on_device && resident)
        for (int u = 0; u < units; ++u) ANALYSIS_TRY(slot, upload(u, d_units.get() + (size_t)u * L * E));

    std::vector<mcmcpp::EssWindow> win(P);
    long long done = 0, previous = 0;
    const auto rho_of = [&](int p, long long t) {
        return mcmcpp::ess_rho(t, mcmcpp::ess_gamma(S[(size_t)t * P + p], (double)M, (double)L), h_within[p], mcmcpp::ess_varplus(h_within[p], h_between[p], (double)L));
    };
    for (bool more = true; more;)
    {
        long long lags = mcmcpp::ess_round_lags(done, previous, knobs, series, cap, n_functions);
        if (lags < B) return ess_fail(MCMCPP_HIP_E_UNSUPPORTED, w + ": a round without lags");
        if (mcmcpp::grow(d_A, 8 * (size_t)lags * series, stream) != hipSuccess)
        {
            knobs.work_bytes = 0;  // one block a round from here on
            lags = B;
            if (mcmcpp::grow(d_A, 8 * (size_t)lags * series, stream) != hipSuccess)
                return ess_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * (size_t)lags * series) + " bytes of one block of lagged products");
        }
        if (mcmcpp::grow(d_part, 8 * (size_t)lags * sum.slices * P, stream) != hipSuccess || mcmcpp::grow(d_S, 8 * (size_t)lags * P, stream) != hipSuccess)
            return ess_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the sums of a round of " + std::to_string(lags) + " lags");
        const long long blocks = lags / B;
        if (r.on_device || resident)
        {
            const mcmcpp::EssGrid g = mcmcpp::ess_lag_grid(E, blocks, units);
            hipLaunchKernelGGL(ess_lag_kernel<T>, dim3(g.x, g.y, g.z), dim3(kThreads), 0, stream, base, step_stride, chain_stride, half_offset, H, E, L, done, blocks, 0,
                               seq_mean, d_A.get(), series);
            ANALYSIS_TRY(slot, hipGetLastError());
        }
        else
            for (int u = 0; u < units; ++u)
            {
                ANALYSIS_TRY(slot, upload(u, d_units.get()));  // (in stream order behind the kernel that read the unit before)
                const mcmcpp::EssGrid g = mcmcpp::ess_lag_grid(E, blocks, 1);
                hipLaunchKernelGGL(ess_lag_kernel<T>, dim3(g.x, g.y, g.z), dim3(kThreads), 0, stream, base, step_stride, chain_stride, half_offset, 1, E, L, done, blocks,
                                   u, seq_mean, d_A.get(), series);
                ANALYSIS_TRY(slot, hipGetLastError());
            }
        const unsigned sum_blocks = (unsigned)(((long long)sum.slices * P + kThreads - 1) / kThreads);
        for (long long l0 = 0; l0 < lags; l0 += mcmcpp::kRhatGridYMax)
        {
            const long long now = lags - l0 < mcmcpp::kRhatGridYMax ? lags - l0 : mcmcpp::kRhatGridYMax;
            hipLaunchKernelGGL(ess_slice_sums_kernel, dim3(sum_blocks, (unsigned)now), dim3(kThreads), 0, stream, (const double*)d_A.get(), P, M, sum.slen, sum.slices, l0,
                               d_part.get());
            ANALYSIS_TRY(slot, hipGetLastError());
        }
        hipLaunchKernelGGL(ess_slice_join_kernel, dim3((unsigned)((lags * P + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (const double*)d_part.get(), P, lags,
                           sum.slices, d_S.get());
        ANALYSIS_TRY(slot, hipGetLastError());
        S.resize((size_t)(done + lags) * P);
        ANALYSIS_TRY(slot, hipMemcpyAsync(S.data() + (size_t)done * P, d_S.get(), 8 * (size_t)lags * P, hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
        done += lags;
        previous = lags;
        more = done < F;
        for (int p = 0; p < P; ++p)
        {
            win[p] = mcmcpp::ess_walk_window([&](long long t) { return rho_of(p, t); }, done, kmax);
            more = more || win[p].state < 0;
        }
    }

    // the call has succeeded: the outputs
    const double N = (double)(M * L), nan = std::numeric_limits<double>::quiet_NaN();
    for (int p = 0; p < P; ++p)
    {
        const double tau = mcmcpp::ess_tau(win[p].total, N);
        if (out.tau) out.tau[p] = tau;
        if (out.ess) out.ess[p] = N / tau;
        if (out.lags_used) out.lags_used[p] = 2 * win[p].pairs;
        if (out.closed) out.closed[p] = win[p].state == 1;
        for (long long t = 0; t < n_functions; ++t)
        {
            if (out.rho) out.rho[(size_t)p * n_functions + t] = t < F ? rho_of(p, t) : nan;
            if (out.autocov) out.autocov[(size_t)p * n_functions + t] = t < F ? mcmcpp::ess_gamma(S[(size_t)t * P + p], (double)M, (double)L) : nan;
        }
        if (out.rhat) out.rhat[p] = std::sqrt(mcmcpp::ess_varplus(h_within[p], h_between[p], (double)L) / h_within[p]);
    }
    if (out.mean) std::memcpy(out.mean, h_mean, 8 * (size_t)P);
    if (out.within) std::memcpy(out.within, h_within, 8 * (size_t)P);
    if (out.between) std::memcpy(out.between, h_between, 8 * (size_t)P);
    if (out.sequence_length) *out.sequence_length = L;
    if (out.num_sequences) *out.num_sequences = M;
    return MCMCPP_HIP_OK;
}

int ess_entry(const mcmcpp::RhatRequest& r, int64_t max_lag, int64_t n_functions, const EssOutputs& out)
{
    const auto ess_fail = [](int code, const std::string& msg) { return mcmcpp::analysis_fail(g_ess_error, code, msg); };
    const std::string w(r.what);
    long long n = 0;
    mcmcpp::RhatShape shape;
    if (int rc = mcmcpp::rhat_check_request(g_ess_error, r, &n, &shape)) return rc;
    if (max_lag < 0) return ess_fail(MCMCPP_HIP_E_ARG, w + ": max_lag >= 0 (0: up to L - 1)");
    if (n_functions < 0) return ess_fail(MCMCPP_HIP_E_ARG, w + ": n_functions >= 0");
    hipDeviceProp_t prop;
    std::string why;
    int device = r.device;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return ess_fail(rc, w + ": " + why);
    if (int rc = mcmcpp::rhat_check_device_steps(g_ess_error, r, device)) return rc;
    mcmcpp::Stream stream;
    ANALYSIS_TRY(g_ess_error, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    return mcmcpp::ess_compute(g_ess_error, r, max_lag, n_functions, prop, n, shape, stream, out);
}
}  // namespace

namespace mcmcpp
{
int ess_compute(std::string& slot, const RhatRequest& r, int64_t max_lag, int64_t n_functions, const hipDeviceProp_t& prop, long long n, const RhatShape& shape,
                hipStream_t stream, const EssOutputs& out)
{
    return r.dtype == MCMCPP_HIP_F64 ? run_request<double>(slot, r, max_lag, n_functions, prop, n, shape, stream, out)
                                     : run_request<float>(slot, r, max_lag, n_functions, prop, n, shape, stream, out);
}
}  // namespace mcmcpp

extern "C"
{
const char* mcmcpp_hip_effective_sample_size_last_error(void) { return g_ess_error.c_str(); }

int mcmcpp_hip_effective_sample_size(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps, int32_t num_walkers,
                                     int32_t num_params, int32_t split, int64_t max_lag, int64_t n_functions, double* ess, double* tau, int64_t* lags_used,
                                     int64_t* closed, double* rho, double* autocov, double* rhat, double* mean, double* within, double* between,
                                     int64_t* sequence_length, int64_t* num_sequences)
{
    return ess_entry(mcmcpp::rhat_host_request("effective_sample_size", dtype, device, steps, num_chains, n_steps, num_walkers, num_params, split), max_lag, n_functions,
                     EssOutputs{ess, tau, lags_used, closed, rho, autocov, rhat, mean, within, between, sequence_length, num_sequences});
}

int mcmcpp_hip_effective_sample_size_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains, int64_t chain_stride_steps, int64_t n_steps,
                                            int64_t slice_interval, int32_t num_walkers, int32_t num_params, int32_t split, int64_t max_lag, int64_t n_functions,
                                            double* ess, double* tau, int64_t* lags_used, int64_t* closed, double* rho, double* autocov, double* rhat, double* mean,
                                            double* within, double* between, int64_t* sequence_length, int64_t* num_sequences)
{
    return ess_entry(mcmcpp::rhat_device_request("effective_sample_size_device", dtype, device, device_steps, num_chains, chain_stride_steps, n_steps, slice_interval,
                                                 num_walkers, num_params, split),
                     max_lag, n_functions, EssOutputs{ess, tau, lags_used, closed, rho, autocov, rhat, mean, within, between, sequence_length, num_sequences});
}
}
