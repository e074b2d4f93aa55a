// rhat.hip -- the Gelman-Rubin potential scale reduction (split R-hat, BDA3 form) of every parameter, with the walkers of K
// chains as sequences: what a user asks of several independent ensembles of one target (num_chains of one handle, or several
// handles) -- have they converged to the same distribution?  An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_gelman_rubin).  Every sum has one fixed shape (sum_fixed:
// rhat_plan.hpp), all arithmetic is fp64 with every operation rounded on its own, and nothing is added atomically: a result is
// a function of the data alone, whatever the schedule, the CU count, the chunk size, or where the chain lies.
//
//   * rhat_series_kernel streams the steps once.  Lanes lie along the W*P contiguous elements of a step row (one 16-byte
//     piece per lane where rows are whole pieces and the base is aligned, else one element); block z takes one (chain, half).
//     A lane keeps c (its sequences' first samples) and the open slice's (sum d, sum d*d), d = x - c, in registers and walks
//     its steps in ascending order, kRhatRowsInFlight rows' loads in flight.  At a slice end it adds the slice sums into its
//     running totals (the lane owns the whole sequence: state slots "total" and "open slice") or stores them to slot
//     [slice] of the state (one block per (element tile, slice)).  The state [z][slot][2][E] and c [z][E] carry everything
//     across upload chunks: a chunk boundary only decides which launch performs an addition, never its operands.
//   * rhat_sequence_kernel: state -> (mean_m, M2_m) as [M][P].
//   * rhat_slice_sums_kernel / rhat_slice_join_kernel: sum_fixed over m of a function of [M][P], per parameter and per chain:
//     the means and within-variances first, then the squared deviations from the mean in a second pass.
// The last step, P square roots, is the host's.  A device chain is read in place; host chains are uploaded chain by chain in
// chunks of MCMCPP_HIP_RHAT_CHUNK_MB (read per call, default 1024).  The argument check and everything up to the figures in
// device memory are also the first phase of mcmcpp_hip_effective_sample_size (ess.hip), which calls them through rhat_state.hpp;
// the entry points' body behind the checks, the open device and the range probe is rhat_compute there, which rank.hip calls.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mcmcpp_hip.h"
#include "analysis_host.hpp"
#include "rhat_plan.hpp"
#include "rhat_state.hpp"

namespace
{
constexpr int kRhatThreads = mcmcpp::kRhatPlanThreads;
constexpr int kRows = mcmcpp::kRhatRowsInFlight;

// V consecutive elements of a row as doubles: one 16-byte load where V > 1 (the plan has checked the alignment)
template <class T, int V>
__device__ __forceinline__ void load_piece(const T* p, double (&x)[V])
{
    if (V == 1)
        x[0] = (double)p[0];
    else
    {
        typedef T Vec __attribute__((ext_vector_type(V)));
        const Vec v = *reinterpret_cast<const Vec*>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = (double)v[j];
    }
}
template <int V>
__device__ __forceinline__ void load_state(const double* p, double (&x)[V])
{
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = p[j];
}
template <int V>
__device__ __forceinline__ void store_state(double* p, const double (&x)[V])
{
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = x[j];
}

// Used step g of the chunk [g0, g1) of chain kl of this launch is the row base + kl * chain_stride + (g - g0) * step_stride.
// Block (x, y, z): elements [x * 256 * V, ...), the slices of rhat_block_slices(own, slices, y), z = kl * H + h; its state is
// that of (chain, half) z_first + z.
template <class T, int V>
__global__ void __launch_bounds__(kRhatThreads)
rhat_series_kernel(const T* base, long long step_stride, long long chain_stride, long long E, long long n, long long L, int H, long long g0, long long g1,
                   long long slen, int slices, int own, int z_first, double* __restrict__ first, double* __restrict__ state)
{
    const long long e0 = ((long long)blockIdx.x * kRhatThreads + threadIdx.x) * V;
    if (e0 >= E) return;
    const int kl = (int)blockIdx.z / H, h = (int)blockIdx.z % H;
    const long long z = (long long)z_first + blockIdx.z;
    const long long a = mcmcpp::rhat_half_begin(n, L, h);
    if (a + L <= g0 || a >= g1) return;  // nothing of this half in the chunk
    const T* rows = base + (long long)kl * chain_stride + e0;
    const int slots = own ? 2 : slices;
    double* c_at = first + z * E + e0;
    double* st = state + z * slots * 2 * E + e0;  // slot sl: sum d at st + (2 sl) E, sum d*d at st + (2 sl + 1) E

    double c[V], s1[V], s2[V], t1[V], t2[V];
    if (a >= g0)
    {
        load_piece<T, V>(rows + (a - g0) * step_stride, c);
        if (blockIdx.y == 0) store_state<V>(c_at, c);
    }
    else
        load_state<V>(c_at, c);
    int t0, t1_;
    mcmcpp::rhat_block_slices(own, slices, (int)blockIdx.y, &t0, &t1_);
    const bool resumes = own && a < g0;  // totals of the chunks before
#pragma unroll
    for (int j = 0; j < V; ++j) t1[j] = t2[j] = 0.0;
    if (resumes)
    {
        load_state<V>(st, t1);
        load_state<V>(st + E, t2);
    }
    bool open = false;
    for (int t = t0; t < t1_; ++t)
    {
        const mcmcpp::RhatWalk w = mcmcpp::rhat_slice_walk(a, L, slen, t, g0, g1);
        if (w.s >= w.f) continue;
        const int slot = own ? 1 : t;
        if (w.fresh)
        {
#pragma unroll
            for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
        }
        else
        {
            load_state<V>(st + (2LL * slot) * E, s1);
            load_state<V>(st + (2LL * slot + 1) * E, s2);
        }
        const T* row = rows + (w.s - g0) * step_stride;
        long long g = w.s;
        for (; g + kRows <= w.f; g += kRows)
        {
            double x[kRows][V];
#pragma unroll
            for (int u = 0; u < kRows; ++u) load_piece<T, V>(row + u * step_stride, x[u]);
            row += kRows * step_stride;
#pragma unroll
            for (int u = 0; u < kRows; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j)
                {
                    const double d = x[u][j] - c[j];
                    s1[j] = s1[j] + d;
                    s2[j] = s2[j] + d * d;
                }
        }
        for (; g < w.f; ++g, row += step_stride)
        {
            double x[V];
            load_piece<T, V>(row, x);
#pragma unroll
            for (int j = 0; j < V; ++j)
            {
                const double d = x[j] - c[j];
                s1[j] = s1[j] + d;
                s2[j] = s2[j] + d * d;
            }
        }
        if (own && w.closes)
        {
#pragma unroll
            for (int j = 0; j < V; ++j)
            {
                t1[j] = t1[j] + s1[j];
                t2[j] = t2[j] + s2[j];
            }
            open = false;
        }
        else if (own)
            open = true;
        else
        {
            store_state<V>(st + (2LL * slot) * E, s1);
            store_state<V>(st + (2LL * slot + 1) * E, s2);
        }
    }
    if (own)
    {
        store_state<V>(st, t1);
        store_state<V>(st + E, t2);
        if (open)
        {
            store_state<V>(st + 2 * E, s1);
            store_state<V>(st + 3 * E, s2);
        }
    }
}

// Series i of `series` = Z * E (i = z E + e = m P + p): the first `add` of its `slots` slots added in ascending order (the
// slices' sums; or the one total a lane that owned the sequence has made of them), then the sequence's mean and sum of squared
// deviations
__global__ void __launch_bounds__(kRhatThreads)
rhat_sequence_kernel(const double* __restrict__ first, const double* __restrict__ state, long long E, long long series, int slots, int add, double L,
                     double* __restrict__ seq_mean, double* __restrict__ seq_m2)
{
    const long long i = (long long)blockIdx.x * kRhatThreads + threadIdx.x;
    if (i >= series) return;
    const long long z = i / E, e = i % E;
    const double* st = state + z * slots * 2 * E + e;
    double S1 = st[0], S2 = st[E];
    for (int sl = 1; sl < add; ++sl)
    {
        S1 = S1 + st[(2LL * sl) * E];
        S2 = S2 + st[(2LL * sl + 1) * E];
    }
    const double q = S1 / L;
    const double r = S2 - S1 * q;
    seq_mean[i] = first[i] + q;
    seq_m2[i] = r < 0.0 ? 0.0 : r;
}

// Thread (slice j, parameter p) of segment g = blockIdx.y (items [g N, (g + 1) N) of [M][P]) sums its slice in ascending
// order from +0.  Squares == 0: a = sum of seq_mean, b = sum of seq_m2 / Lm1.  Squares == 1: a = sum of (seq_mean - center[p])^2.
// out_a, out_b: [segments][slices][P].
template <int Squares>
__global__ void __launch_bounds__(kRhatThreads)
rhat_slice_sums_kernel(const double* __restrict__ seq_mean, const double* __restrict__ seq_m2, const double* __restrict__ center, int P, long long N,
                       long long slen, int slices, double Lm1, double* __restrict__ out_a, double* __restrict__ out_b)
{
    const long long id = (long long)blockIdx.x * kRhatThreads + threadIdx.x;
    if (id >= (long long)slices * P) return;
    const int j = (int)(id / P), p = (int)(id % P);
    const long long g = blockIdx.y;
    const long long m0 = g * N + (long long)j * slen;
    const long long m1 = g * N + ((j + 1) * slen < N ? (j + 1) * slen : N);
    const double mu = Squares ? center[p] : 0.0;
    double a = 0.0, b = 0.0;
    long long m = m0;
    for (; m + kRows <= m1; m += kRows)
    {
        double x[kRows], y[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u)
        {
            x[u] = seq_mean[(m + u) * P + p];
            y[u] = Squares ? 0.0 : seq_m2[(m + u) * P + p];
        }
#pragma unroll
        for (int u = 0; u < kRows; ++u)
        {
            if (Squares)
            {
                const double e = x[u] - mu;
                a = a + e * e;
            }
            else
            {
                a = a + x[u];
                b = b + y[u] / Lm1;
            }
        }
    }
    for (; m < m1; ++m)
    {
        const double x = seq_mean[m * P + p];
        if (Squares)
        {
            const double e = x - mu;
            a = a + e * e;
        }
        else
        {
            a = a + x;
            b = b + seq_m2[m * P + p] / Lm1;
        }
    }
    out_a[(g * slices + j) * P + p] = a;
    if (!Squares) out_b[(g * slices + j) * P + p] = b;
}

// Thread (segment g, parameter p): the slice sums in ascending order, over `div`.  in, out: [segments][slices][P] -> [segments][P]
__global__ void __launch_bounds__(kRhatThreads)
rhat_slice_join_kernel(const double* __restrict__ in_a, const double* __restrict__ in_b, int P, int segments, int slices, double div, double* __restrict__ out_a,
                       double* __restrict__ out_b)
{
    const int id = blockIdx.x * kRhatThreads + threadIdx.x;
    if (id >= segments * P) return;
    const int g = id / P, p = id % P;
    const double* a = in_a + ((long long)g * slices) * P + p;
    double s = a[0];
    for (int j = 1; j < slices; ++j) s = s + a[(long long)j * P];
    out_a[id] = s / div;
    if (in_b)
    {
        const double* b = in_b + ((long long)g * slices) * P + p;
        double r = b[0];
        for (int j = 1; j < slices; ++j) r = r + b[(long long)j * P];
        out_b[id] = r / div;
    }
}

thread_local std::string g_rhat_error;

using mcmcpp::RhatRequest;
using mcmcpp::RhatOutputs;
using mcmcpp::StepSpan;

template <class T, int V>
void launch_series(const mcmcpp::RhatSeriesPlan& plan, hipStream_t stream, const StepSpan<T>& sp, long long chain_stride, long long E, long long n, long long L,
                   int H, long long g0, int z_first, double* first, double* state)
{
    hipLaunchKernelGGL((rhat_series_kernel<T, V>), dim3(plan.etiles, plan.slice_blocks, plan.zs), dim3(kRhatThreads), 0, stream, sp.base, sp.step_stride, chain_stride,
                       E, n, L, H, g0, g0 + sp.n_steps, plan.slen, plan.slices, plan.own, z_first, first, state);
}

// sum_fixed over the N items of each of G segments of [M][P]: means and within-variances (center == nullptr), or squared
// deviations from center[P]; into out_a, out_b [G][P], over div
int sum_over_sequences(std::string& slot, hipStream_t stream, const double* seq_mean, const double* seq_m2, const double* center, int P, long long N, int G, double Lm1,
                       double div, double* part, size_t part_stride, double* out_a, double* out_b)
{
    const mcmcpp::RhatSumPlan plan = mcmcpp::rhat_sum_plan(N, P, G);
    const auto kernel = center ? rhat_slice_sums_kernel<1> : rhat_slice_sums_kernel<0>;
    hipLaunchKernelGGL(kernel, dim3(plan.blocks, plan.segments), dim3(kRhatThreads), 0, stream, seq_mean, seq_m2, center, P, N, plan.slen, plan.slices, Lm1, part,
                       part + part_stride);
    ANALYSIS_TRY(slot, hipGetLastError());
    hipLaunchKernelGGL(rhat_slice_join_kernel, dim3((unsigned)((G * P + kRhatThreads - 1) / kRhatThreads)), dim3(kRhatThreads), 0, stream, (const double*)part,
                       center ? (const double*)nullptr : (const double*)(part + part_stride), P, G, plan.slices, div, out_a, out_b);
    ANALYSIS_TRY(slot, hipGetLastError());
    return MCMCPP_HIP_OK;
}

template <class T>
int run_state(std::string& slot, const RhatRequest& r, const hipDeviceProp_t& prop, long long n, const mcmcpp::RhatShape& shape, hipStream_t stream, mcmcpp::RhatState& st)
{
    const int K = r.K, P = r.P, H = shape.H;
    const long long E = (long long)r.W * P, L = shape.L, M = shape.M;
    const size_t step_bytes = sizeof(T) * (size_t)E;
    const long long chain_stride_steps = r.chain_stride_steps ? r.chain_stride_steps : r.n_steps;
    mcmcpp::DeviceBuffer<>& d_chunk = st.chunk;
    mcmcpp::DeviceBuffer<double>& d_first = st.first;
    mcmcpp::DeviceBuffer<double>& d_state = st.state;
    mcmcpp::DeviceBuffer<double>& d_seq = st.seq;
    mcmcpp::DeviceBuffer<double>& d_part = st.part;
    mcmcpp::DeviceBuffer<double>& d_res = st.res;
    // a device chain is read in place, all chains in one launch; host chains are uploaded chain by chain, a chunk at a time
    const long long per = r.on_device ? n : mcmcpp::rhat_steps_per_chunk(mcmcpp::chunk_bytes_from_env("MCMCPP_HIP_RHAT_CHUNK_MB", 1024), step_bytes);
    const size_t series = (size_t)M * P;
    if (mcmcpp::grow(d_chunk, r.on_device ? 0 : step_bytes * (size_t)(n < per ? n : per), stream) != hipSuccess)
        return mcmcpp::analysis_fail(slot, MCMCPP_HIP_E_NOMEM, std::string(r.what) + ": cannot allocate the upload buffer");
    const int vec = mcmcpp::rhat_vector_width(sizeof(T), E, r.on_device ? (uintptr_t)r.device_steps : (uintptr_t)d_chunk.get());
    const mcmcpp::RhatSeriesPlan plan = mcmcpp::rhat_series_plan(E, vec, L, r.on_device ? K * H : H, mcmcpp::rhat_plan_cus(prop.multiProcessorCount));
    const size_t part_all = (size_t)mcmcpp::rhat_sum_plan(M, P, 1).slices * P, part_chain = (size_t)K * mcmcpp::rhat_sum_plan((long long)H * r.W, P, K).slices * P;
    const size_t part = part_all > part_chain ? part_all : part_chain;
    const size_t res = 3 * (size_t)P + 2 * (size_t)K * P;  // mean, within, between [P]; chain_mean, chain_within [K][P]
    if (d_first.alloc(8 * series) != hipSuccess || d_state.alloc(8 * series * 2 * plan.slots) != hipSuccess || d_seq.alloc(8 * series * 2) != hipSuccess ||
        d_part.alloc(8 * part * 2) != hipSuccess || d_res.alloc(8 * res) != hipSuccess)
        return mcmcpp::analysis_fail(slot, MCMCPP_HIP_E_NOMEM,
                                     std::string(r.what) + ": cannot allocate the " + std::to_string(8 * series * (3 + 2 * (size_t)plan.slots)) + "-byte state of the sequences");

    constexpr int kPiece = mcmcpp::kRhatVectorBytes / (int)sizeof(T);
    const auto launch = vec == 1 ? launch_series<T, 1> : launch_series<T, kPiece>;
    for (int k = 0; k < (r.on_device ? 1 : K); ++k)
    {
        mcmcpp::StepSource<T> src{r.on_device ? nullptr : r.steps + (size_t)k * n, static_cast<const T*>(r.device_steps), n, r.slice, r.W, P, stream, &d_chunk, &slot};
        long long g0 = 0;
        int rc = src.for_each_chunk(per, [&](const StepSpan<T>& sp) -> int {
            launch(plan, stream, sp, chain_stride_steps * E, E, n, L, H, g0, k * H, d_first.get(), d_state.get());
            ANALYSIS_TRY(slot, hipGetLastError());
            g0 += sp.n_steps;
            return MCMCPP_HIP_OK;
        });
        if (rc) return rc;
    }
    double *seq_mean = d_seq.get(), *seq_m2 = d_seq.get() + series;
    double *mean = d_res.get(), *within = mean + P, *between = within + P, *chain_mean = between + P, *chain_within = chain_mean + (size_t)K * P;
    hipLaunchKernelGGL(rhat_sequence_kernel, dim3((unsigned)((series + kRhatThreads - 1) / kRhatThreads)), dim3(kRhatThreads), 0, stream, (const double*)d_first.get(),
                       (const double*)d_state.get(), E, (long long)series, plan.slots, plan.own ? 1 : plan.slices, (double)L, seq_mean, seq_m2);
    ANALYSIS_TRY(slot, hipGetLastError());
    const double Lm1 = (double)(L - 1);
    if (int rc = sum_over_sequences(slot, stream, seq_mean, seq_m2, nullptr, P, M, 1, Lm1, (double)M, d_part.get(), part, mean, within)) return rc;
    if (int rc = sum_over_sequences(slot, stream, seq_mean, seq_m2, nullptr, P, (long long)H * r.W, K, Lm1, (double)((long long)H * r.W), d_part.get(), part, chain_mean,
                                    chain_within))
        return rc;
    if (int rc = sum_over_sequences(slot, stream, seq_mean, seq_m2, mean, P, M, 1, Lm1, (double)(M - 1), d_part.get(), part, between, nullptr)) return rc;
    st.h_res.resize(res);
    ANALYSIS_TRY(slot, hipMemcpyAsync(st.h_res.data(), d_res, 8 * res, hipMemcpyDeviceToHost, stream));
    return MCMCPP_HIP_OK;
}

int rhat_entry(const RhatRequest& r, const RhatOutputs& out)
{
    long long n = 0;
    mcmcpp::RhatShape shape;
    if (int rc = mcmcpp::rhat_check_request(g_rhat_error, r, &n, &shape)) return rc;
    hipDeviceProp_t prop;
    std::string why;
    int device = r.device;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return mcmcpp::analysis_fail(g_rhat_error, rc, std::string(r.what) + ": " + why);
    if (int rc = mcmcpp::rhat_check_device_steps(g_rhat_error, r, device)) return rc;
    mcmcpp::Stream stream;
    ANALYSIS_TRY(g_rhat_error, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    return mcmcpp::rhat_compute(g_rhat_error, r, prop, n, shape, stream, out);
}
}  // namespace

namespace mcmcpp
{
int rhat_compute(std::string& slot, const RhatRequest& r, const hipDeviceProp_t& prop, long long n, const RhatShape& shape, hipStream_t stream, const RhatOutputs& out)
{
    const int K = r.K, P = r.P;
    const long long L = shape.L, M = shape.M;
    const size_t series = (size_t)M * P;
    RhatState st;
    std::vector<double> h_seq;
    IdleOnReturn idle{stream};  // (behind the buffers: the stream is idle when they go)
    if (int rc = rhat_sequences_state(slot, r, prop, n, shape, stream, st)) return rc;
    const std::vector<double>& h_res = st.h_res;
    if (out.sequence_mean || out.sequence_m2)
    {
        h_seq.resize(2 * series);
        ANALYSIS_TRY(slot, hipMemcpyAsync(h_seq.data(), st.seq, 16 * series, hipMemcpyDeviceToHost, stream));
    }
    ANALYSIS_TRY(slot, hipStreamSynchronize(stream));
    // the call has succeeded: the outputs
    const double Lm1 = (double)(L - 1);
    const double *h_mean = h_res.data(), *h_within = h_mean + P, *h_between = h_within + P;
    if (out.rhat)
        for (int p = 0; p < P; ++p)
        {
            const double varplus = (h_within[p] * Lm1) / (double)L + h_between[p];
            out.rhat[p] = std::sqrt(varplus / h_within[p]);
        }
    if (out.mean) std::memcpy(out.mean, h_mean, 8 * (size_t)P);
    if (out.within) std::memcpy(out.within, h_within, 8 * (size_t)P);
    if (out.between) std::memcpy(out.between, h_between, 8 * (size_t)P);
    if (out.chain_mean) std::memcpy(out.chain_mean, h_between + P, 8 * (size_t)K * P);
    if (out.chain_within) std::memcpy(out.chain_within, h_between + P + (size_t)K * P, 8 * (size_t)K * P);
    if (out.sequence_mean) std::memcpy(out.sequence_mean, h_seq.data(), 8 * series);
    if (out.sequence_m2) std::memcpy(out.sequence_m2, h_seq.data() + series, 8 * series);
    if (out.sequence_length) *out.sequence_length = L;
    if (out.num_sequences) *out.num_sequences = M;
    return MCMCPP_HIP_OK;
}

int rhat_check_request(std::string& slot, const RhatRequest& r, long long* n_out, RhatShape* shape_out)
{
    const std::string w(r.what);
    const auto rhat_fail = [&](int code, const std::string& msg) { return analysis_fail(slot, code, msg); };
    if (r.dtype != MCMCPP_HIP_F64 && r.dtype != MCMCPP_HIP_F32) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": dtype must be MCMCPP_HIP_F64 or MCMCPP_HIP_F32");
    if (r.K < 1 || r.K > mcmcpp::kRhatMaxChains) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": 1 <= num_chains <= " + std::to_string(mcmcpp::kRhatMaxChains));
    if (r.P < 1 || r.P > mcmcpp::kRhatMaxParams) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": 1 <= num_params <= " + std::to_string(mcmcpp::kRhatMaxParams));
    if (r.W < 1) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": num_walkers >= 1");
    if ((long long)r.W * r.P >= (1LL << 31)) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": num_walkers * num_params < 2^31");
    if (r.slice < 1) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": slice_interval >= 1");
    if (r.chain_stride_steps < 0 || (r.chain_stride_steps > 0 && r.chain_stride_steps < r.n_steps))
        return rhat_fail(MCMCPP_HIP_E_ARG, w + ": chain_stride_steps must be 0 (the chains follow each other) or at least n_steps");
    if (r.on_device ? !r.device_steps : !r.steps) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": the steps must not be NULL");
    const long long n = r.n_steps < 1 ? 0 : (r.n_steps + r.slice - 1) / r.slice;
    if (!r.on_device)
        for (int64_t k = 0; k < (int64_t)r.K * n; ++k)
            if (!r.steps[k]) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": a step pointer is NULL");
    const mcmcpp::RhatShape shape = mcmcpp::rhat_shape(r.K, n, r.W, r.split);
    if (shape.L < 2)
        return rhat_fail(MCMCPP_HIP_E_ARG, w + ": a sequence needs two steps (L >= 2): " + std::to_string(n) + " used steps give L = " + std::to_string(shape.L));
    if (shape.M < 2) return rhat_fail(MCMCPP_HIP_E_ARG, w + ": two sequences at the least (M >= 2): one chain of one walker, unsplit, is one");
    *n_out = n;
    *shape_out = shape;
    return MCMCPP_HIP_OK;
}

int rhat_sequences_state(std::string& slot, const RhatRequest& r, const hipDeviceProp_t& prop, long long n, const RhatShape& shape, hipStream_t stream, RhatState& st)
{
    return r.dtype == MCMCPP_HIP_F64 ? run_state<double>(slot, r, prop, n, shape, stream, st) : run_state<float>(slot, r, prop, n, shape, stream, st);
}
}  // namespace mcmcpp

extern "C"
{
const char* mcmcpp_hip_gelman_rubin_last_error(void) { return g_rhat_error.c_str(); }

int mcmcpp_hip_gelman_rubin(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                            int32_t split, double* rhat, double* mean, double* within, double* between, double* chain_mean, double* chain_within,
                            double* sequence_mean, double* sequence_m2, int64_t* sequence_length, int64_t* num_sequences)
{
    return rhat_entry(mcmcpp::rhat_host_request("gelman_rubin", dtype, device, steps, num_chains, n_steps, num_walkers, num_params, split),
                      RhatOutputs{rhat, mean, within, between, chain_mean, chain_within, sequence_mean, sequence_m2, sequence_length, num_sequences});
}

int mcmcpp_hip_gelman_rubin_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains, int64_t chain_stride_steps, int64_t n_steps,
                                   int64_t slice_interval, int32_t num_walkers, int32_t num_params, int32_t split, double* rhat, double* mean, double* within,
                                   double* between, double* chain_mean, double* chain_within, double* sequence_mean, double* sequence_m2,
                                   int64_t* sequence_length, int64_t* num_sequences)
{
    return rhat_entry(mcmcpp::rhat_device_request("gelman_rubin_device", dtype, device, device_steps, num_chains, chain_stride_steps, n_steps, slice_interval, num_walkers,
                                                  num_params, split),
                      RhatOutputs{rhat, mean, within, between, chain_mean, chain_within, sequence_mean, sequence_m2, sequence_length, num_sequences});
}
}
