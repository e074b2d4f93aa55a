// summary.hip -- the posterior summary of every parameter: mean, sd, quantiles and a highest-density interval, each with its
// Monte Carlo standard error and effective sample size (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021, section 4), over
// the sequences of rhat.hip / ess.hip and the sort of rank.hip.  An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_posterior_summary).  Every effective sample size is that of
// the existing entry point's body (rhat_state.hpp: ess_compute of mcmcpp_hip_effective_sample_size_device, on this call's stream
// and into this family's message slot) on a chain in device memory: the draws themselves, their squared deviations, or the
// indicators of a quantile.  The order statistics come from rank_kernels.hpp's sort of a tile of parameters (summary_plan.hpp
// has the host's decisions):
//   * summary_square_kernel: thread (draw, parameter): c = (x - mean)(x - mean) in double, at the draw's place of the fp64 chain.
//   * summary_pick_kernel: block = parameter of the tile, thread = one rank: the sorted key at that rank, as a double.  The
//     ranks of the quantiles are the same for every parameter; those of the standard errors are the parameter's own.
//   * summary_hdi_kernel: block (span of window starts, parameter): w_i = x_(i+m) - x_(i), the block's best (w, i) in the order
//     "smaller width that is not NaN, then smaller i": lanes by shuffles, wavefronts through LDS.  The order is total, so the
//     tree of the reduction changes nothing.  summary_hdi_final_kernel: block = parameter: the best of the blocks' partials, and
//     the bounds x_(i), x_(i+m).  No workgroup waits for another: every dependence is a kernel boundary.
// The parameters are sorted once, a tile at a time; the quantiles and the interval are read from that sort.  The ranks of a
// quantile's standard error are known only after the indicator chains of all parameters have been through the ESS call: where
// the parameters fit one tile its sorted keys are still there; where they do not, the sorted keys of every tile are kept in a
// buffer of their own (key bytes x S x P, within MCMCPP_HIP_SUMMARY_KEEP_MB), and where that cannot be had every tile is sorted
// a second time.  The picks read the same sorted keys either way.
#include "rank_kernels.hpp"
#include "summary_plan.hpp"

namespace
{
constexpr unsigned kNoWindow = 0xFFFFFFFFu;

template <class T>
__global__ void __launch_bounds__(kThreads) summary_square_kernel(Draws<T> d, const double* __restrict__ mean, double* __restrict__ out)
{
    const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (long long)d.S * d.P) return;
    const int p = (int)(id % d.P);
    const double e = (double)draw_row(d, (unsigned)(id / d.P))[p] - mean[p];
    out[id] = e * e;
}

// picked [parameter of the tile][n]; ranks [n] for all parameters, or [parameter of the tile][n]
template <class K>
__global__ void summary_pick_kernel(const K* __restrict__ keys, unsigned S, const unsigned* __restrict__ ranks, int n, int per_parameter, double* __restrict__ picked)
{
    if ((int)threadIdx.x >= n) return;
    const unsigned r = ranks[(per_parameter ? (size_t)blockIdx.x * n : 0) + threadIdx.x];
    if (r < S) picked[(size_t)blockIdx.x * n + threadIdx.x] = key_value(keys[(size_t)blockIdx.x * S + r]);
}

// is window (w, i) ahead of (bw, bi)?  kNoWindow: no width that is not NaN yet
__device__ __forceinline__ bool hdi_ahead(double w, unsigned i, double bw, unsigned bi)
{
    if (i == kNoWindow) return false;
    if (bi == kNoWindow) return true;
    return w < bw || (w == bw && i < bi);
}

// the best of the block's (w, i) in thread 0
__device__ __forceinline__ void hdi_block_best(double* w, unsigned* i, double* s_w, unsigned* s_i)
{
#pragma unroll
    for (int off = mcmcpp::kRankWave / 2; off >= 1; off >>= 1)
    {
        const double ow = __shfl_down(*w, off);
        const unsigned oi = __shfl_down(*i, off);
        if (hdi_ahead(ow, oi, *w, *i))
        {
            *w = ow;
            *i = oi;
        }
    }
    const unsigned lane = threadIdx.x % mcmcpp::kRankWave, wave = threadIdx.x / mcmcpp::kRankWave;
    if (lane == 0)
    {
        s_w[wave] = *w;
        s_i[wave] = *i;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int v = 1; v < kWaves; ++v)
            if (hdi_ahead(s_w[v], s_i[v], *w, *i))
            {
                *w = s_w[v];
                *i = s_i[v];
            }
}

// partials [parameter of the tile][blocks]
template <class K>
__global__ void __launch_bounds__(kThreads) summary_hdi_kernel(const K* __restrict__ keys, unsigned S, unsigned m, double* __restrict__ part_w, unsigned* __restrict__ part_i)
{
    __shared__ double s_w[kWaves];
    __shared__ unsigned s_i[kWaves];
    const K* k = keys + (size_t)blockIdx.y * S;
    long long first, count;
    mcmcpp::summary_hdi_block_span((long long)S - m, blockIdx.x, &first, &count);
    double best_w = 0.0;
    unsigned best_i = kNoWindow;
    for (long long at = threadIdx.x; at < count; at += kThreads)
    {
        const unsigned i = (unsigned)(first + at);  // i + m <= S - 1
        const double w = key_value(k[i + m]) - key_value(k[i]);
        if (w == w && hdi_ahead(w, i, best_w, best_i))
        {
            best_w = w;
            best_i = i;
        }
    }
    hdi_block_best(&best_w, &best_i, s_w, s_i);
    if (threadIdx.x == 0)
    {
        part_w[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = best_w;
        part_i[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = best_i;
    }
}

// bounds [parameter of the tile][2]
template <class K>
__global__ void __launch_bounds__(kThreads)
summary_hdi_final_kernel(const K* __restrict__ keys, unsigned S, unsigned m, const double* __restrict__ part_w, const unsigned* __restrict__ part_i, unsigned blocks,
                         double* __restrict__ bounds)
{
    __shared__ double s_w[kWaves];
    __shared__ unsigned s_i[kWaves];
    double best_w = 0.0;
    unsigned best_i = kNoWindow;
    for (unsigned b = threadIdx.x; b < blocks; b += kThreads)
    {
        const double w = part_w[(size_t)blockIdx.x * blocks + b];
        const unsigned i = part_i[(size_t)blockIdx.x * blocks + b];
        if (hdi_ahead(w, i, best_w, best_i))
        {
            best_w = w;
            best_i = i;
        }
    }
    hdi_block_best(&best_w, &best_i, s_w, s_i);
    if (threadIdx.x == 0)
    {
        const K* k = keys + (size_t)blockIdx.x * S;
        const bool found = best_i != kNoWindow && best_i < S - m;
        const double nan = __builtin_nan("");
        bounds[2 * (size_t)blockIdx.x] = found ? key_value(k[best_i]) : nan;
        bounds[2 * (size_t)blockIdx.x + 1] = found ? key_value(k[best_i + m]) : nan;
    }
}

thread_local std::string g_summary_error;

int summary_fail(int code, const std::string& msg) { return mcmcpp::analysis_fail(g_summary_error, code, msg); }

struct SummaryOutputs
{
    double *mean, *sd, *mcse_mean, *ess_mean, *ess_sd, *mcse_sd, *quantile, *ess_quantile, *mcse_quantile;
    int64_t *rank_lower, *rank_upper;
    double *hdi_lower, *hdi_upper;
    int64_t *sequence_length, *num_sequences;
};
struct Request
{
    mcmcpp::RhatRequest in;
    int64_t max_lag;
    const double* probs;
    int32_t n_probs;
    double hdi_prob;
    SummaryOutputs out;
};

template <class T>
int run_request(const Request& q, int device, const hipDeviceProp_t& prop, long long n, const mcmcpp::RhatShape& shape)
{
    typedef typename Ranker<T>::OwnKey Key;
    const mcmcpp::RhatRequest& r = q.in;
    const std::string w(r.what);
    const int K = r.K, P = r.P, Q = q.n_probs;
    const long long E = (long long)r.W * P, L = shape.L, M = shape.M, HL = (long long)shape.H * L, S = M * L;
    const size_t chain_elems = (size_t)K * HL * E;
    if (int rc = mcmcpp::rhat_check_device_steps(g_summary_error, r, device)) return rc;
    mcmcpp::DeviceBuffer<T> d_up;
    mcmcpp::DeviceBuffer<double> d_chain, d_q, d_values, d_bounds, d_part_w;
    mcmcpp::DeviceBuffer<unsigned> d_ranks, d_part_i;
    mcmcpp::DeviceBuffer<Key> d_kept;
    mcmcpp::DeviceBuffer<int> d_nan;
    Ranker<T> rk;
    mcmcpp::Stream stream;  // (behind the buffers: the stream is idle and gone when they go)
    ANALYSIS_TRY(g_summary_error, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    rk.stream = stream;
    rk.err = &g_summary_error;
    if (int rc = rk.locate_draws(r, n, shape, d_up, d_nan)) return rc;
    const Draws<T>& d = rk.d;
    const unsigned all_blocks = (unsigned)mcmcpp::rank_element_blocks(S, P), n32 = (unsigned)S;
    if (d_chain.alloc(8 * chain_elems) != hipSuccess || d_q.alloc(8 * (size_t)P) != hipSuccess)
        return summary_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * chain_elems) + " bytes of the fp64 chain");

    // The ESS call (its body: ess_compute of rhat_state.hpp, on this call's stream) on a chain in device memory: the steps of
    // the sequences [K][HL][W][P], or the device chain of the request where it lies
    const char* const ess_name = "effective_sample_size_device";
    const mcmcpp::RhatShape chain_shape = mcmcpp::rhat_shape(K, HL, r.W, r.split);
    const auto ess_of = [&](const mcmcpp::RhatRequest& chain, long long used, const mcmcpp::RhatShape& sh, double* ess, double* mean, double* within, double* between) -> int {
        mcmcpp::EssOutputs out{};
        out.ess = ess;
        out.mean = mean;
        out.within = within;
        out.between = between;
        return mcmcpp::nested_result(g_summary_error, r.what, mcmcpp::ess_compute(g_summary_error, chain, q.max_lag, 0, prop, used, sh, stream, out));
    };
    const auto ess_of_chain = [&](double* ess, double* mean, double* within, double* between) -> int {
        return ess_of(mcmcpp::rhat_device_request(ess_name, MCMCPP_HIP_F64, device, d_chain.get(), K, 0, HL, 1, r.W, P, r.split), HL, chain_shape, ess, mean, within, between);
    };

    // mean, sd: the ESS call on the draws as they are, where they lie (a float draw converts to double exactly, and the call
    // converts first: its results are those of the fp64 chain of the same draws)
    std::vector<double> mean(P), ess_mean(P), within(P), between(P), sd(P), mcse_mean(P);
    {
        const int rc = r.on_device ? ess_of(mcmcpp::rhat_device_request(ess_name, r.dtype, device, r.device_steps, K, r.chain_stride_steps, r.n_steps, r.slice, r.W, P, r.split),
                                            n, shape, ess_mean.data(), mean.data(), within.data(), between.data())
                                   : ess_of(mcmcpp::rhat_device_request(ess_name, r.dtype, device, d_up.get(), K, 0, HL, 1, r.W, P, r.split), HL, chain_shape, ess_mean.data(),
                                            mean.data(), within.data(), between.data());
        if (rc) return rc;
    }
    for (int p = 0; p < P; ++p)
    {
        sd[p] = std::sqrt(mcmcpp::summary_pooled(L, M, within[p], between[p], S - 1));
        mcse_mean[p] = sd[p] / std::sqrt(ess_mean[p]);
    }

    // ess_sd, mcse_sd: the chain of the squared deviations
    std::vector<double> ess_sd(P), evar(P), within_c(P), between_c(P), mcse_sd(P);
    ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(d_q.get(), mean.data(), 8 * (size_t)P, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(summary_square_kernel<T>, dim3(all_blocks), dim3(kThreads), 0, stream, d, (const double*)d_q.get(), d_chain.get());
    ANALYSIS_TRY(g_summary_error, hipGetLastError());
    if (int rc = ess_of_chain(ess_sd.data(), evar.data(), within_c.data(), between_c.data())) return rc;
    for (int p = 0; p < P; ++p) mcse_sd[p] = std::sqrt(((mcmcpp::summary_pooled(L, M, within_c[p], between_c[p], S) / ess_sd[p]) / evar[p]) / 4.0);

    // the sort: quantiles and the interval
    const bool hdi = q.hdi_prob != 0.0, sorts = hdi || Q > 0;
    const unsigned m = hdi ? (unsigned)mcmcpp::summary_hdi_m(q.hdi_prob, S) : 0u;
    const long long windows = mcmcpp::summary_hdi_windows(S, m);
    const unsigned hdi_blocks = (unsigned)mcmcpp::summary_hdi_blocks(windows);
    std::vector<double> quantile((size_t)P * Q), ess_quantile((size_t)P * Q), mcse_quantile((size_t)P * Q), hdi_lower(P), hdi_upper(P);
    std::vector<int64_t> rank_lower((size_t)P * Q), rank_upper((size_t)P * Q);
    std::vector<mcmcpp::RankQuantile> rq(Q);
    std::vector<unsigned> ranks(2 * (size_t)Q);
    const int picks = 2 * Q;
    if (sorts)
    {
        if (int rc = rk.prepare(8 * (int)sizeof(Key))) return rc;
        const size_t tile = (size_t)rk.tile;
        if (!mcmcpp::summary_grids_fit(windows, rk.tile)) return summary_fail(MCMCPP_HIP_E_ARG, w + ": too many windows for a launch grid");
        if (d_values.alloc(8 * (tile * picks + 1)) != hipSuccess || d_ranks.alloc(4 * (tile * picks + 1)) != hipSuccess || d_bounds.alloc(16 * tile) != hipSuccess ||
            (hdi && (d_part_w.alloc(8 * tile * hdi_blocks) != hipSuccess || d_part_i.alloc(4 * tile * hdi_blocks) != hipSuccess)))
            return summary_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the order statistics");
    }
    const int tiles = sorts ? mcmcpp::rank_tiles(P, rk.tile) : 0;
    // more tiles than one: the sorted keys of every parameter are kept for the ranks of mcse_quantile, where
    // MCMCPP_HIP_SUMMARY_KEEP_MB allows and the device has the memory; otherwise every tile is sorted a second time
    bool kept = false;
    if (tiles > 1 && Q > 0)
    {
        const size_t keep_bytes = mcmcpp::summary_keep_bytes(S, P, 8 * (int)sizeof(Key));
        kept = keep_bytes <= mcmcpp::summary_keep_limit_from_env() && d_kept.alloc(keep_bytes) == hipSuccess;
    }
    std::vector<double> values, bounds;
    for (int i = 0; i < Q; ++i)
    {
        rq[i] = mcmcpp::rank_quantile(q.probs[i], S);
        ranks[2 * i] = (unsigned)rq[i].lo;
        ranks[2 * i + 1] = (unsigned)rq[i].hi;
    }
    if (Q > 0) ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(d_ranks.get(), ranks.data(), 4 * ranks.size(), hipMemcpyHostToDevice, stream));
    for (int t = 0; t < tiles; ++t)
    {
        const int p0 = t * rk.tile, now = P - p0 < rk.tile ? P - p0 : rk.tile;
        if (int rc = rk.template rank_tile<Key, false>(p0, now, nullptr, nullptr)) return rc;
        const Key* keys = rk.template sorted_keys<Key>();
        if (kept) ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(d_kept.get() + (size_t)p0 * S, keys, sizeof(Key) * (size_t)S * now, hipMemcpyDeviceToDevice, stream));
        if (Q > 0)
        {
            hipLaunchKernelGGL(summary_pick_kernel<Key>, dim3(now), dim3(64), 0, stream, keys, n32, (const unsigned*)d_ranks.get(), picks, 0, d_values.get());
            ANALYSIS_TRY(g_summary_error, hipGetLastError());
            values.resize((size_t)now * picks);
            ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(values.data(), d_values.get(), 8 * values.size(), hipMemcpyDeviceToHost, stream));
        }
        if (hdi)
        {
            hipLaunchKernelGGL(summary_hdi_kernel<Key>, dim3(hdi_blocks, now), dim3(kThreads), 0, stream, keys, n32, m, d_part_w.get(), d_part_i.get());
            ANALYSIS_TRY(g_summary_error, hipGetLastError());
            hipLaunchKernelGGL(summary_hdi_final_kernel<Key>, dim3(now), dim3(kThreads), 0, stream, keys, n32, m, (const double*)d_part_w.get(),
                               (const unsigned*)d_part_i.get(), hdi_blocks, d_bounds.get());
            ANALYSIS_TRY(g_summary_error, hipGetLastError());
            bounds.resize(2 * (size_t)now);
            ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(bounds.data(), d_bounds.get(), 8 * bounds.size(), hipMemcpyDeviceToHost, stream));
        }
        ANALYSIS_TRY(g_summary_error, hipStreamSynchronize(stream));
        for (int i = 0; i < now; ++i)
        {
            for (int j = 0; j < Q; ++j)
                quantile[(size_t)(p0 + i) * Q + j] = mcmcpp::rank_quantile_value(values[(size_t)i * picks + 2 * j], values[(size_t)i * picks + 2 * j + 1], rq[j]);
            if (hdi)
            {
                hdi_lower[p0 + i] = bounds[2 * (size_t)i];
                hdi_upper[p0 + i] = bounds[2 * (size_t)i + 1];
            }
        }
    }
    if (sorts)
        if (int rc = rk.check_fault()) return rc;

    // ess_quantile: the ESS call on the indicators of x <= quantile, one probability at a time
    std::vector<double> column(P), ess_column(P);
    for (int j = 0; j < Q; ++j)
    {
        for (int p = 0; p < P; ++p) column[p] = quantile[(size_t)p * Q + j];
        ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(d_q.get(), column.data(), 8 * (size_t)P, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(rank_indicator_kernel<T>, dim3(all_blocks), dim3(kThreads), 0, stream, d, (const double*)d_q.get(), d_chain.get());
        ANALYSIS_TRY(g_summary_error, hipGetLastError());
        if (int rc = ess_of_chain(ess_column.data(), nullptr, nullptr, nullptr)) return rc;
        for (int p = 0; p < P; ++p)
        {
            const size_t at = (size_t)p * Q + j;
            ess_quantile[at] = ess_column[p];
            const mcmcpp::SummaryMcseRanks mr = mcmcpp::summary_mcse_ranks(ess_column[p], q.probs[j], S);
            rank_lower[at] = mr.lower;
            rank_upper[at] = mr.upper;
        }
    }

    // mcse_quantile: the order statistics at the parameter's own ranks
    for (int t = 0; t < tiles && Q > 0; ++t)
    {
        const int p0 = t * rk.tile, now = P - p0 < rk.tile ? P - p0 : rk.tile;
        if (tiles > 1 && !kept)
            if (int rc = rk.template rank_tile<Key, false>(p0, now, nullptr, nullptr)) return rc;
        const Key* keys = kept ? d_kept.get() + (size_t)p0 * S : rk.template sorted_keys<Key>();
        ranks.assign((size_t)now * picks, 0u);
        for (int i = 0; i < now; ++i)
            for (int j = 0; j < Q; ++j)
            {
                const size_t at = (size_t)(p0 + i) * Q + j;
                if (rank_lower[at] < 0) continue;  // (no ess: no standard error; rank 0 is read and not used)
                ranks[(size_t)i * picks + 2 * j] = (unsigned)rank_lower[at];
                ranks[(size_t)i * picks + 2 * j + 1] = (unsigned)rank_upper[at];
            }
        ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(d_ranks.get(), ranks.data(), 4 * ranks.size(), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(summary_pick_kernel<Key>, dim3(now), dim3(64), 0, stream, keys, n32, (const unsigned*)d_ranks.get(), picks, 1,
                           d_values.get());
        ANALYSIS_TRY(g_summary_error, hipGetLastError());
        values.resize((size_t)now * picks);
        ANALYSIS_TRY(g_summary_error, hipMemcpyAsync(values.data(), d_values.get(), 8 * values.size(), hipMemcpyDeviceToHost, stream));
        ANALYSIS_TRY(g_summary_error, hipStreamSynchronize(stream));
        for (int i = 0; i < now; ++i)
            for (int j = 0; j < Q; ++j)
            {
                const size_t at = (size_t)(p0 + i) * Q + j;
                mcse_quantile[at] = rank_lower[at] < 0 ? std::numeric_limits<double>::quiet_NaN() : (values[(size_t)i * picks + 2 * j + 1] - values[(size_t)i * picks + 2 * j]) / 2.0;
            }
    }
    if (tiles > 1 && !kept && Q > 0)
        if (int rc = rk.check_fault()) return rc;

    // the call has succeeded: the outputs
    const SummaryOutputs& o = q.out;
    const auto give = [](double* out, const std::vector<double>& v) {
        if (out && !v.empty()) std::memcpy(out, v.data(), 8 * v.size());
    };
    give(o.mean, mean);
    give(o.sd, sd);
    give(o.mcse_mean, mcse_mean);
    give(o.ess_mean, ess_mean);
    give(o.ess_sd, ess_sd);
    give(o.mcse_sd, mcse_sd);
    give(o.quantile, quantile);
    give(o.ess_quantile, ess_quantile);
    give(o.mcse_quantile, mcse_quantile);
    if (o.rank_lower && Q > 0) std::memcpy(o.rank_lower, rank_lower.data(), 8 * rank_lower.size());
    if (o.rank_upper && Q > 0) std::memcpy(o.rank_upper, rank_upper.data(), 8 * rank_upper.size());
    if (hdi)
    {
        give(o.hdi_lower, hdi_lower);
        give(o.hdi_upper, hdi_upper);
    }
    if (o.sequence_length) *o.sequence_length = L;
    if (o.num_sequences) *o.num_sequences = M;
    return MCMCPP_HIP_OK;
}

int summary_entry(const Request& q)
{
    const std::string w(q.in.what);
    long long n = 0;
    mcmcpp::RhatShape shape;
    if (int rc = mcmcpp::rhat_check_request(g_summary_error, q.in, &n, &shape)) return rc;
    if (q.max_lag < 0) return summary_fail(MCMCPP_HIP_E_ARG, w + ": max_lag >= 0 (0: up to L - 1)");
    if (int rc = rank_check_draw_counts(g_summary_error, w, shape, q.in.P)) return rc;
    std::string why = mcmcpp::summary_check_probs(q.probs, q.n_probs);
    if (why.empty()) why = mcmcpp::summary_check_hdi(q.hdi_prob, shape.M * shape.L);
    if (!why.empty()) return summary_fail(MCMCPP_HIP_E_ARG, w + ": " + why);
    hipDeviceProp_t prop;
    int device = q.in.device;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return summary_fail(rc, w + ": " + why);
    return q.in.dtype == MCMCPP_HIP_F64 ? run_request<double>(q, device, prop, n, shape) : run_request<float>(q, device, prop, n, shape);
}
}  // namespace

extern "C"
{
const char* mcmcpp_hip_posterior_summary_last_error(void) { return g_summary_error.c_str(); }

double mcmcpp_hip_beta_quantile(double p, double a, double b) { return mcmcpp::beta_quantile(p, a, b); }

int mcmcpp_hip_posterior_summary(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                                 int32_t split, int64_t max_lag, const double* probs, int32_t n_probs, double hdi_prob, double* mean, double* sd, double* mcse_mean,
                                 double* ess_mean, double* ess_sd, double* mcse_sd, double* quantile, double* ess_quantile, double* mcse_quantile, int64_t* rank_lower,
                                 int64_t* rank_upper, double* hdi_lower, double* hdi_upper, int64_t* sequence_length, int64_t* num_sequences)
{
    return summary_entry(Request{mcmcpp::rhat_host_request("posterior_summary", dtype, device, steps, num_chains, n_steps, num_walkers, num_params, split), max_lag, probs,
                                 n_probs, hdi_prob,
                                 SummaryOutputs{mean, sd, mcse_mean, ess_mean, ess_sd, mcse_sd, quantile, ess_quantile, mcse_quantile, rank_lower, rank_upper, hdi_lower,
                                                hdi_upper, sequence_length, num_sequences}});
}

int mcmcpp_hip_posterior_summary_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains, int64_t chain_stride_steps, int64_t n_steps,
                                        int64_t slice_interval, int32_t num_walkers, int32_t num_params, int32_t split, int64_t max_lag, const double* probs,
                                        int32_t n_probs, double hdi_prob, double* mean, double* sd, double* mcse_mean, double* ess_mean, double* ess_sd, double* mcse_sd,
                                        double* quantile, double* ess_quantile, double* mcse_quantile, int64_t* rank_lower, int64_t* rank_upper, double* hdi_lower,
                                        double* hdi_upper, int64_t* sequence_length, int64_t* num_sequences)
{
    return summary_entry(Request{mcmcpp::rhat_device_request("posterior_summary_device", dtype, device, device_steps, num_chains, chain_stride_steps, n_steps, slice_interval,
                                                             num_walkers, num_params, split),
                                 max_lag, probs, n_probs, hdi_prob,
                                 SummaryOutputs{mean, sd, mcse_mean, ess_mean, ess_sd, mcse_sd, quantile, ess_quantile, mcse_quantile, rank_lower, rank_upper, hdi_lower,
                                                hdi_upper, sequence_length, num_sequences}});
}
}
