// rank.hip -- the normal scores of the draws of every parameter, and the rank-normalised diagnostics of Vehtari, Gelman, Simpson,
// Carpenter and Buerkner (2021) that rest on them: rank-normalised split R-hat (bulk and folded), bulk-ESS and tail-ESS, over
// the sequences of rhat.hip / ess.hip.  An extension: the reference has no such class.
//
// The definition is the header's (include/mcmcpp_hip.h, mcmcpp_hip_normal_scores and mcmcpp_hip_rank_diagnostics).  Ranks are
// integers, found exactly; the score of a rank is normal_score.hpp's, one value in bits on device and host.  The diagnostics are
// the bodies of the existing entry points (rhat_state.hpp: ess_compute of mcmcpp_hip_effective_sample_size_device, rhat_compute
// of mcmcpp_hip_gelman_rubin_device) run on fp64 chains this file builds in device memory, on this call's stream and into this
// family's message slot: their bits, by construction.
//
// The kernels and the Ranker are rank_kernels.hpp's (summary.hip sorts with them too).
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
#include "rank_kernels.hpp"

namespace
{
thread_local std::string g_rank_error;

int rank_fail(int code, const std::string& msg) { return mcmcpp::analysis_fail(g_rank_error, code, msg); }

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

template <class T>
int run_request(const Request& q, int device, const hipDeviceProp_t& prop, long long n, const mcmcpp::RhatShape& shape)
{
    const mcmcpp::RhatRequest& r = q.in;
    const std::string w(r.what);
    const int K = r.K, P = r.P, H = shape.H;
    const long long E = (long long)r.W * P, L = shape.L, HL = (long long)H * L;
    const size_t chain_elems = (size_t)K * HL * E;
    if (int rc = mcmcpp::rhat_check_device_steps(g_rank_error, r, device)) return rc;
    if (r.on_device && !q.diagnostics)  // the scores' buffer of the device form: memory of this device, and large enough
        if (int rc = mcmcpp::check_device_range(g_rank_error, r.what, "scores", q.so.scores, 8 * chain_elems, device,
                                                "the " + std::to_string(8 * chain_elems) + " bytes of the scores do not end inside the allocation around scores"))
            return rc;
    mcmcpp::DeviceBuffer<T> d_up;
    mcmcpp::DeviceBuffer<double> d_chain, d_q;
    mcmcpp::DeviceBuffer<int> d_nan;
    Ranker<T> rk;
    mcmcpp::Stream stream;  // (behind the buffers: the stream is idle and gone when they go)
    ANALYSIS_TRY(g_rank_error, hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
    rk.stream = stream;
    rk.err = &g_rank_error;
    if (int rc = rk.locate_draws(r, n, shape, d_up, d_nan)) return rc;
    const Draws<T>& d = rk.d;
    const unsigned all_blocks = (unsigned)mcmcpp::rank_element_blocks(rk.S, P);  // (rank_entry has checked that it fits)
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

    // the diagnostics: the bodies of the existing entry points on fp64 chains [K][HL][W][P] built here, on this call's stream
    if (d_chain.alloc(8 * chain_elems) != hipSuccess || d_q.alloc(8 * (size_t)P) != hipSuccess)
        return rank_fail(MCMCPP_HIP_E_NOMEM, w + ": cannot allocate the " + std::to_string(8 * chain_elems) + " bytes of the score chain");
    std::vector<double> rhat_rank(P), ess_bulk(P), rhat_folded(P), lower(P), upper(P);
    std::vector<int64_t> closed_bulk(P), closed_lower(P), closed_upper(P);
    const mcmcpp::RhatShape chain_shape = mcmcpp::rhat_shape(K, HL, r.W, r.split);
    const auto chain_request = [&](const char* what) { return mcmcpp::rhat_device_request(what, MCMCPP_HIP_F64, device, d_chain.get(), K, 0, HL, 1, r.W, P, r.split); };
    const auto ess_of_chain = [&](double* ess, int64_t* closed, double* rhat) -> int {
        mcmcpp::EssOutputs out{};
        out.ess = ess;
        out.closed = closed;
        out.rhat = rhat;
        return mcmcpp::nested_result(g_rank_error, r.what,
                                     mcmcpp::ess_compute(g_rank_error, chain_request("effective_sample_size_device"), q.max_lag, 0, prop, HL, chain_shape, stream, out));
    };
    if (int rc = rk.rank_all(false, &quant, d_chain.get())) return rc;
    if (int rc = ess_of_chain(ess_bulk.data(), closed_bulk.data(), rhat_rank.data())) return rc;
    if (int rc = rk.set_fold_center(quant)) return rc;
    if (int rc = rk.rank_all(true, nullptr, d_chain.get())) return rc;
    mcmcpp::RhatOutputs folded{};
    folded.rhat = rhat_folded.data();
    if (int rc = mcmcpp::nested_result(g_rank_error, r.what, mcmcpp::rhat_compute(g_rank_error, chain_request("gelman_rubin_device"), prop, HL, chain_shape, stream, folded)))
        return rc;
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
    if (int rc = rank_check_draw_counts(g_rank_error, w, shape, q.in.P)) return rc;
    if (!q.diagnostics && !q.so.scores) return rank_fail(MCMCPP_HIP_E_ARG, w + ": scores must not be NULL");
    hipDeviceProp_t prop;
    std::string why;
    int device = q.in.device;
    if (int rc = mcmcpp::open_gfx950_device(device, &device, &prop, &why)) return rank_fail(rc, w + ": " + why);
    return q.in.dtype == MCMCPP_HIP_F64 ? run_request<double>(q, device, prop, n, shape) : run_request<float>(q, device, prop, n, shape);
}
}  // namespace

extern "C"
{
const char* mcmcpp_hip_rank_diagnostics_last_error(void) { return g_rank_error.c_str(); }

int mcmcpp_hip_normal_scores(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                             int32_t split, int32_t fold, double* scores, double* median, double* q05, double* q95, int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::rhat_host_request("normal_scores", dtype, device, steps, num_chains, n_steps, num_walkers, num_params, split), false, fold, 0,
                              ScoreOutputs{scores, median, q05, q95, sequence_length, num_sequences}, DiagOutputs{}});
}

int mcmcpp_hip_normal_scores_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains, int64_t chain_stride_steps, int64_t n_steps,
                                    int64_t slice_interval, int32_t num_walkers, int32_t num_params, int32_t split, int32_t fold, double* scores, double* median,
                                    double* q05, double* q95, int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::rhat_device_request("normal_scores_device", dtype, device, device_steps, num_chains, chain_stride_steps, n_steps, slice_interval,
                                                          num_walkers, num_params, split),
                              false, fold, 0, ScoreOutputs{scores, median, q05, q95, sequence_length, num_sequences}, DiagOutputs{}});
}

int mcmcpp_hip_rank_diagnostics(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                                int32_t split, int64_t max_lag, double* rhat, double* rhat_rank, double* rhat_folded, double* ess_bulk, double* ess_tail,
                                double* ess_tail_lower, double* ess_tail_upper, double* median, double* q05, double* q95, int64_t* closed_bulk, int64_t* closed_tail,
                                int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::rhat_host_request("rank_diagnostics", dtype, device, steps, num_chains, n_steps, num_walkers, num_params, split), true, 0, max_lag,
                              ScoreOutputs{},
                              DiagOutputs{rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper, median, q05, q95, closed_bulk, closed_tail,
                                          sequence_length, num_sequences}});
}

int mcmcpp_hip_rank_diagnostics_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains, int64_t chain_stride_steps, int64_t n_steps,
                                       int64_t slice_interval, int32_t num_walkers, int32_t num_params, int32_t split, int64_t max_lag, double* rhat, double* rhat_rank,
                                       double* rhat_folded, double* ess_bulk, double* ess_tail, double* ess_tail_lower, double* ess_tail_upper, double* median,
                                       double* q05, double* q95, int64_t* closed_bulk, int64_t* closed_tail, int64_t* sequence_length, int64_t* num_sequences)
{
    return rank_entry(Request{mcmcpp::rhat_device_request("rank_diagnostics_device", dtype, device, device_steps, num_chains, chain_stride_steps, n_steps, slice_interval,
                                                          num_walkers, num_params, split),
                              true, 0, max_lag, ScoreOutputs{},
                              DiagOutputs{rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper, median, q05, q95, closed_bulk, closed_tail,
                                          sequence_length, num_sequences}});
}
}
