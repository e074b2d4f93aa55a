// sampler_host.hpp -- the host code the three sampler handles share: the fused stretch move (Sampler, mcmcpp_hip.hip), the
// differential-evolution mover (DeSampler, diffevo.hip) and the stretch move with a batched callback (BatchSampler,
// batch.hip).  A thin base class (device, stream, lane mapping, the recovery rule, read-back) and the plain functions
// behind their init.  Where the movers differ, the difference stays in the mover.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "launch_table.hpp"
#include "run_plan.hpp"
#include "run_refusal.hpp"
#include "sampler_base.hpp"
#include "tie_eps.h"

namespace mcmcpp
{

// t[k] = the map of k steps: t[0] = identity, t[k] = step after t[k-1]
inline std::vector<Affine128> jump_powers(const Affine128& step, size_t count)
{
    std::vector<Affine128> t(count);
    if (count == 0) return t;
    t[0].mult = make_u128(0, 1);
    t[0].plus = make_u128(0, 0);
    for (size_t k = 1; k < count; ++k) t[k] = compose(step, t[k - 1]);
    return t;
}

// The stretch move's jump tables (see JumpTables): lo[k] maps 3k draws, hi[m] 768m draws, and (with_task) task[t] the t + 1
// draws from a half-step's base state to the state behind its draw t
struct StretchJumpTables
{
    std::vector<Affine128> lo, hi, task;
};
inline StretchJumpTables stretch_jump_tables(U128 inc, int n, bool with_task)
{
    StretchJumpTables j;
    j.lo = jump_powers(pcg_jump(inc, 3), 256);
    j.hi = jump_powers(pcg_jump(inc, 768), (size_t)(n + 255) / 256);
    if (with_task)
    {
        j.task = jump_powers(pcg_jump(inc, 1), (size_t)3 * n + 1);
        j.task.erase(j.task.begin());
    }
    return j;
}

// Calculator parameters as the kernels read them: the dense Gaussian's matrix transposed (see DenseGaussianFn) and, with
// `padded`, P^T zero-padded to 32 x 32, which the matrix-core kernels read straight into registers
template <class T>
struct CalcParams
{
    std::vector<T> prm, pad;
};
template <class T>
CalcParams<T> calc_params_host(const mcmcpp_hip_config& c, bool padded)
{
    const int D = c.num_params;
    const T* p = (const T*)c.calc_params;
    CalcParams<T> r;
    r.prm.assign(p, p + c.calc_params_len);
    if (c.calc_id == MCMCPP_HIP_CALC_DENSE_GAUSSIAN)
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) r.prm[(size_t)j * D + i] = p[(size_t)i * D + j];
    if (padded)
    {
        r.pad.assign((size_t)32 * 32, (T)0);
        for (int k = 0; k < D; ++k)
            for (int i = 0; i < D; ++i) r.pad[(size_t)k * 32 + i] = r.prm[(size_t)k * D + i];
    }
    return r;
}

// The near-tie band of the accept test in the element type (tie_eps.h: the oracle reads the same two numbers)
template <class T>
inline T accept_tie_eps()
{
    return sizeof(T) == 8 ? (T)MCMCPP_TIE_EPS_F64 : (T)MCMCPP_TIE_EPS_F32;
}

// The fields of the stretch move's HalfStepArgs that follow from the configuration and the stream alone; the mover fills in
// its buffers, the colour and its launch geometry.  One definition for the fused and the batch path: the same constants
// are what makes their chains the same.
template <class T>
HalfStepArgs<T> stretch_args(const mcmcpp_hip_config& cfg, int vec_ok, U128 inc, const Affine128& half_jump)
{
    const int n = cfg.num_walkers / 2, D = cfg.num_params;
    HalfStepArgs<T> a;
    std::memset(&a, 0, sizeof a);
    a.half_jump = half_jump;
    for (int k = 0; k < 3; ++k) a.draw_jump[k] = pcg_jump(inc, (unsigned)k + 1);
    a.inc = inc;
    a.redraw_threshold = (uint64_t)(0 - (uint64_t)n) % (uint64_t)n;
    // GwDistribution<T,2,1> (MCMCpp/Utility/GwDistribution.h:45-55)
    const T alpha = (T)(cfg.gw_alpha_num > 0 ? cfg.gw_alpha_num : 2) / (T)(cfg.gw_alpha_den > 0 ? cfg.gw_alpha_den : 1);
    const T sqrt_a = std::sqrt(alpha);
    const T inv_sqrt_a = (T)1 / sqrt_a;
    a.gw_term1 = sqrt_a - inv_sqrt_a;
    a.gw_inv_sqrt = inv_sqrt_a;
    a.dims_minus_one = (T)(D - 1);
    a.tie_eps = accept_tie_eps<T>();
    a.n = n;
    a.n_is_pow2 = (n & (n - 1)) == 0;
    a.dims = D;
    a.vec_ok = vec_ok;
    a.direct_save_slot = -1;
    a.use_ctl_save = 1;
    return a;
}

// The run record of a handle that is not inside run(): no chain, no per-step counters, nothing forwarded.  A run starts
// from it and sets what differs.
inline RunInfo idle_run_info()
{
    RunInfo ri = {};
    ri.interval = 1;
    ri.slot_mask = -1;  // (slots are not reused; stage nullptr and slice_bytes 0: no forwarding)
    return ri;
}

// The run record of a run(): the idle one with the device chain (or ring), the per-step counters, the slicing interval and
// the size of a stored step; the caller sets what its path adds (chain_slot_base; stage, slot_mask, slice_bytes).
inline RunInfo run_info_of_run(void* chain, uint32_t* accepted_per_step, int32_t interval, size_t step_bytes)
{
    RunInfo ri = idle_run_info();
    ri.chain = chain;
    ri.accepted_per_step = accepted_per_step;
    ri.interval = interval;
    ri.step_bytes = (int64_t)step_bytes;
    return ri;
}

// S<double> or S<float> by cfg.dtype, then its init; nullptr: out of host memory.  *rc receives the init result, the
// handle carries the message.
template <template <class> class S>
mcmcpp_hip_sampler* make_handle(const mcmcpp_hip_config& cfg, int* rc)
{
    if (cfg.dtype == MCMCPP_HIP_F64)
    {
        S<double>* s = new (std::nothrow) S<double>();
        if (s) *rc = s->init(cfg);
        return s;
    }
    S<float>* s = new (std::nothrow) S<float>();
    if (s) *rc = s->init(cfg);
    return s;
}

// The state and plumbing every sampler handle has, and the one entry of a run.  Each mover keeps the precondition checks of
// its other calls in its own overrides and calls the helpers below from there.
template <class T>
class SamplerHost : public mcmcpp_hip_sampler
{
public:
    int last_run_timing(double* ms, int64_t* launches) override
    {
        if (ms) *ms = last_ms;
        if (launches) *launches = last_launches;
        return MCMCPP_HIP_OK;
    }
    void* device_positions() override { return d_pos; }
    // (a handle of the whole ensemble; sharded handles override it)
    int shard_span(int32_t color, int64_t* off, int64_t* cnt) override
    {
        if (color != 0 && color != 1) return fail(MCMCPP_HIP_E_ARG, "shard_span: colour must be 0 or 1");
        if (off) *off = (int64_t)(color ? n : 0) * D;
        if (cnt) *cnt = (int64_t)n * D;
        return MCMCPP_HIP_OK;
    }
    int synchronize() override
    {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }

    // EnsembleSampler::runMCMC (EnsembleSampler.h:284-310): interval-1 unsaved ensemble steps, one saved, n_saved times;
    // run_device leaves the stored steps in the caller's device memory.  Both are run_entry, for every mover.
    int run(int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step) override
    {
        return run_entry(n_saved, interval, chain_out, accepted_per_step, false);
    }
    int run_device(int64_t n_saved, int32_t interval, void* device_chain, uint32_t* accepted_per_step) override
    {
        return run_entry(n_saved, interval, device_chain, accepted_per_step, true);
    }

protected:
    // ---- what a mover decides about a run: nothing else of run_entry is its business --------------------------------------
    // the ensembles whose stored steps a device destination holds
    virtual int run_chains() const { return 1; }
    // which mover it is and the facts only it knows (run_refusal.hpp); run_entry fills in the rest
    virtual RunFacts run_facts() const = 0;
    // The run itself, behind the checks: n_saved > 0 and the arguments are good -- unless the handle runs collectively
    // (run_is_collective), which hears of its own refusal through refuse_run.  It sets run_touched in front of its first launch.
    virtual int run_mover(int64_t n_saved, int32_t interval, void* chain, uint32_t* accepted_per_step, bool to_device) = 0;
    // the run failed behind its first launch and the walker state has been abandoned
    virtual void state_abandoned() {}

    // the refusal of a run call, if any (run_refusal.hpp), with its message
    int refuse_run(int64_t n_saved, int32_t interval, bool to_device, bool* collective = nullptr)
    {
        RunFacts f = run_facts();
        f.to_device = to_device;
        f.have_state = have_state;
        f.bad_arguments = n_saved < 0 || interval < 1;
        if (collective) *collective = run_is_collective(f);
        const RunRefusal r = run_refusal(f);
        return r == RunRefusal::None ? MCMCPP_HIP_OK : fail(run_refusal_code(r), "%s: %s", to_device ? "run_device" : "run", run_refusal_text(r));
    }

    int run_entry(int64_t n_saved, int32_t interval, void* chain, uint32_t* accepted_per_step, bool to_device)
    {
        run_touched = false;
        bool collective = false;
        const int refused = refuse_run(n_saved, interval, to_device, &collective);
        if (refused && !collective) return refused;
        HIP_TRY(hipSetDevice(device));
        // the destination, asked of the runtime before anything is launched or allocated (nothing to store: NULL is fine)
        if (to_device && n_saved > 0)
            if (int rc = check_device_range("run_device", "device_chain", chain, sizeof(T) * (size_t)W * D * (size_t)n_saved * (size_t)run_chains(), 16)) return rc;
        last_ms = 0.0;
        last_launches = 0;
        if (n_saved == 0 && !collective) return MCMCPP_HIP_OK;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = run_mover(n_saved, interval, chain, accepted_per_step, to_device);
        host_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc != MCMCPP_HIP_OK && run_touched)
        {
            abandon_state();
            state_abandoned();
        }
        return rc;
    }

    // W, D, n and the lane mapping of the kernels: LPW lanes x EPL elements cover the walker's D-vector padded to a power of
    // two (16 bytes per lane until a walker fills a wavefront)
    void set_shape(const mcmcpp_hip_config& c)
    {
        W = c.num_walkers;
        D = c.num_params;
        n = W / 2;
        const LaneMap m = lane_map(D, (int)sizeof(T));
        lpw = m.lpw;
        epl = m.epl;
        vec_ok = m.vec_ok;
    }

    int open_device(const mcmcpp_hip_config& c, hipDeviceProp_t* prop)
    {
        std::string why;
        if (int rc = open_gfx950_device(c.device, &device, prop, &why)) return fail(rc, "%s", why.c_str());
        return MCMCPP_HIP_OK;
    }

    // the caller's stream (MCMCPP_HIP_FLAG_CALLER_STREAM; may be the null, legacy default stream) or one of the handle's own
    int open_stream(const mcmcpp_hip_config& c)
    {
        if (c.flags & MCMCPP_HIP_FLAG_CALLER_STREAM)
            stream = (hipStream_t)c.hip_stream;
        else
        {
            HIP_TRY(hipStreamCreateWithFlags(owned_stream.replace(), hipStreamNonBlocking));
            stream = owned_stream;
            own_stream = true;
        }
        stream_valid = true;
        return MCMCPP_HIP_OK;
    }

    // first thing of a mover's destructor: nothing the handle enqueued is still in flight when its members free themselves
    void quiesce()
    {
        if (device >= 0) (void)hipSetDevice(device);
        if (stream_valid) (void)hipStreamSynchronize(stream);
    }

    // A failure after the first launch of a run leaves walkers, control and draw records ahead of the host's counters (and
    // possibly the stream in capture mode): nothing on the device can be trusted any more, the handle insists on a new
    // set_state.
    void abandon_state()
    {
        const std::string keep = error;
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
        {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(stream, &g);
            if (g) (void)hipGraphDestroy(g);
        }
        (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
        have_state = false;
        error = keep + " (the walker state on the device is no longer consistent: call set_state again)";
    }

    // set_state of one ensemble: positions, log-posteriors, zeroed accepted counters and diagnostics, enqueued on the stream
    int upload_state(const void* pos, const void* logp)
    {
        if (!pos || !logp) return fail(MCMCPP_HIP_E_ARG, "set_state: null pointer");
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemcpyAsync(d_pos, pos, sizeof(T) * (size_t)W * D, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_logp, logp, sizeof(T) * (size_t)W, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_nacc, 0, sizeof(uint32_t) * (size_t)W, stream));
        HIP_TRY(hipMemsetAsync(d_diag, 0, sizeof(Diag), stream));
        steps_since_reset = 0;
        return MCMCPP_HIP_OK;
    }

    // get_state of one ensemble
    int read_state(void* pos, void* logp, uint32_t* n_accept)
    {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
        if (pos) HIP_TRY(hipMemcpy(pos, d_pos, sizeof(T) * (size_t)W * D, hipMemcpyDeviceToHost));
        if (logp) HIP_TRY(hipMemcpy(logp, d_logp, sizeof(T) * (size_t)W, hipMemcpyDeviceToHost));
        if (n_accept) HIP_TRY(hipMemcpy(n_accept, d_nacc, sizeof(uint32_t) * (size_t)W, hipMemcpyDeviceToHost));
        return MCMCPP_HIP_OK;
    }

    // reset_counters of one ensemble
    int clear_accepted()
    {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemsetAsync(d_nacc, 0, sizeof(uint32_t) * (size_t)W, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        steps_since_reset = 0;
        return MCMCPP_HIP_OK;
    }

    // get_counters behind a synchronisation: the accepted counters of one ensemble summed, the step count, the
    // diagnostics record (any pointer may be null)
    int read_counters(uint64_t* accepted, uint64_t* steps, uint64_t* ties, uint64_t* redraws)
    {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
        if (accepted)
        {
            std::vector<uint32_t> a((size_t)W);
            HIP_TRY(hipMemcpy(a.data(), d_nacc, sizeof(uint32_t) * (size_t)W, hipMemcpyDeviceToHost));
            uint64_t s = 0;
            for (uint32_t v : a) s += v;
            *accepted = s;
        }
        if (steps) *steps = steps_since_reset;
        if (ties || redraws)
        {
            Diag d;
            HIP_TRY(hipMemcpy(&d, d_diag, sizeof(Diag), hipMemcpyDeviceToHost));
            if (ties) *ties = d.near_ties;
            if (redraws) *redraws = d.redraws;
        }
        return MCMCPP_HIP_OK;
    }

    // Does [p, p + bytes) lie inside ONE allocation of this handle's device, aligned to `align` bytes?  Asked of the runtime
    // before anything is launched (probe_device_range, sampler_base.hpp): p must be device memory of the device (a host pointer
    // -- pageable, pinned or managed -- is refused here, never dereferenced), and the range must end inside the allocation
    // around p.  MCMCPP_HIP_E_ARG with a message otherwise.
    int check_device_range(const char* what, const char* name, const void* p, size_t bytes, size_t align)
    {
        if (!p) return fail(MCMCPP_HIP_E_ARG, "%s: %s is NULL", what, name);
        if (((uintptr_t)p & (align - 1)) != 0) return fail(MCMCPP_HIP_E_ARG, "%s: %s must be %zu-byte aligned", what, name, align);
        const DeviceRange r = probe_device_range(p, device);
        switch (r.kind)
        {
        case DeviceRange::NotDevice:
            return fail(MCMCPP_HIP_E_ARG, "%s: %s is not device memory (%zu bytes from %p must lie in memory of device %d)", what, name, bytes, p, device);
        case DeviceRange::OtherDevice: return fail(MCMCPP_HIP_E_ARG, "%s: %s is memory of device %d, the handle runs on device %d", what, name, r.device, device);
        case DeviceRange::NoAllocation: return fail(MCMCPP_HIP_E_ARG, "%s: the runtime does not know the allocation %s lies in", what, name);
        case DeviceRange::Found: break;
        }
        if (bytes > r.room) return fail(MCMCPP_HIP_E_ARG, "%s: %s needs %zu bytes, but its allocation ends %zu bytes behind it", what, name, bytes, r.room);
        return MCMCPP_HIP_OK;
    }

    // calc_logp_device by the calculator's own kernel: device rows in, device log-posteriors out, no copies.  Returns when
    // the values are there.
    int kernel_calc_logp_device(typename LaunchTable<T>::CalcFn calc_fn, const T* params, const void* pos, int64_t count, void* out)
    {
        if (count < 0) return fail(MCMCPP_HIP_E_ARG, "calc_logp_device: count must not be negative");
        if (count == 0) return MCMCPP_HIP_OK;
        HIP_TRY(hipSetDevice(device));
        // (rows are read in 16-byte pieces where a row is a whole number of them)
        if (int rc = check_device_range("calc_logp_device", "device_positions", pos, sizeof(T) * (size_t)count * D, vec_ok ? 16 : sizeof(T))) return rc;
        if (int rc = check_device_range("calc_logp_device", "device_logp_out", out, sizeof(T) * (size_t)count, sizeof(T))) return rc;
        const long long per_block = (long long)(64 / lpw) * kWavesPerBlock;
        const unsigned grid = (unsigned)((count + per_block - 1) / per_block);
        calc_fn((const T*)pos, (T*)out, params, count, D, vec_ok, grid, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }

    // mcmcpp_hip_evidence_gaussian behind the mover's own refusals: the handle's shape and its `chains` sets of parameters, then
    // gaussian_bridge.hip
    int gaussian_evidence(GaussianBridgeRequest g, int chains)
    {
        if (g.chain < 0 || g.chain >= chains) return fail(MCMCPP_HIP_E_ARG, "%s: chain %d outside 0..%d", g.q.what, g.chain, chains - 1);
        g.q.dtype = sizeof(T) == 8 ? MCMCPP_HIP_F64 : MCMCPP_HIP_F32;
        g.q.device = device, g.q.K = 1, g.q.W = W, g.q.D = D;
        return gaussian_bridge_compute(*this, g);
    }

    // calc_logp by the calculator's own kernel (`calc` of its launch table)
    int kernel_calc_logp(typename LaunchTable<T>::CalcFn calc_fn, const T* params, const void* pos, int64_t count, void* out)
    {
        if (count < 0 || (count > 0 && (!pos || !out))) return fail(MCMCPP_HIP_E_ARG, "calc_logp: bad arguments");
        if (count == 0) return MCMCPP_HIP_OK;
        HIP_TRY(hipSetDevice(device));
        DeviceBuffer<T> dp, dout;  // (freed on every way out)
        HIP_TRY(dp.alloc(sizeof(T) * (size_t)count * D));
        HIP_TRY(dout.alloc(sizeof(T) * (size_t)count));
        HIP_TRY(hipMemcpyAsync(dp, pos, sizeof(T) * (size_t)count * D, hipMemcpyHostToDevice, stream));
        const long long per_block = (long long)(64 / lpw) * kWavesPerBlock;
        const unsigned grid = (unsigned)((count + per_block - 1) / per_block);
        calc_fn(dp, dout, params, count, D, vec_ok, grid, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, dout, sizeof(T) * (size_t)count, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }

    int W = 0, D = 0, n = 0, lpw = 1, epl = 1, vec_ok = 0, device = -1;
    hipStream_t stream = nullptr;
    Stream owned_stream;  // `stream`, where the handle made it (own_stream); goes with this base, after the mover's members
    bool own_stream = false, stream_valid = false, have_state = false;
    bool run_touched = false;  // the run in hand has launched: a failure from here on leaves the device ahead of the host's bookkeeping
    // the walkers: positions [W][D], log-posteriors [W], accepted counters [W] (the mover allocates them)
    T *d_pos = nullptr, *d_logp = nullptr;
    uint32_t* d_nacc = nullptr;
    Diag* d_diag = nullptr;
    uint64_t steps_since_reset = 0;
    double last_ms = 0.0;
    int64_t last_launches = 0;
};

// The names a mover uses from its dependent base (a class template does not see them without this)
#define MCMCPP_SAMPLER_HOST_NAMES                                                                                               \
    using Host = SamplerHost<T>;                                                                                                \
    using Host::W, Host::D, Host::n, Host::lpw, Host::epl, Host::vec_ok, Host::device, Host::stream, Host::own_stream,        \
        Host::stream_valid, Host::have_state, Host::d_pos, Host::d_logp, Host::d_nacc, Host::d_diag, Host::steps_since_reset, \
        Host::last_ms, Host::last_launches, Host::run_touched;                                                                                   \
    using Host::set_shape, Host::open_device, Host::open_stream, Host::quiesce, Host::abandon_state, Host::read_state,         \
        Host::clear_accepted, Host::read_counters, Host::kernel_calc_logp, Host::kernel_calc_logp_device, Host::check_device_range,   \
        Host::upload_state, Host::refuse_run, Host::gaussian_evidence;                                       \
    using Host::fail, Host::error, Host::publish_stored, Host::host_enqueue_ms, Host::host_wall_ms

}  // namespace mcmcpp
