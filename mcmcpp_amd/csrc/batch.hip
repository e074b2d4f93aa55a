// batch.hip -- StretchMove with a batched log-posterior callback (calc_id MCMCPP_HIP_CALC_BATCH).
//
// The fused half-step kernel (stretch_kernel.hpp) evaluates a device Calculator between forming a proposal and
// accepting it.  A batch target is evaluated by the caller instead -- a GEMM over a dataset, a neural-network density,
// a torch function -- for all W/2 proposals of a half-step at once.  That is exact, not an approximation: every update
// of a half-step reads only the other colour (StretchMove.h:105-113), so the half-step splits into
//   stretch_propose_kernel   record + own row + partner row -> prop[W/2][D]; hand-over; the colour's next draws
//   callback                 prop -> lp_new[W/2] (the caller's work, on the handle's stream)
//   stretch_accept_kernel    the accept test of the fused kernel, row / logp / counter / chain slot / partial counts
// with the same draws, the same operations in the same order, and therefore the same chain as a built-in Calculator that
// computes the same bits.  Plain launches on one stream; the accepted counts of an ensemble step are summed by the
// library's accepted_reduce_kernel behind the black accept.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/mcmcpp_hip.h"
#include "launch_table.hpp"
#include "sampler_host.hpp"

namespace mcmcpp
{

constexpr int kBatchThreads = 256;  // 4 wavefronts; a walker is LPW lanes x EPL elements, as in the fused kernels

// One walker per group of LPW lanes.  Reads the walker's draw record (buffer draw_parity, this colour), its own row and
// its partner's row and writes prop = par + z*(own - par) into row `li` of the dense [n][D] proposal buffer, every
// operation rounded on its own (-ffp-contract=off; the loop above Calc::eval in stretch_half_step_kernel).  One lane of
// the grid hands the stream and the counters to the next launch; the lanes of each walker make the three draws of the
// colour's NEXT update into the other record buffer (the records this launch reads stay untouched: the accept kernel
// reads them again).
template <class T, int EPL, int LPW>
__global__ void __launch_bounds__(kBatchThreads) stretch_propose_kernel(const HalfStepArgs<T> a, T* prop)
{
    const int sub = (int)threadIdx.x & (LPW - 1);
    const int li = (int)blockIdx.x * (kBatchThreads / LPW) + (int)threadIdx.x / LPW;
    const bool active = li < a.n;
    const int lic = active ? li : 0;  // (a valid walker for every lane: nothing below reads out of bounds)
    const int half_base = a.color ? a.n : 0, other_base = a.color ? 0 : a.n;
    const bool vec_ok = a.vec_ok != 0;
    const int i0 = sub * EPL;
    const StepCtl ctl = *a.ctl_in;  // (wave-uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) hand_over<T>(a, ctl, *a.run, a.color, a.ctl_out);

    const DrawRec<T>* recs = a.draws + draw_buffer_index(a.draw_parity, a.color, a.n);
    DrawRec<T>* next = a.draws + draw_buffer_index(1 - a.draw_parity, a.color, a.n);
    const DrawUse<T> rec(recs[lic]);
    T own[EPL], par[EPL];
    load_slice<T, EPL>(a.pos + (size_t)(half_base + lic) * a.dims, i0, a.dims, vec_ok, active, own);
    load_slice<T, EPL>(a.pos + (size_t)(other_base + (int)rec.partner) * a.dims, i0, a.dims, vec_ok, active, par);
    T p[EPL];
    stretch_propose(own, par, rec.z, p);
    if (active) store_slice<T, EPL>(prop + (size_t)li * a.dims, i0, a.dims, vec_ok, p);

    // the draws of this walker's next update (half-step + 2, base state ctl.state2): draw k by lane k of the group
    if (active)
    {
        const bool direct = a.task_jump != nullptr;
        for (int k = sub; k < 3; k += LPW)
        {
            Affine128 j_a, j_b;
            load_draw_jump<T>(a, direct, li, k, j_a, j_b);
            compute_draw<T>(a, ctl.state2, j_a, j_b, direct, k, next + li);
        }
    }
}

// The accept half of stretch_half_step_kernel for the proposals in `prop` and their log-posteriors `lp_new` (the
// callback's output).  It reads the same control record (ctl_in) and the same draw records as the propose launch of this
// half-step: neither is written again before this colour's next update (the propose launch writes ctl_out and the other
// record buffer; the other colour's launches read and write the other control record and the other colour's records).
template <class T, int EPL, int LPW>
__global__ void __launch_bounds__(kBatchThreads) stretch_accept_kernel(const HalfStepArgs<T> a, const T* prop, const T* lp_batch)
{
    const int lane = (int)threadIdx.x & 63;
    const int sub = (int)threadIdx.x & (LPW - 1);
    const int li = (int)blockIdx.x * (kBatchThreads / LPW) + (int)threadIdx.x / LPW;
    const bool active = li < a.n;
    const int lic = active ? li : 0;
    const int w = (a.color ? a.n : 0) + lic;
    const bool vec_ok = a.vec_ok != 0;
    const int i0 = sub * EPL;
    const StepCtl ctl = *a.ctl_in;
    const RunInfo run = *a.run;

    const DrawUse<T> rec(a.draws[draw_buffer_index(a.draw_parity, a.color, a.n) + lic]);
    T own[EPL], p[EPL];
    T* row = a.pos + (size_t)w * a.dims;
    load_slice<T, EPL>(prop + (size_t)lic * a.dims, i0, a.dims, vec_ok, active, p);
    const T lp_new = lp_batch[lic];
    const T lp_old = a.logp[w];
    const uint32_t nacc_old = a.n_accept[w];

    const long long save_slot = stored_step_slot(run, ctl, true, false);  // (a batch run always saves by its control record)
    if (save_slot >= 0) load_slice<T, EPL>(row, i0, a.dims, vec_ok, active, own);

    const bool accept = stretch_accept(a, rec.ln_u, rec.zs, lp_new, lp_old, active && sub == 0) && active;
    if (accept)
    {
        // Walker::jumpToNewPointSwap (Walker/Walker.h:172-179)
        store_slice<T, EPL>(row, i0, a.dims, vec_ok, p);
        if (sub == 0)
        {
            a.logp[w] = lp_new;
            a.n_accept[w] = nacc_old + 1u;
        }
    }
    if (save_slot >= 0 && active)
    {
        // Walker -> Chain::storeWalker (Chain/ChainBlock.h:125-131): cell = slot*W*D + walker*D + p
        T* crow = reinterpret_cast<T*>(run.chain) + ((size_t)save_slot * (size_t)(2 * a.n) + (size_t)w) * a.dims;
        if (accept)
            store_slice<T, EPL>(crow, i0, a.dims, vec_ok, p);
        else
            store_slice<T, EPL>(crow, i0, a.dims, vec_ok, own);
    }
    // per-wavefront accepted count (every wavefront of the grid writes its entry, zero or not)
    const unsigned accepted_here = (unsigned)__popcll(__ballot(accept && sub == 0));
    store_partial<T>(a, run, ctl, a.color, (int)blockIdx.x * (kBatchThreads / 64) + ((int)threadIdx.x >> 6), lane, accepted_here);
}

namespace
{

template <class T>
struct BatchKernels
{
    typedef void (*Fn)(const HalfStepArgs<T>&, T* prop, const T* lp, unsigned grid, hipStream_t);
    Fn propose, accept;
};

template <class T, int EPL, int LPW>
void launch_propose(const HalfStepArgs<T>& a, T* prop, const T*, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((stretch_propose_kernel<T, EPL, LPW>), dim3(grid), dim3(kBatchThreads), 0, st, a, prop);
}
template <class T, int EPL, int LPW>
void launch_accept(const HalfStepArgs<T>& a, T* prop, const T* lp, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((stretch_accept_kernel<T, EPL, LPW>), dim3(grid), dim3(kBatchThreads), 0, st, a, (const T*)prop, lp);
}
template <class T, int EPL, int LPW>
BatchKernels<T> kernels_of()
{
    BatchKernels<T> k;
    k.propose = &launch_propose<T, EPL, LPW>;
    k.accept = &launch_accept<T, EPL, LPW>;
    return k;
}

// the lane mapping of the fused kernels: LPW lanes x EPL elements cover D padded to a power of two (16 bytes per lane
// until a walker fills a wavefront); one instantiation per (T, EPL, LPW) serves every D and every target
template <class T>
bool kernels_for(int lpw, int epl, BatchKernels<T>* out)
{
    constexpr int B = Vec16<T>::N;
    switch (lpw)
    {
    case 1: *out = kernels_of<T, B, 1>(); return epl == B;
    case 2: *out = kernels_of<T, B, 2>(); return epl == B;
    case 4: *out = kernels_of<T, B, 4>(); return epl == B;
    case 8: *out = kernels_of<T, B, 8>(); return epl == B;
    case 16: *out = kernels_of<T, B, 16>(); return epl == B;
    case 32: *out = kernels_of<T, B, 32>(); return epl == B;
    case 64:
        if (epl == B) *out = kernels_of<T, B, 64>();
        else if (epl == 2 * B) *out = kernels_of<T, 2 * B, 64>();
        else if (epl == 4 * B) *out = kernels_of<T, 4 * B, 64>();
        else if (epl == 8 * B) *out = kernels_of<T, 8 * B, 64>();
        else return false;
        return true;
    default: return false;
    }
}

template <class T>
class BatchSampler final : public SamplerHost<T>
{
    MCMCPP_SAMPLER_HOST_NAMES;

public:
    ~BatchSampler() override { quiesce(); }

    int init(const mcmcpp_hip_config& c)
    {
        cfg = c;
        set_shape(c);
        if (!kernels_for<T>(lpw, epl, &kern)) return fail(MCMCPP_HIP_E_UNSUPPORTED, "no batch kernels for D=%d (LPW=%d EPL=%d)", D, lpw, epl);
        grid = (unsigned)(((long)n * lpw + kBatchThreads - 1) / kBatchThreads);
        partial_waves = (int)grid * (kBatchThreads / 64);

        hipDeviceProp_t prop;
        if (int rc = open_device(c, &prop)) return rc;
        if (int rc = open_stream(c)) return rc;
        HIP_TRY(hipEventCreate(ev_t0.replace()));
        HIP_TRY(hipEventCreate(ev_t1.replace()));

        if (c.device_positions)
        {
            if (((uintptr_t)c.device_positions & 15u) != 0) return fail(MCMCPP_HIP_E_ARG, "device_positions must be 16-byte aligned");
            d_pos = (T*)c.device_positions;
        }
        else
        {
            HIP_TRY(d_own_pos.alloc(sizeof(T) * (size_t)W * D));
            d_pos = d_own_pos;
        }
        HIP_TRY(d_own_logp.alloc(sizeof(T) * (size_t)W));
        HIP_TRY(d_own_nacc.alloc(sizeof(uint32_t) * (size_t)W));
        HIP_TRY(d_ctl.alloc(2 * sizeof(StepCtl)));
        HIP_TRY(d_run.alloc(sizeof(RunInfo)));
        HIP_TRY(d_own_diag.alloc(sizeof(Diag)));
        HIP_TRY(d_draws.alloc(sizeof(DrawRec<T>) * draws_count(1, n)));
        HIP_TRY(d_partials.alloc(sizeof(uint32_t) * 2 * (size_t)partial_waves));
        d_logp = d_own_logp;
        d_nacc = d_own_nacc;
        d_diag = d_own_diag;
        HIP_TRY(hipMemset(d_logp, 0, sizeof(T) * (size_t)W));
        HIP_TRY(hipMemset(d_nacc, 0, sizeof(uint32_t) * (size_t)W));
        HIP_TRY(hipMemset(d_ctl, 0, 2 * sizeof(StepCtl)));
        HIP_TRY(hipMemset(d_diag, 0, sizeof(Diag)));
        HIP_TRY(hipMemset(d_draws, 0, sizeof(DrawRec<T>) * draws_count(1, n)));
        HIP_TRY(hipMemset(d_partials, 0, sizeof(uint32_t) * 2 * (size_t)partial_waves));
        HIP_TRY(h_pinned.alloc(sizeof(Pinned)));
        std::memset(h_pinned, 0, sizeof(Pinned));
        h_pinned->run = idle_run_info();
        HIP_TRY(hipMemcpy(d_run, &h_pinned->run, sizeof(RunInfo), hipMemcpyHostToDevice));

        // pcg64 stream (MultiSampler.h:54) and its jump tables, as the fused sampler builds them
        pcg_seed(c.seed, c.stream, &state0, &inc);
        half_jump = pcg_jump(inc, (unsigned __int128)3 * (unsigned)n);
        const Knobs knobs = Knobs::from_environment();
        {
            const StretchJumpTables j = stretch_jump_tables(inc, n, (size_t)3 * n * sizeof(Affine128) <= ((size_t)knobs.task_table_mb << 20));
            HIP_TRY(d_jump_lo.alloc(sizeof(Affine128) * j.lo.size()));
            HIP_TRY(d_jump_hi.alloc(sizeof(Affine128) * j.hi.size()));
            HIP_TRY(hipMemcpy(d_jump_lo, j.lo.data(), sizeof(Affine128) * j.lo.size(), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_jump_hi, j.hi.data(), sizeof(Affine128) * j.hi.size(), hipMemcpyHostToDevice));
            if (!j.task.empty())
            {
                HIP_TRY(d_task_jump.alloc(sizeof(Affine128) * j.task.size()));
                HIP_TRY(hipMemcpy(d_task_jump, j.task.data(), sizeof(Affine128) * j.task.size(), hipMemcpyHostToDevice));
            }
        }
        chain_subchunk_bytes = (size_t)(knobs.chain_subchunk_mb > 0 ? knobs.chain_subchunk_mb : 32) << 20;
        return MCMCPP_HIP_OK;
    }

    int set_batch_calculator(mcmcpp_hip_batch_logp_fn f, void* u, void* dprop, void* dlogp) override
    {
        if (!f) return fail(MCMCPP_HIP_E_ARG, "set_batch_calculator: fn is NULL");
        if ((((uintptr_t)dprop) & 15u) != 0 || (((uintptr_t)dlogp) & 15u) != 0)
            return fail(MCMCPP_HIP_E_ARG, "set_batch_calculator: device_proposals and device_logp must be 16-byte aligned");
        HIP_TRY(hipSetDevice(device));
        if ((!dprop && !d_own_prop) || (!dlogp && !d_own_lp)) HIP_TRY(hipStreamSynchronize(stream));
        if (!dprop && !d_own_prop) HIP_TRY(d_own_prop.alloc(sizeof(T) * (size_t)n * D));
        if (!dlogp && !d_own_lp) HIP_TRY(d_own_lp.alloc(sizeof(T) * (size_t)n));
        fn = f;
        user = u;
        d_prop = dprop ? (T*)dprop : d_own_prop.get();
        d_lp = dlogp ? (T*)dlogp : d_own_lp.get();
        return MCMCPP_HIP_OK;
    }

    int set_state(const void* pos, const void* logp) override
    {
        if (!fn) return fail(MCMCPP_HIP_E_STATE, "set_state: no batch calculator (mcmcpp_hip_set_batch_calculator)");
        if (int rc = upload_state(pos, logp)) return rc;
        half_steps = 0;
        if (int rc = write_ctl()) return rc;
        have_state = true;
        return MCMCPP_HIP_OK;
    }

    int get_state(void* pos, void* logp, uint32_t* n_accept) override
    {
        if (!have_state) return fail(MCMCPP_HIP_E_STATE, "get_state: no walker state (set_state has not been called, or a run failed half way)");
        return read_state(pos, logp, n_accept);
    }

    int seek(uint64_t steps_done) override
    {
        if (!have_state) return fail(MCMCPP_HIP_E_STATE, "seek: set_state has not been called");
        if (steps_done > (~0ULL >> 2)) return fail(MCMCPP_HIP_E_ARG, "seek: step count out of range");
        HIP_TRY(hipSetDevice(device));
        half_steps = 2 * steps_done;
        return write_ctl();
    }

    int reset_counters() override { return clear_accepted(); }

    int get_counters(uint64_t* accepted, uint64_t* steps, uint64_t* ties, uint64_t* redraws) override
    {
        return read_counters(accepted, steps, ties, redraws);
    }

    // the callback on the caller's rows, in chunks of at most W/2 (the proposal buffer's size)
    int calc_logp(const void* pos, int64_t count, void* out) override
    {
        if (!fn) return fail(MCMCPP_HIP_E_STATE, "calc_logp: no batch calculator (mcmcpp_hip_set_batch_calculator)");
        if (count < 0 || (count > 0 && (!pos || !out))) return fail(MCMCPP_HIP_E_ARG, "calc_logp: bad arguments");
        HIP_TRY(hipSetDevice(device));
        // (the proposal buffer may still be read by the last run's work on the stream)
        HIP_TRY(hipStreamSynchronize(stream));
        for (int64_t first = 0; first < count; first += n)
        {
            const int64_t now = count - first < n ? count - first : n;
            HIP_TRY(hipMemcpyAsync(d_prop, (const T*)pos + (size_t)first * D, sizeof(T) * (size_t)now * D, hipMemcpyHostToDevice, stream));
            const int cb = fn(user, d_prop, d_lp, now, D, (void*)stream);
            if (cb != 0)
            {
                (void)hipStreamSynchronize(stream);
                return fail(MCMCPP_HIP_E_CALLBACK, "calc_logp: the batch log-posterior callback returned %d", cb);
            }
            HIP_TRY(hipMemcpyAsync((T*)out + first, d_lp, sizeof(T) * (size_t)now, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        return MCMCPP_HIP_OK;
    }

    // the callback directly on the caller's device rows, in chunks of at most W/2 (what a callback is ever given), writing
    // into the caller's device array: no copies.  A chunk is a whole number of 16-byte pieces of log-posteriors (and so of
    // rows) wherever W/2 allows one, so that the callback sees both pointers 16-byte aligned, as it does in a run
    int calc_logp_device(int32_t chain, const void* pos, int64_t count, void* out) override
    {
        if (!fn) return fail(MCMCPP_HIP_E_STATE, "calc_logp_device: no batch calculator (mcmcpp_hip_set_batch_calculator)");
        if (chain != 0) return fail(MCMCPP_HIP_E_ARG, "calc_logp_device: chain %d, but a batch handle holds one ensemble (chain 0)", chain);
        if (count < 0) return fail(MCMCPP_HIP_E_ARG, "calc_logp_device: count must not be negative");
        if (count == 0) return MCMCPP_HIP_OK;
        HIP_TRY(hipSetDevice(device));
        if (int rc = check_device_range("calc_logp_device", "device_positions", pos, sizeof(T) * (size_t)count * D, 16)) return rc;
        if (int rc = check_device_range("calc_logp_device", "device_logp_out", out, sizeof(T) * (size_t)count, 16)) return rc;
        const int64_t per16 = 16 / (int64_t)sizeof(T);
        const int64_t chunk = n >= per16 ? n - n % per16 : n;  // (W/2 < 4 fp32 walkers: element-aligned chunks, see the header)
        for (int64_t first = 0; first < count; first += chunk)
        {
            const int64_t now = count - first < chunk ? count - first : chunk;
            const int cb = fn(user, (const T*)pos + (size_t)first * D, (T*)out + first, now, D, (void*)stream);
            if (cb != 0)
            {
                (void)hipStreamSynchronize(stream);
                return fail(MCMCPP_HIP_E_CALLBACK, "calc_logp_device: the batch log-posterior callback returned %d", cb);
            }
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }
    // (the callback sees the proposals of the Gaussian where gaussian_bridge.hip made them)
    int evidence_gaussian(GaussianBridgeRequest g) override
    {
        if (!fn) return fail(MCMCPP_HIP_E_STATE, "%s: no batch calculator (mcmcpp_hip_set_batch_calculator)", g.q.what);
        return gaussian_evidence(g, 1);
    }

    int set_chain_params(int32_t, const void*, int32_t) override
    {
        return fail(MCMCPP_HIP_E_ARG, "set_chain_params: the batch target takes no parameters (the callback's user pointer carries them)");
    }
    int calc_logp_chain(int32_t, const void*, int64_t, void*) override
    {
        return fail(MCMCPP_HIP_E_ARG, "calc_logp_chain: the batch target takes no parameters (the callback's user pointer carries them)");
    }

    int half_step_async(int32_t, int64_t) override
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED, "half_step_async: not with a batch target (its half-steps need the host callback; use run)");
    }
    int bind_device_chain(void*, int64_t) override
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED, "bind_device_chain: not with a batch target (it serves half_step_async)");
    }

private:
    struct Pinned  // host records on their way to the device (rewritten only after the stream has been synchronised)
    {
        StepCtl ctl;
        RunInfo run;
    };

    template <class P>
    int ensure(DeviceBuffer<P>& buf, size_t bytes)
    {
        if (grow(buf, bytes, stream)) return fail(MCMCPP_HIP_E_NOMEM, "run: cannot allocate %zu bytes of device memory", bytes);
        return MCMCPP_HIP_OK;
    }

    HalfStepArgs<T> make_args(int color, int parity) const
    {
        HalfStepArgs<T> a = stretch_args<T>(cfg, vec_ok, inc, half_jump);
        a.task_jump = d_task_jump;
        a.jump_hi = d_jump_hi;
        a.jump_lo = d_jump_lo;
        a.diag = d_diag;
        a.color = color;
        a.shard_begin = 0;
        a.shard_count = n;
        a.pos = d_pos;
        a.logp = d_logp;
        a.n_accept = d_nacc;
        a.ctl_in = d_ctl + color;
        a.ctl_out = d_ctl + (1 - color);
        a.run = d_run;
        a.draws = d_draws;
        a.partials = d_partials;
        a.partial_slots = 1;
        a.partial_waves = partial_waves;
        a.passes = 1;
        a.draw_parity = parity;
        a.chains = 1;
        return a;
    }

    // device StepCtl[0] <- {stream position of half-step `half_steps` (even), zeroed run counters}, and the draw records of
    // the coming red and black updates (record buffer (half_steps / 2) & 1)
    int write_ctl()
    {
        const Affine128 j = pcg_jump(inc, (unsigned __int128)3 * (unsigned)n * (unsigned __int128)half_steps);
        StepCtl* c = &h_pinned->ctl;
        HIP_TRY(hipStreamSynchronize(stream));  // (the pinned record may still be on its way from the previous call)
        std::memset(c, 0, sizeof *c);
        c->state = apply(j, state0);
        const U128 state1 = apply(half_jump, c->state);
        c->state2 = apply(half_jump, state1);
        c->half_step = half_steps;
        HIP_TRY(hipMemcpyAsync(d_ctl, c, sizeof(StepCtl), hipMemcpyHostToDevice, stream));
        const int parity = (int)((half_steps >> 1) & 1);
        launch_fill_draws(make_args(0, parity), c->state, nullptr, stream);
        launch_fill_draws(make_args(1, parity), state1, nullptr, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }

    RunFacts run_facts() const override
    {
        RunFacts f = {};
        f.mover = Mover::Batch;
        f.callback_set = fn != nullptr;
        return f;
    }

    // The run, a sub-chunk at a time (plan_batch_pieces): stored steps go to a device buffer of a sub-chunk's slots and from
    // there to chain_out.  A destination in device memory: the run record points at it, the accept launches write every
    // stored step to its final place, the run is one sub-chunk with no chain buffer and no copy.
    int run_mover(int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step, bool to_device) override
    {
        const int64_t total = n_saved * (int64_t)interval;
        const size_t step_bytes = sizeof(T) * (size_t)W * D;
        const PiecePlan plan = plan_batch_pieces(chain_subchunk_bytes, step_bytes, n_saved, interval, chain_out != nullptr, to_device, accepted_per_step != nullptr);
        if (int rc = ensure(d_chain, plan.chain_bytes)) return rc;
        if (int rc = ensure(d_acc, sizeof(uint32_t) * plan.acc_entries)) return rc;
        run_touched = true;  // (whatever fails from here on, write_ctl included, abandons the walker state)
        if (int rc = write_ctl()) return rc;  // step_in_run = 0, stream position from the host-side half-step count
        if (accepted_per_step) HIP_TRY(hipMemsetAsync(d_acc, 0, sizeof(uint32_t) * (size_t)total, stream));
        HIP_TRY(hipEventRecord(ev_t0, stream));
        const auto tp1 = std::chrono::steady_clock::now();
        uint64_t step = half_steps >> 1;  // ensemble steps since set_state: its low bit selects the record buffer
        int64_t done_steps = 0;
        for (int64_t c = 0; c < plan.n_pieces; ++c)
        {
            const int64_t first = plan.piece(c).from, now = plan.piece(c).to - first;
            RunInfo* ri = &h_pinned->run;  // (the stream was synchronised behind the previous sub-chunk)
            *ri = idle_run_info();
            ri->chain = !chain_out ? nullptr : to_device ? chain_out : d_chain.get();  // (a device destination is one sub-chunk: first = 0)
            ri->accepted_per_step = accepted_per_step ? d_acc.get() : nullptr;
            ri->interval = interval;
            ri->chain_slot_base = subchunk_slot_base(first);
            ri->step_bytes = (int64_t)step_bytes;
            HIP_TRY(hipMemcpyAsync(d_run, ri, sizeof(RunInfo), hipMemcpyHostToDevice, stream));
            for (int64_t s = 0; s < now * (int64_t)interval; ++s, ++step)
            {
                const int parity = (int)(step & 1);
                for (int color = 0; color < 2; ++color)
                {
                    const HalfStepArgs<T> a = make_args(color, parity);
                    kern.propose(a, d_prop, d_lp, grid, stream);
                    HIP_TRY(hipGetLastError());
                    const int cb = fn(user, d_prop, d_lp, n, D, (void*)stream);
                    if (cb != 0) return fail(MCMCPP_HIP_E_CALLBACK, "run: the batch log-posterior callback returned %d", cb);
                    kern.accept(a, d_prop, d_lp, grid, stream);
                    HIP_TRY(hipGetLastError());
                }
                // (the black propose launch left the control record of the next step in [0]: step_in_run = steps done)
                if (accepted_per_step) launch_accepted_reduce(d_partials, 1, partial_waves, 1, d_ctl, d_run, stream, 1);
                half_steps += 2;
                steps_since_reset += 1;
                ++done_steps;
            }
            if (chain_out && !to_device)
                HIP_TRY(hipMemcpyAsync((char*)chain_out + step_bytes * (size_t)first, d_chain, step_bytes * (size_t)now, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (chain_out) publish_stored(first + now);
        }
        HIP_TRY(hipEventRecord(ev_t1, stream));
        if (accepted_per_step)
            HIP_TRY(hipMemcpyAsync(accepted_per_step, d_acc, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev_t0, ev_t1));
        last_ms = ms;
        last_launches = 4 * done_steps;
        host_enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp1).count();
        return MCMCPP_HIP_OK;
    }

    mcmcpp_hip_config cfg;
    BatchKernels<T> kern;
    mcmcpp_hip_batch_logp_fn fn = nullptr;
    void* user = nullptr;
    int partial_waves = 0;
    unsigned grid = 1;
    Event ev_t0, ev_t1;
    // the buffers behind the base's d_pos (unless the caller's), d_logp, d_nacc and d_diag
    DeviceBuffer<T> d_own_pos, d_own_logp;
    DeviceBuffer<uint32_t> d_own_nacc;
    DeviceBuffer<Diag> d_own_diag;
    T *d_prop = nullptr, *d_lp = nullptr;
    DeviceBuffer<T> d_own_prop, d_own_lp;
    DeviceBuffer<StepCtl> d_ctl;
    DeviceBuffer<RunInfo> d_run;
    DeviceBuffer<DrawRec<T>> d_draws;  // [2 buffers][2 colours][n]: buffer (ensemble step & 1) holds the records of that step
    DeviceBuffer<uint32_t> d_partials; // [2 colours][partial_waves]
    DeviceBuffer<Affine128> d_jump_lo, d_jump_hi, d_task_jump;
    DeviceBuffer<> d_chain;            // [sub_saved][W][D] stored steps of the sub-chunk in hand
    DeviceBuffer<uint32_t> d_acc;
    size_t chain_subchunk_bytes = 0;
    PinnedBuffer<Pinned> h_pinned;
    U128 state0, inc;
    Affine128 half_jump;
    uint64_t half_steps = 0;
};

}  // namespace

mcmcpp_hip_sampler* make_batch_sampler(const mcmcpp_hip_config& cfg, int* rc) { return make_handle<BatchSampler>(cfg, rc); }

}  // namespace mcmcpp
