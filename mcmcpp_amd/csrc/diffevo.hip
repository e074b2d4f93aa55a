// diffevo.hip -- host side of Mover::DifferentialEvolution on gfx950 (reference
// MCMCpp/Movers/DifferentialEvolution.h:80-112 inside EnsembleSampler::performStep, EnsembleSampler.h:342-354).
// See diffevo_kernel.hpp for the scheme: one update launch per half-step; the random stream is planned a batch of half-steps
// at a time (scan, resolve, records) by two launches at every batch boundary; a run is replayed from hipGraphs; the stream
// head, the error flags and the per-run counters travel in device memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "diffevo_planner.hpp"
#include "launch_table.hpp"
#include "sampler_host.hpp"

using namespace mcmcpp;

namespace
{
template <class T>
class DeSampler final : public SamplerHost<T>
{
    MCMCPP_SAMPLER_HOST_NAMES;

public:
    ~DeSampler() override { quiesce(); }

    int init(const mcmcpp_hip_config& c)
    {
        const Knobs knobs = Knobs::from_environment();
        set_shape(c);
        table = static_cast<const LaunchTable<T>*>(launch_table_lookup(c.dtype, c.calc_id));
        if (!table) return fail(MCMCPP_HIP_E_ARG, "calc_id %d has no kernels for this element type", c.calc_id);
        if (table->abi != kLaunchTableAbi || table->elem_size != sizeof(T))
            return fail(MCMCPP_HIP_E_ARG, "calc_id %d: the plug-in was built against other headers (table abi %08x)", c.calc_id, table->abi);
        const int lpw_log = ilog2(lpw), epl_shift = ilog2(epl / Vec16<T>::N);
        if (epl_shift >= kMaxEplShift || !table->de_update[lpw_log][epl_shift])
            return fail(MCMCPP_HIP_E_UNSUPPORTED, "no differential-evolution kernel for D=%d with this calculator (LPW=%d EPL=%d)", D, lpw, epl);
        update_fn = table->de_update[lpw_log][epl_shift];
        walkers_per_block = (64 / lpw) * kWavesPerBlock;
        {
            // the dense Gaussian's product on the matrix cores (de_update_mfma_kernel), where plan_de_update says so
            StepShape s = {};
            s.W = W, s.D = D, s.n = n, s.lpw = lpw, s.elem_size = (int)sizeof(T), s.calc_id = c.calc_id;
            s.de_update_mc = table->de_update_mc[0][lpw_log][epl_shift] != nullptr;
            if (const int per_wave = plan_de_update(s, knobs))
            {
                update_fn = table->de_update_mc[per_wave == 16 ? 1 : 0][lpw_log][epl_shift];
                walkers_per_block = per_wave * kWavesPerBlock;
                matrix_core = true;
            }
        }
        calc_fn = table->calc[lpw_log][epl_shift];

        hipDeviceProp_t prop;
        if (int rc = open_device(c, &prop)) return rc;
        if (int rc = open_stream(c)) return rc;

        // the batch of half-steps the stream is planned by, and every size that follows from it (de_batch_plan.hpp)
        const DeBatchPlan bp = plan_de_batch(n, D, knobs.de_batch.has_value(), knobs.de_batch.value_or(0), knobs.de_scan_run.has_value(), knobs.de_scan_run.value_or(0));
        if (!bp.ok)
            return fail(MCMCPP_HIP_E_UNSUPPORTED, "differential evolution: %d walkers x %d parameters exceed what the stream planner holds (one half-step exceeds %s)", W, D,
                        de_batch_bound_text(bp.bound));
        batch_max = bp.batch_max;

        HIP_TRY(d_own_pos.alloc(sizeof(T) * (size_t)W * D));
        HIP_TRY(d_own_logp.alloc(sizeof(T) * (size_t)W));
        HIP_TRY(d_own_nacc.alloc(sizeof(uint32_t) * (size_t)W));
        HIP_TRY(d_own_diag.alloc(sizeof(Diag)));
        d_pos = d_own_pos;
        d_logp = d_own_logp;
        d_nacc = d_own_nacc;
        d_diag = d_own_diag;
        HIP_TRY(d_recs.alloc(sizeof(DeRec<T>) * (size_t)bp.updates_max));  // the records of the batch being stepped through
        for (int k = 0; k < 2; ++k)
        {
            HIP_TRY(hipEventCreate(ev_t0[k].replace()));
            HIP_TRY(hipEventCreate(ev_t1[k].replace()));
        }
        graph_steps = c.graph_steps == 0 ? 128 : (c.graph_steps > 32768 ? 32768 : c.graph_steps);  // (the step inside a replay travels in 16 bits)
        // HIP cannot capture on the legacy default stream: a caller that hands it over gets plain launches
        if (!own_stream && (stream == nullptr || stream == hipStreamLegacy)) graph_steps = -1;
        replay_steps_max = graph_steps >= 1 ? graph_steps : 16;  // (plain launches: enqueued in groups of this many steps)
        const int per_block = walkers_per_block;
        update_blocks = (n + per_block - 1) / per_block;
        partial_waves = update_blocks * kWavesPerBlock;
        // the run record and, right behind it, the wavefronts' accepted counts of a replay: one allocation (the update kernel
        // reaches both through one preloaded pointer)
        {
            const size_t bytes = sizeof(DeRunInfo) + sizeof(uint32_t) * (size_t)replay_steps_max * 2 * (size_t)partial_waves;
            HIP_TRY(d_run.alloc(bytes));
            HIP_TRY(hipMemset(d_run, 0, bytes));
        }
        HIP_TRY(hipMemset(d_nacc, 0, sizeof(uint32_t) * (size_t)W));
        HIP_TRY(hipMemset(d_diag, 0, sizeof(Diag)));
        if (c.calc_params_len > 0)
        {
            const CalcParams<T> p = calc_params_host<T>(c, matrix_core);
            HIP_TRY(d_params.alloc(sizeof(T) * p.prm.size()));
            HIP_TRY(hipMemcpy(d_params, p.prm.data(), sizeof(T) * p.prm.size(), hipMemcpyHostToDevice));
            if (!p.pad.empty())
            {
                HIP_TRY(d_params_padded.alloc(sizeof(T) * p.pad.size()));
                HIP_TRY(hipMemcpy(d_params_padded, p.pad.data(), sizeof(T) * p.pad.size(), hipMemcpyHostToDevice));
            }
        }

        // the stream (MultiSampler.h:54); the planner's buffers and jump tables
        pcg_seed(c.seed, c.stream, &state0, &inc);
        planner.take(bp, state0, inc);
        HIP_TRY(planner.create());
        gamma = (T)(2.38 / std::sqrt((double)(2 * D)));  // DifferentialEvolution.h:57

        args.calc_params = d_params;
        args.diag = d_diag;
        args.inc = inc;
        args.gamma = gamma;
        args.jitter_width = (T)2.0e-4;  // DifferentialEvolution.h:120-121
        args.jitter_low = (T)-1.0e-4;
        args.tie_eps = accept_tie_eps<T>();
        args.partial_waves = partial_waves;
        return MCMCPP_HIP_OK;
    }

    int set_state(const void* pos, const void* logp) override
    {
        if (int rc = upload_state(pos, logp)) return rc;
        HIP_TRY(planner.rewind(stream));
        HIP_TRY(hipStreamSynchronize(stream));
        half_steps = 0;
        primed = false;
        have_state = true;
        return MCMCPP_HIP_OK;
    }

    RunFacts run_facts() const override
    {
        RunFacts f = {};
        f.mover = Mover::DiffEvo;
        return f;
    }

    // The run, a piece at a time (plan_de_pieces).  A destination in device memory: every piece writes in place (its run
    // record points at the piece's first stored step in the caller's array), so there is no chain buffer of the handle's
    // own and no copy.
    int run_mover(int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step, bool to_device) override
    {
        const int64_t total = n_saved * (int64_t)interval;
        const size_t step_bytes = sizeof(T) * (size_t)W * D;
        const PiecePlan plan = plan_de_pieces(step_bytes, n_saved, interval, chain_out != nullptr, to_device, accepted_per_step != nullptr);
        if (const hipError_t e = grow(d_chain, plan.chain_bytes, stream))
            return fail(MCMCPP_HIP_E_HIP, "hipMalloc of %zu bytes of device chain failed: %s", plan.chain_bytes, hipGetErrorString(e));
        if (const hipError_t e = grow(d_acc, sizeof(uint32_t) * plan.acc_entries, stream))
            return fail(MCMCPP_HIP_E_HIP, "hipMalloc of %zu accepted counters failed: %s", plan.acc_entries, hipGetErrorString(e));

        run_touched = true;
        double gpu_ms = 0.0;
        for (int64_t c = 0; c < plan.n_pieces; ++c)
        {
            const int64_t first = plan.piece(c).from, now = plan.piece(c).to - first;
            {
                DeRunInfo ri;
                std::memset(&ri, 0, sizeof ri);
                ri.chain = !chain_out ? nullptr : to_device ? static_cast<void*>(static_cast<char*>(chain_out) + device_piece_offset(step_bytes, first)) : d_chain.get();
                ri.accepted = accepted_per_step ? d_acc.get() : nullptr;
                ri.interval = (uint32_t)interval;
                HIP_TRY(hipMemcpyAsync(d_run, &ri, sizeof ri, hipMemcpyHostToDevice, stream));
                HIP_TRY(hipStreamSynchronize(stream));  // (the source is on this stack frame)
            }
            HIP_TRY(hipEventRecord(ev_t0[0], stream));
            int rc = enqueue_steps(now * interval);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(ev_t1[0], stream));
            if (chain_out && !to_device)
                HIP_TRY(hipMemcpyAsync(static_cast<char*>(chain_out) + (size_t)first * step_bytes, d_chain, (size_t)now * step_bytes, hipMemcpyDeviceToHost, stream));
            if (accepted_per_step)
                HIP_TRY(hipMemcpyAsync(accepted_per_step + first * interval, d_acc, sizeof(uint32_t) * (size_t)(now * interval), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            {
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, ev_t0[0], ev_t1[0]));
                gpu_ms += ms;
            }
            if (chain_out) publish_stored(first + now);
        }
        steps_since_reset += (uint64_t)total;
        DeHead h;
        HIP_TRY(hipMemcpy(&h, planner.d_head, sizeof h, hipMemcpyDeviceToHost));
        last_ms = gpu_ms;  // GPU time of the launches (planning included) between HIP events on the launch stream (transfers excluded)
        last_launches = 2 * total;
        if (h.error)
            return fail(MCMCPP_HIP_E_UNSUPPORTED,
                        "differential evolution: the random stream could not be followed (flags %u: 1 = more than %d draws thrown away in one "
                        "batch of half-steps, 2 = more bad stream positions or events than the planner's lists hold, 4 = one update threw away more than %d draws)",
                        h.error, kDeShiftMax, kDeWindow - 2);
        return MCMCPP_HIP_OK;
    }

    // Behind a set_state: batch 0 scanned and resolved, batch 1 scanned (see enqueue_replay)
    int prime()
    {
        planner.prime(stream);
        HIP_TRY(hipGetLastError());
        primed = true;
        return MCMCPP_HIP_OK;
    }

    // `steps` ensemble steps (at most replay_steps_max) from half-step h0 (counted from the set_state) on the launch stream:
    // one update launch per half-step; in front of the first half-step of batch b the boundary launch -- the resolve of
    // batch b + 1 (scanned at the boundary before), the records of batch b (resolved at the boundary before) and the scan
    // of batch b + 2.  Behind the steps: the accepted counts and the run record.
    int enqueue_replay(int steps, uint64_t h0)
    {
        typename LaunchTable<T>::DeLaunch l;
        l.pos = d_pos;
        l.logp = d_logp;
        l.n_accept = d_nacc;
        l.jump_small = planner.d_jump_small;
        l.run = d_run;
        l.n = n;
        l.dims = D;
        l.vec_ok = vec_ok;
        l.matrix_padded = d_params_padded;
        for (int i = 0; i < 2 * steps; ++i)
        {
            const uint64_t h = h0 + (uint64_t)i;
            const uint64_t b = h / (uint64_t)batch_max;
            const int j = (int)(h % (uint64_t)batch_max);
            if (j == 0) planner.launch_boundary((long long)b + 1, (long long)b, (long long)b + 2, d_recs, stream);
            l.recs = d_recs + (size_t)j * (size_t)n;
            l.color = (int)(h & 1);
            l.step = i >> 1;
            update_fn(l, args, (unsigned)update_blocks, stream);
        }
        hipLaunchKernelGGL(de_accepted_kernel, dim3((unsigned)steps), dim3(256), 0, stream, d_run, partial_waves);
        hipLaunchKernelGGL(de_advance_kernel, dim3(1), dim3(1), 0, stream, d_run, steps);
        return MCMCPP_HIP_OK;
    }

    // hipGraph of `steps` ensemble steps that start at half-step h0: where the batch boundaries fall, and which of the two
    // batch records a boundary writes, depends on h0 mod two batches
    int graph_for(int steps, uint64_t h0, hipGraphExec_t* out)
    {
        const uint64_t phase = h0 % (2 * (uint64_t)batch_max);
        const uint64_t key = (uint64_t)steps * (2 * (uint64_t)batch_max) + phase;
        auto it = graph_cache.find(key);
        if (it == graph_cache.end())
        {
            if (graph_cache.size() >= 64)
            {
                // (runs of ever-changing lengths: the graphs still queued have been launched, not destroyed under them)
                HIP_TRY(hipStreamSynchronize(stream));
                graph_cache.clear();
            }
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
            int rc = enqueue_replay(steps, phase);
            if (rc) return rc;
            HIP_TRY(hipStreamEndCapture(stream, &g));
            GraphExec ex;
            HIP_TRY(hipGraphInstantiate(ex.replace(), g, nullptr, nullptr, 0));
            HIP_TRY(hipGraphDestroy(g));
            it = graph_cache.emplace(key, std::move(ex)).first;
        }
        *out = it->second;
        return MCMCPP_HIP_OK;
    }

    int enqueue_steps(int64_t steps)
    {
        if (!primed)
        {
            int rc = prime();
            if (rc) return rc;
        }
        int64_t left = steps;
        while (left > 0)
        {
            const int now = (int)(left < replay_steps_max ? left : replay_steps_max);
            if (graph_steps >= 1)
            {
                hipGraphExec_t ex = nullptr;
                int rc = graph_for(now, half_steps, &ex);
                if (rc) return rc;
                HIP_TRY(hipGraphLaunch(ex, stream));
            }
            else
            {
                int rc = enqueue_replay(now, half_steps);
                if (rc) return rc;
            }
            half_steps += 2 * (uint64_t)now;
            left -= now;
        }
        HIP_TRY(hipGetLastError());
        return MCMCPP_HIP_OK;
    }

    // (known inconsistency: unlike the stretch movers, no have_state check -- before set_state this returns OK)
    int get_state(void* pos, void* logp, uint32_t* n_accept) override { return read_state(pos, logp, n_accept); }

    int reset_counters() override { return clear_accepted(); }

    int seek(uint64_t) override
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED, "seek: with the differential-evolution mover the stream position depends on the draws thrown away so far");
    }

    int get_counters(uint64_t* accepted, uint64_t* steps, uint64_t* ties, uint64_t* redraws) override
    {
        if (int rc = read_counters(accepted, steps, ties, nullptr)) return rc;
        if (redraws)
        {
            // every draw thrown away so far (bounded_rand, ind2 == ind1): the stream is planned ahead of the updates, so
            // count from the record of the batch the next half-step belongs to
            *redraws = 0;
            if (primed)
            {
                std::vector<DeBatch> rec(1);
                const uint64_t b = half_steps / (uint64_t)batch_max;
                HIP_TRY(hipMemcpy(rec.data(), planner.d_batch + (b & 1), sizeof(DeBatch), hipMemcpyDeviceToHost));
                const uint64_t done = (half_steps % (uint64_t)batch_max) * (uint64_t)n;  // updates of this batch behind us
                uint64_t shift = 0;
                for (uint32_t e = 0; e < rec[0].events && e < (uint32_t)kDeMaxEvents && (uint64_t)rec[0].plan[e].m < done; ++e) shift = rec[0].plan[e].shift_after;
                *redraws = rec[0].extra_base + shift;
            }
        }
        return MCMCPP_HIP_OK;
    }

    int calc_logp(const void* pos, int64_t count, void* out) override { return kernel_calc_logp(calc_fn, d_params, pos, count, out); }
    // (one ensemble, the create-time parameters: chain 0 only)
    int calc_logp_device(int32_t chain, const void* pos, int64_t count, void* out) override
    {
        if (chain != 0) return fail(MCMCPP_HIP_E_ARG, "calc_logp_device: chain %d, but a differential-evolution handle holds one ensemble (chain 0)", chain);
        return kernel_calc_logp_device(calc_fn, d_params, pos, count, out);
    }
    int evidence_gaussian(GaussianBridgeRequest g) override { return gaussian_evidence(g, 1); }

    int half_step_async(int32_t, int64_t) override { return unsupported("half_step_async"); }
    int bind_device_chain(void*, int64_t) override { return unsupported("bind_device_chain"); }

private:
    int unsupported(const char* what) { return fail(MCMCPP_HIP_E_UNSUPPORTED, "%s: not available with the differential-evolution mover", what); }
    const LaunchTable<T>* table = nullptr;
    typename LaunchTable<T>::DeFn update_fn = nullptr;
    typename LaunchTable<T>::CalcFn calc_fn = nullptr;
    int walkers_per_block = 0;
    // the buffers behind the base's d_pos, d_logp, d_nacc and d_diag
    DeviceBuffer<T> d_own_pos, d_own_logp;
    DeviceBuffer<uint32_t> d_own_nacc;
    DeviceBuffer<Diag> d_own_diag;
    DeviceBuffer<T> d_params, d_params_padded, d_chain;
    bool matrix_core = false;
    DeviceBuffer<uint32_t> d_acc;
    DePlanner<T> planner;  // the stream head, the batch records, the lists and the tables; the boundary launch
    int batch_max = kDeBatchMax;
    DeviceBuffer<DeRec<T>> d_recs;
    DeviceBuffer<DeRunInfo> d_run;
    DeArgs<T> args;
    int update_blocks = 0, partial_waves = 0, graph_steps = 128, replay_steps_max = 128;
    bool primed = false;    // batches 0 and 1 planned behind the last set_state
    Event ev_t0[2], ev_t1[2];
    std::unordered_map<uint64_t, GraphExec> graph_cache;

    U128 state0, inc;
    uint64_t half_steps = 0;
    T gamma = 0;
};
}  // namespace

namespace mcmcpp
{
mcmcpp_hip_sampler* make_de_sampler(const mcmcpp_hip_config& cfg, int* rc) { return make_handle<DeSampler>(cfg, rc); }
}  // namespace mcmcpp
