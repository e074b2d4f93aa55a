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

#include "diffevo_plan.hpp"
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

        scan_run = (int)knobs.de_scan_run.value_or(kDeScanRun);
        if (scan_run < 1) scan_run = 1;
        batch_max = (int)knobs.de_batch.value_or(kDeBatchMax);
        // the batch: as many half-steps as the position counters (32 bits), the resolver's lists and a sensible amount of
        // record memory (256 MiB) allow
        const unsigned per = (unsigned)D + 3u;
        {
            long long b = batch_max < 1 ? 1 : (batch_max > kDeBatchMax ? kDeBatchMax : batch_max);
            const long long by_positions = ((1LL << 30) - 2 * (kDeShiftMax + 1)) / ((long long)per * n);
            const long long by_lists = (kDeMaxBad * 5LL / 8 - 2 * (kDeShiftMax + 1) / n) / per;
            const long long by_records = (8LL << 20) / n;
            b = b < by_positions ? b : by_positions;
            b = b < by_lists ? b : by_lists;
            b = b < by_records ? b : by_records;
            if (b < 1)
                return fail(MCMCPP_HIP_E_UNSUPPORTED, "differential evolution: %d walkers x %d parameters exceed what the stream planner holds (per half-step: 2^30 stream "
                            "positions, 8 Mi updates)", W, D);
            batch_max = (int)b;
        }
        const size_t updates_max = (size_t)batch_max * n;
        positions_max = (long long)per * (long long)(updates_max - 1) + 2 * (kDeShiftMax + 1);  // (what a scan looks at)
        // one stream position in n is bad: a batch lists about (D + 3) of them per half-step (and as many again as the
        // kDeShiftMax positions behind its end hold, which matters for tiny ensembles), spread evenly over the lists
        {
            const long long expected = positions_max / n + 1;
            bad_capacity = (int)(4 * ((expected + kDeSegments - 1) / kDeSegments) + 64);
            const long long cap = 2 * expected + 512;
            resolve_capacity = cap > kDeMaxBad ? kDeMaxBad : (int)cap;
        }
        scan_blocks = (int)(((positions_max + scan_run - 1) / scan_run + kDePlanThreads - 1) / kDePlanThreads);

        HIP_TRY(d_own_pos.alloc(sizeof(T) * (size_t)W * D));
        HIP_TRY(d_own_logp.alloc(sizeof(T) * (size_t)W));
        HIP_TRY(d_own_nacc.alloc(sizeof(uint32_t) * (size_t)W));
        HIP_TRY(d_own_diag.alloc(sizeof(Diag)));
        d_pos = d_own_pos;
        d_logp = d_own_logp;
        d_nacc = d_own_nacc;
        d_diag = d_own_diag;
        HIP_TRY(d_counts.alloc(sizeof(uint32_t) * 2 * kDeSegments * kDeCountStride));  // two sets of lists (launch_boundary)
        HIP_TRY(hipMemset(d_counts, 0, sizeof(uint32_t) * 2 * kDeSegments * kDeCountStride));
        HIP_TRY(d_bad.alloc(sizeof(DeBad) * 2 * kDeSegments * (size_t)bad_capacity));
        HIP_TRY(hipMemset(d_bad, 0, sizeof(DeBad) * 2 * kDeSegments * (size_t)bad_capacity));
        HIP_TRY(d_recs.alloc(sizeof(DeRec<T>) * updates_max));  // the records of the batch being stepped through
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
        HIP_TRY(d_head.alloc(sizeof(DeHead)));
        HIP_TRY(d_batch.alloc(sizeof(DeBatch) * 2));  // batch b resolves into record b & 1
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

        // the stream (MultiSampler.h:54) and its jump tables: D + 3 draws per update
        pcg_seed(c.seed, c.stream, &state0, &inc);
        {
            const size_t scan_lanes = ((size_t)positions_max + scan_run - 1) / scan_run;
            const std::vector<Affine128> small = jump_powers(pcg_jump(inc, 1), (size_t)kDeShiftMax + (size_t)D + 2);
            const std::vector<Affine128> lo = jump_powers(pcg_jump(inc, per), 256);
            const std::vector<Affine128> hi = jump_powers(pcg_jump(inc, (unsigned __int128)per * 256u), (updates_max + 255) / 256);
            const std::vector<Affine128> slo = jump_powers(pcg_jump(inc, (unsigned)scan_run), 256);
            const std::vector<Affine128> shi = jump_powers(pcg_jump(inc, (unsigned __int128)scan_run * 256u), (scan_lanes + 255) / 256);
            std::vector<Affine128> all;  // one allocation
            all.insert(all.end(), small.begin(), small.end());
            all.insert(all.end(), slo.begin(), slo.end());
            all.insert(all.end(), lo.begin(), lo.end());
            all.insert(all.end(), hi.begin(), hi.end());
            all.insert(all.end(), shi.begin(), shi.end());
            HIP_TRY(d_tables.alloc(sizeof(Affine128) * all.size()));
            HIP_TRY(hipMemcpy(d_tables, all.data(), sizeof(Affine128) * all.size(), hipMemcpyHostToDevice));
            d_jump_small = d_tables;
            d_scan_lo = d_jump_small + small.size();
            d_jump_lo = d_scan_lo + slo.size();
            d_jump_hi = d_jump_lo + lo.size();
            d_scan_hi = d_jump_hi + hi.size();
        }
        batch_jump = pcg_jump(inc, (unsigned __int128)per * (unsigned)n * (unsigned)batch_max);
        threshold = (uint64_t)(0 - (uint64_t)n) % (uint64_t)n;
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
        DeHead h;
        std::memset(&h, 0, sizeof h);
        h.state = state0;
        h.provisional[0] = state0;  // (batches 0 and 1 are scanned before anything has been resolved)
        h.provisional[1] = apply(batch_jump, state0);
        HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * 2 * kDeSegments * kDeCountStride, stream));
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
        HIP_TRY(hipMemcpy(&h, d_head, sizeof h, hipMemcpyDeviceToHost));
        last_ms = gpu_ms;  // GPU time of the launches (planning included) between HIP events on the launch stream (transfers excluded)
        last_launches = 2 * total;
        if (h.error)
            return fail(MCMCPP_HIP_E_UNSUPPORTED,
                        "differential evolution: the random stream could not be followed (flags %u: 1 = more than %d draws thrown away in one "
                        "batch of half-steps, 2 = more bad stream positions or events than the planner's lists hold, 4 = one update threw away more than %d draws)",
                        h.error, kDeShiftMax, kDeWindow - 2);
        return MCMCPP_HIP_OK;
    }

    // The boundary launch in front of a batch: the resolve of batch `resolve_batch` (scanned before), the records of batch
    // `record_batch` (resolved before) and the scan of batch `scan_batch`; any of them < 0: not in this launch (priming).
    void launch_boundary(long long resolve_batch, long long record_batch, long long scan_batch)
    {
        const unsigned per = (unsigned)D + 3u;
        DePlanArgs p;
        std::memset(&p, 0, sizeof p);
        p.head = d_head;
        p.scan_hi = d_scan_hi;
        p.scan_lo = d_scan_lo;
        p.jump_hi = d_jump_hi;
        p.jump_lo = d_jump_lo;
        p.jump_small = d_jump_small;
        p.batch_jump = batch_jump;
        p.inc = inc;
        p.threshold = threshold;
        p.n = n;
        p.dims = D;
        p.updates = n * batch_max;
        p.positions = (int)((long long)per * (long long)(p.updates - 1) + kDeShiftMax + 1);
        p.scan_positions = p.positions + kDeShiftMax + 1;
        p.scan_run = scan_run;
        p.seg_len = (p.scan_positions + kDeSegments - 1) / kDeSegments;
        p.bad_capacity = bad_capacity;
        // two sets of lists: batch b is scanned into set b & 1 (its resolve runs beside the scan of batch b + 1)
        const long long sb = scan_batch >= 0 ? scan_batch : resolve_batch + 1;
        p.scan_parity = (int)(sb & 1);
        p.bad = d_bad + (size_t)(sb & 1) * kDeSegments * (size_t)bad_capacity;
        p.counts = d_counts + (size_t)(sb & 1) * kDeSegments * kDeCountStride;
        p.resolve_bad = d_bad + (size_t)((sb + 1) & 1) * kDeSegments * (size_t)bad_capacity;
        p.resolve_counts = d_counts + (size_t)((sb + 1) & 1) * kDeSegments * kDeCountStride;
        p.batch = d_batch + (resolve_batch >= 0 ? (resolve_batch & 1) : 0);
        const int resolve = resolve_batch >= 0 ? 1 : 0;
        const int record_blocks = record_batch >= 0 ? (p.updates + kDePlanThreads - 1) / kDePlanThreads : 0;
        const int scan_now = scan_batch >= 0 ? scan_blocks : 0;
        size_t lds = record_blocks ? sizeof(DePlan) * kDeMaxEvents : 0;
        const size_t need = resolve ? de_resolve_lds_bytes(resolve_capacity, D + 3) : 0;
        lds = need > lds ? need : lds;
        hipLaunchKernelGGL((de_boundary_kernel<T>), dim3((unsigned)(resolve + record_blocks + scan_now)), dim3(kDePlanThreads), lds, stream, p, resolve, resolve_capacity,
                           record_blocks, d_batch + (record_batch >= 0 ? (record_batch & 1) : 0), d_recs);
    }

    // Behind a set_state: batch 0 scanned and resolved, batch 1 scanned -- what the boundary in front of a batch finds
    // (see enqueue_replay).
    int prime()
    {
        launch_boundary(-1, -1, 0);
        launch_boundary(0, -1, 1);
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
        l.jump_small = d_jump_small;
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
            if (j == 0) launch_boundary((long long)b + 1, (long long)b, (long long)b + 2);
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
                HIP_TRY(hipMemcpy(rec.data(), d_batch + (b & 1), sizeof(DeBatch), hipMemcpyDeviceToHost));
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
    DeviceBuffer<DeHead> d_head;
    DeviceBuffer<DeBatch> d_batch;
    DeviceBuffer<Affine128> d_tables;  // jump_small, scan_lo, jump_lo, jump_hi, scan_hi
    DeviceBuffer<uint32_t> d_counts;
    DeviceBuffer<DeBad> d_bad;
    Affine128 *d_scan_lo = nullptr, *d_scan_hi = nullptr;
    int bad_capacity = 0, scan_run = kDeScanRun, batch_max = kDeBatchMax;
    long long positions_max = 0;
    DeviceBuffer<DeRec<T>> d_recs;
    DeviceBuffer<DeRunInfo> d_run;
    DeArgs<T> args;
    int update_blocks = 0, partial_waves = 0, graph_steps = 128, replay_steps_max = 128;
    int resolve_capacity = 0, scan_blocks = 0;
    bool primed = false;    // batches 0 and 1 planned behind the last set_state
    Affine128 batch_jump;   // (D+3) * n * batch_max draws
    Event ev_t0[2], ev_t1[2];
    std::unordered_map<uint64_t, GraphExec> graph_cache;

    Affine128 *d_jump_lo = nullptr, *d_jump_hi = nullptr, *d_jump_small = nullptr;
    U128 state0, inc;
    uint64_t threshold = 0, half_steps = 0;
    T gamma = 0;
};
}  // namespace

namespace mcmcpp
{
mcmcpp_hip_sampler* make_de_sampler(const mcmcpp_hip_config& cfg, int* rc) { return make_handle<DeSampler>(cfg, rc); }
}  // namespace mcmcpp
