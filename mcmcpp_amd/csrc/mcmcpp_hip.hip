// mcmcpp_hip.hip -- host side of libmcmcpp_hip.so: the C ABI of include/mcmcpp_hip.h on top of the
// gfx950 kernels in stretch_kernel.hpp.
//
// Reference roles replaced (paths relative to /root/reference):
//   EnsembleSampler ctor / setInitialWalkerPos / runMCMC / reset / counters  MCMCpp/EnsembleSampler.h:199-360
//   ParallelEnsembleSampler's thread pool + red/black controller             MCMCpp/Threading/*.h
//     -> one kernel launch per ensemble step (small ensembles: full_step_kernel.hpp) or per half-step (large ones)
//        on one HIP stream, replayed from a hipGraph; the stream and step counters travel in device memory
//        (StepCtl) so a replay needs no host-side updates
//   Walker[] (heap row per walker)  MCMCpp/Walker/Walker.h:142-149 -> pos[W][D], logp[W], n_accept[W] in HBM
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mcmcpp_hip.h"
#define MCMCPP_DEFINE_REDUCE_KERNEL
#include "launch_table.hpp"
#include "replica_round.hpp"
#include "sampler_host.hpp"
#include "split_exchange.hpp"
#include "temper_plan.hpp"

using namespace mcmcpp;

namespace
{
thread_local std::string g_create_error;

// memcpy of a large block split over a few threads (the un-overlapped tail of a run's chain download: a single core
// moves ~12 GB/s into pageable memory)
void parallel_memcpy(char* dst, const char* src, size_t bytes)
{
    const size_t kMinPiece = 512u << 10;
    int pieces = (int)(bytes / kMinPiece);
    if (pieces > 4) pieces = 4;
    if (pieces < 2)
    {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t piece = ((bytes / (size_t)pieces) + 63) & ~(size_t)63;
    std::thread helpers[3];
    for (int k = 1; k < pieces; ++k)
    {
        const size_t off = piece * (size_t)k;
        const size_t len = (k == pieces - 1) ? bytes - off : piece;
        helpers[k - 1] = std::thread([=]() { std::memcpy(dst + off, src + off, len); });
    }
    std::memcpy(dst, src, piece);
    for (int k = 1; k < pieces; ++k) helpers[k - 1].join();
}

struct RegisteredCalc
{
    const void* f64;
    const void* f32;
    int params_len;
};
std::mutex g_registry_mutex;
std::map<int, RegisteredCalc> g_registry;

bool registered_calc(int calc_id, RegisteredCalc* out)
{
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    std::map<int, RegisteredCalc>::const_iterator it = g_registry.find(calc_id);
    if (it == g_registry.end()) return false;
    if (out) *out = it->second;
    return true;
}

template <class T>
const LaunchTable<T>* table_for(int calc_id);
template <>
const LaunchTable<double>* table_for<double>(int calc_id)
{
    switch (calc_id)
    {
    case MCMCPP_HIP_CALC_ISO_GAUSSIAN: return launch_table_f64_iso();
    case MCMCPP_HIP_CALC_DENSE_GAUSSIAN: return launch_table_f64_dense();
    case MCMCPP_HIP_CALC_ROSENBROCK: return launch_table_f64_rosenbrock();
    case MCMCPP_HIP_CALC_SKEWED_GAUSSIAN_2D: return launch_table_f64_skewed();
    default:
    {
        RegisteredCalc r;
        return registered_calc(calc_id, &r) ? static_cast<const LaunchTable<double>*>(r.f64) : nullptr;
    }
    }
}
template <>
const LaunchTable<float>* table_for<float>(int calc_id)
{
    switch (calc_id)
    {
    case MCMCPP_HIP_CALC_ISO_GAUSSIAN: return launch_table_f32_iso();
    case MCMCPP_HIP_CALC_DENSE_GAUSSIAN: return launch_table_f32_dense();
    case MCMCPP_HIP_CALC_ROSENBROCK: return launch_table_f32_rosenbrock();
    case MCMCPP_HIP_CALC_SKEWED_GAUSSIAN_2D: return launch_table_f32_skewed();
    default:
    {
        RegisteredCalc r;
        return registered_calc(calc_id, &r) ? static_cast<const LaunchTable<float>*>(r.f32) : nullptr;
    }
    }
}
}  // namespace

namespace mcmcpp
{
const void* launch_table_lookup(int dtype, int calc_id)
{
    return dtype == MCMCPP_HIP_F64 ? static_cast<const void*>(table_for<double>(calc_id)) : static_cast<const void*>(table_for<float>(calc_id));
}
void launch_fill_draws(const HalfStepArgs<double>& a, U128 base, const U128* red_base, hipStream_t stream)
{
    const unsigned grid = (unsigned)((3 * (long)a.shard_count + 255) / 256);
    hipLaunchKernelGGL(fill_draws_kernel<double>, dim3(grid), dim3(256), 0, stream, a, base, red_base ? *red_base : base, red_base ? 1 : 0);
}
void launch_fill_draws(const HalfStepArgs<float>& a, U128 base, const U128* red_base, hipStream_t stream)
{
    const unsigned grid = (unsigned)((3 * (long)a.shard_count + 255) / 256);
    hipLaunchKernelGGL(fill_draws_kernel<float>, dim3(grid), dim3(256), 0, stream, a, base, red_base ? *red_base : base, red_base ? 1 : 0);
}
void launch_fill_draws_batch(const HalfStepArgs<double>& a, const StepCtl* ctl, const Affine128* step_jump, DrawRec<double>* out, int steps, hipStream_t stream)
{
    const unsigned grid = (unsigned)((a.shard_count + 63) / 64);
    hipLaunchKernelGGL(fill_draws_batch_kernel<double>, dim3(grid, (unsigned)(2 * steps)), dim3(192), 0, stream, a, ctl, step_jump, out);
}
void launch_fill_draws_batch(const HalfStepArgs<float>& a, const StepCtl* ctl, const Affine128* step_jump, DrawRec<float>* out, int steps, hipStream_t stream)
{
    const unsigned grid = (unsigned)((a.shard_count + 63) / 64);
    hipLaunchKernelGGL(fill_draws_batch_kernel<float>, dim3(grid, (unsigned)(2 * steps)), dim3(192), 0, stream, a, ctl, step_jump, out);
}
void launch_accepted_reduce(const uint32_t* partials, int partial_slots, int partial_waves, int count,
                            const StepCtl* ctl_after, const RunInfo* run, hipStream_t stream, int chains)
{
    hipLaunchKernelGGL(accepted_reduce_kernel, dim3((unsigned)count, (unsigned)(chains > 1 ? chains : 1)), dim3(256), 0, stream, partials, partial_slots,
                       partial_waves, count, ctl_after, run);
}
}  // namespace mcmcpp

namespace
{
// The host's pinned scratch of one handle: records on their way to the device.  The host rewrites a slot only once the
// asynchronous copies that read it have been ordered (synchronised, or in the case of the run records four sub-chunks of
// launches later: the sub-chunk loop rotates over them).
struct PinnedScratch
{
    alignas(64) StepCtl ctl;                        // write_ctl, one chain
    alignas(64) RunInfo run[4];                     // one chain: a run's sub-chunks in turn (the split path uses [0])
    alignas(64) StepCtl chain_ctl[kMaxChains];      // write_ctl, several chains
    alignas(64) RunInfo chain_run[4][kMaxChains];   // several chains: [sub-chunk % 4][chain] (the trickle path uses [0], also for one chain)
};
static_assert(sizeof(StepCtl) <= 64 && sizeof(RunInfo) <= 64, "a control or run record is uploaded as one 64-byte line");

int check_config(const mcmcpp_hip_config* c, std::string& err);

template <class T>
class Sampler final : public SamplerHost<T>
{
    MCMCPP_SAMPLER_HOST_NAMES;
    using Host::exchange_us_per_step, Host::xchg_bytes_per_step, Host::xchg_rollbacks, Host::xchg_cap_slots;

public:
    Sampler() {}
    ~Sampler() override
    {
        quiesce();  // (half_step_async work may still be in flight; the members free themselves behind this, xchg and its communicator first)
    }

    int init(const mcmcpp_hip_config& c)
    {
        cfg = c;
        knobs = Knobs::from_environment();
        set_shape(c);
        table = table_for<T>(c.calc_id);
        if (!table) return fail(MCMCPP_HIP_E_ARG, "calc_id %d has no kernels for this element type", c.calc_id);
        if (table->abi != kLaunchTableAbi || table->elem_size != sizeof(T))
            return fail(MCMCPP_HIP_E_ARG, "calc_id %d: the plug-in was built against other headers (table abi %08x)", c.calc_id, table->abi);

        const int lpw_log = ilog2(lpw), epl_shift = ilog2(epl / Vec16<T>::N);
        if (epl_shift >= kMaxEplShift || !table->half_step[lpw_log][epl_shift])
            return fail(MCMCPP_HIP_E_UNSUPPORTED, "no kernel for D=%d with this calculator (LPW=%d EPL=%d)", D, lpw, epl);
        calc_fn = table->calc[lpw_log][epl_shift];

        if (int rc = resolve_shard(c)) return rc;
        hipDeviceProp_t prop;
        if (int rc = open_device(c, &prop)) return rc;
        if (int rc = xchg.open(this, c)) return rc;  // split ensembles: the caller's communicator, or one from the caller's id
        K = c.num_chains > 1 ? c.num_chains : 1;
        if (K > kMaxChains) return fail(MCMCPP_HIP_E_ARG, "num_chains %d exceeds %d", K, kMaxChains);
        if (K > 1 && (shard_count != n || shard_begin != 0 || c.comm_world >= 1 || c.device_positions))
            return fail(MCMCPP_HIP_E_ARG, "num_chains > 1: whole ensembles on one device only (no shards, communicator or caller-owned positions)");
        if (int rc = open_stream(c)) return rc;

        // which kernels step this handle, and their launch geometry (step_plan.hpp)
        StepShape s = {};
        s.W = W, s.D = D, s.n = n, s.lpw = lpw, s.elem_size = (int)sizeof(T), s.calc_id = c.calc_id;
        s.shard_begin = shard_begin, s.shard_count = shard_count, s.chains = K, s.comm_world = c.comm_world;
        s.num_cus = prop.multiProcessorCount;
        s.graph_steps = c.graph_steps;
        s.can_capture = own_stream || !(stream == nullptr || stream == hipStreamLegacy);
        for (int v = 0; v < 3; ++v) s.half_step_mc[v] = table->half_step_mc[v][lpw_log][epl_shift] != nullptr;
        s.full_step = table->full_step[lpw_log][epl_shift] != nullptr;
        s.full_step_mc = table->full_step_mc[lpw_log][epl_shift] != nullptr;
        plan = plan_stretch_step(s, knobs);
        static_assert((int)HalfStepKernel::MatrixCore8 == 1 && (int)HalfStepKernel::MatrixCore16 == 2 && (int)HalfStepKernel::MatrixCore16Late == 3, "half_step_mc[] is indexed by the enum");
        half_fn = plan.matrix_core_half() ? table->half_step_mc[(int)plan.half - 1][lpw_log][epl_shift] : table->half_step[lpw_log][epl_shift];
        full_fn = plan.full == FullStepKernel::MatrixCore ? table->full_step_mc[lpw_log][epl_shift]
                  : plan.full == FullStepKernel::Plain    ? table->full_step[lpw_log][epl_shift]
                                                          : nullptr;

        if (int rc = allocate(c)) return rc;
        return upload_constants(c);
    }

    // the walkers of each colour this handle updates: the whole half, the configured shard, or the rank's slice
    int resolve_shard(const mcmcpp_hip_config& c)
    {
        shard_begin = c.shard_begin;
        shard_count = c.shard_count > 0 ? c.shard_count : n;
        if (c.comm_world >= 1)
        {
            // a rank of a split ensemble owns the comm_rank-th of comm_world equal slices of each half
            if (c.comm_rank < 0 || c.comm_rank >= c.comm_world) return fail(MCMCPP_HIP_E_ARG, "comm_rank %d outside 0..%d", c.comm_rank, c.comm_world - 1);
            if (n % c.comm_world) return fail(MCMCPP_HIP_E_ARG, "W/2 = %d does not divide by comm_world = %d", n, c.comm_world);
            const int per = n / c.comm_world;
            if (c.shard_count == 0)
            {
                shard_begin = c.comm_rank * per;
                shard_count = per;
            }
            else if (shard_begin != c.comm_rank * per || shard_count != per)
                return fail(MCMCPP_HIP_E_ARG, "the shard of rank %d of %d must be [%d, +%d)", c.comm_rank, c.comm_world, c.comm_rank * per, per);
            if (!c.comm && !c.comm_id) return fail(MCMCPP_HIP_E_ARG, "comm_world >= 1 needs comm_id or comm");
        }
        if (shard_begin < 0 || shard_begin + shard_count > n) return fail(MCMCPP_HIP_E_ARG, "shard out of range");
        return MCMCPP_HIP_OK;
    }

    // every buffer of the handle, sized by the plan
    int allocate(const mcmcpp_hip_config& c)
    {
        const size_t step_bytes = sizeof(T) * (size_t)W * D;
        for (int k = 0; k < 4; ++k)
        {
            HIP_TRY(hipEventCreate(ev_t0[k].replace()));
            HIP_TRY(hipEventCreate(ev_t1[k].replace()));
        }

        const size_t partials_bytes = sizeof(uint32_t) * partials_count(K, plan.partial_slots, plan.partial_waves);
        {
            // everything carved below (each piece rounded up to 256 bytes)
            static_assert(sizeof(Affine128) == kJumpEntryBytes, "the plan sizes the task table by this");
            size_t need = (size_t)K * (full_fn ? 2 : 1) * step_bytes  // pos, pos_alt
                          + (size_t)K * logp_chain_stride_bytes<T>(n) + (size_t)K * kCtlChainStride + tables_total_bytes(n, plan.have_task_table, K)
                          + sizeof(T) * ((size_t)(c.calc_params_len > 0 ? c.calc_params_len : 0) + 32 * 32) + partials_bytes + 64 * 1024;
            HIP_TRY(arena.alloc(need));
            arena_used = 0;
        }
        if (c.device_positions)
        {
            if (((uintptr_t)c.device_positions & 15u) != 0) return fail(MCMCPP_HIP_E_ARG, "device_positions must be 16-byte aligned");
            d_pos = (T*)c.device_positions;
            own_pos = false;
        }
        else
        {
            if (int rc = carve(&d_pos, step_bytes * K)) return rc;
            own_pos = true;
        }
        // log-posteriors [2][W] (the second half is the full-step kernels' other buffer) and, right behind them, the
        // accepted counters [W]: one piece, so that kernels short of preloaded arguments can derive both addresses
        static_assert(sizeof(StepCtl) == 64 && sizeof(RunInfo) == 64 && kRunBehindCtlBytes + (int)sizeof(RunInfo) <= kCtlChainStride, "ChainGeometry");
        if (int rc = carve(&d_logp, logp_chain_stride_bytes<T>(n) * (size_t)K)) return rc;
        d_nacc = reinterpret_cast<uint32_t*>(d_logp + 2 * (size_t)W);
        if (full_fn)
            if (int rc = carve(&d_pos_alt, step_bytes * K)) return rc;
        {
            // the two control records and, kRunBehindCtlBytes behind the first, the run record: one piece (a kernel short
            // of preloaded arguments derives the run record's address)
            static_assert(2 * sizeof(StepCtl) <= (size_t)kRunBehindCtlBytes, "the run record follows the control records");
            char* piece = nullptr;
            if (int rc = carve(&piece, (size_t)kCtlChainStride * (size_t)K)) return rc;
            d_ctl = reinterpret_cast<StepCtl*>(piece);
            d_run = reinterpret_cast<RunInfo*>(offset_bytes(piece, kRunBehindCtlBytes));
        }
        if (int rc = carve(&d_diag, sizeof(Diag))) return rc;
        // the draw records (two buffers: see HalfStepArgs::draws) and, right behind them, the jump tables: one piece
        // whose layout follows from n alone (JumpTables), so that kernels reach the tables from the record pointer
        {
            const bool task = plan.have_task_table;
            char* piece = nullptr;
            if (int rc = carve(&piece, tables_total_bytes(n, task, K))) return rc;
            d_draws = reinterpret_cast<DrawRec<T>*>(piece);
            d_task_jump = task ? reinterpret_cast<Affine128*>(piece + tables_offset_task(n, K)) : nullptr;
            d_jump_hi = reinterpret_cast<Affine128*>(piece + tables_offset_hi(n, task, K));
            d_jump_lo = reinterpret_cast<Affine128*>(piece + tables_offset_lo(n, task, K));
        }
        HIP_TRY(hipMemset(d_draws, 0, sizeof(DrawRec<T>) * draws_count(K, n)));
        HIP_TRY(hipMemset(d_logp, 0, logp_chain_stride_bytes<T>(n) * (size_t)K));
        HIP_TRY(hipMemset(d_diag, 0, sizeof(Diag)));
        HIP_TRY(hipMemset(d_ctl, 0, (size_t)kCtlChainStride * (size_t)K));
        HIP_TRY(h_pinned.alloc(sizeof(PinnedScratch)));
        if (plan.batch_draws > 0)
        {
            HIP_TRY(d_draws_batch.alloc(sizeof(DrawRec<T>) * (size_t)plan.batch_draws * 2 * (size_t)n));
            HIP_TRY(hipMemset(d_draws_batch, 0, sizeof(DrawRec<T>) * (size_t)plan.batch_draws * 2 * (size_t)n));  // (partner indices a kernel may follow)
            HIP_TRY(d_step_jump.alloc(sizeof(Affine128) * (size_t)plan.batch_draws));
        }
        if (int rc = carve(&d_partials, partials_bytes)) return rc;
        HIP_TRY(hipMemset(d_partials, 0, partials_bytes));
        chain_subchunk_bytes = (size_t)knobs.chain_subchunk_mb << 20;
        // a rank of a split ensemble: the exchange side works on this replica (split_exchange.hpp)
        SplitReplica<T> replica;
        replica.owner = this, replica.device = device, replica.stream = stream;
        replica.W = W, replica.D = D, replica.n = n, replica.shard_begin = shard_begin, replica.shard_count = shard_count;
        replica.full_step = full_fn != nullptr, replica.compact = plan.compact_exchange;
        replica.pos = d_pos, replica.pos_alt = d_pos_alt, replica.logp = d_logp, replica.nacc = d_nacc, replica.diag = d_diag;
        return xchg.allocate(replica);
    }

    // what the kernels read and no run changes: calculator parameters, the random stream's seeds and jump tables
    int upload_constants(const mcmcpp_hip_config& c)
    {
        // calculator parameters (and, for the matrix-core kernels, the padded matrix)
        if (c.calc_params_len > 0)
        {
            const CalcParams<T> p = calc_params_host<T>(c, c.calc_id == MCMCPP_HIP_CALC_DENSE_GAUSSIAN && D <= 32);
            if (int rc = carve(&d_params, sizeof(T) * p.prm.size())) return rc;
            HIP_TRY(hipMemcpy(d_params, p.prm.data(), sizeof(T) * p.prm.size(), hipMemcpyHostToDevice));
            if (!p.pad.empty())
            {
                if (int rc = carve(&d_params_padded, sizeof(T) * p.pad.size())) return rc;
                HIP_TRY(hipMemcpy(d_params_padded, p.pad.data(), sizeof(T) * p.pad.size(), hipMemcpyHostToDevice));
            }
        }

        // pcg64 stream (MultiSampler.h:54) and its jump tables
        pcg_seed(c.seed, c.stream, &state0_of[0], &inc);
        for (int k = 1; k < K; ++k)
        {
            U128 inc_k;
            pcg_seed(c.seed + (uint64_t)k, c.stream, &state0_of[k], &inc_k);  // (same stream: the same increment)
        }
        {
            const StretchJumpTables j = stretch_jump_tables(inc, n, plan.have_task_table);
            HIP_TRY(hipMemcpy(d_jump_lo, j.lo.data(), sizeof(Affine128) * j.lo.size(), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d_jump_hi, j.hi.data(), sizeof(Affine128) * j.hi.size(), hipMemcpyHostToDevice));
            if (plan.have_task_table) HIP_TRY(hipMemcpy(d_task_jump, j.task.data(), sizeof(Affine128) * j.task.size(), hipMemcpyHostToDevice));
        }
        half_jump = pcg_jump(inc, (unsigned __int128)3 * (unsigned)n);
        if (plan.batch_draws > 0)
        {
            // step_jump[j]: the draws of j ensemble steps
            std::vector<Affine128> sj((size_t)plan.batch_draws);
            for (size_t j = 0; j < sj.size(); ++j) sj[j] = pcg_jump(inc, (unsigned __int128)6 * (unsigned)n * (unsigned __int128)j);
            HIP_TRY(hipMemcpy(d_step_jump, sj.data(), sizeof(Affine128) * sj.size(), hipMemcpyHostToDevice));
        }
        return MCMCPP_HIP_OK;
    }

    // Everything a step launch touches lives in ONE device allocation, carved here (one allocation, one free; tried as
    // a way to make the cold first accesses of a launch cheaper through fewer address translations: no measurable
    // difference, 6.05 us per launch either way).
    template <class P>
    int carve(P** out, size_t bytes)
    {
        const size_t off = (arena_used + 255) & ~(size_t)255;
        if (off + bytes > arena.bytes()) return fail(MCMCPP_HIP_E_NOMEM, "internal: device arena too small (%zu + %zu > %zu)", off, bytes, arena.bytes());
        *out = reinterpret_cast<P*>(arena + off);
        arena_used = off + bytes;
        return MCMCPP_HIP_OK;
    }

    int set_state(const void* pos, const void* logp) override
    {
        if (!pos || !logp) return fail(MCMCPP_HIP_E_ARG, "set_state: null pointer");
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemcpyAsync(d_pos, pos, sizeof(T) * (size_t)W * D * K, hipMemcpyHostToDevice, stream));
        for (int k = 0; k < K; ++k)
        {
            HIP_TRY(hipMemcpyAsync(logp_of(k), (const T*)logp + (size_t)k * W, sizeof(T) * (size_t)W, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemsetAsync(nacc_of(k), 0, sizeof(uint32_t) * (size_t)W, stream));
        }
        HIP_TRY(hipMemsetAsync(d_diag, 0, sizeof(Diag), stream));
        half_steps = 0;
        steps_since_reset = 0;
        records_valid = false;
        int rc = write_ctl(half_steps, 0);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        have_state = true;
        return MCMCPP_HIP_OK;
    }

    // EnsembleSampler::runMCMC.  Stored steps stream out while the sampler keeps stepping: a run is cut into
    // sub-chunks of stored steps; after the launches of sub-chunk c the same stream copies its device chain
    // half into pinned staging, and while the GPU works on sub-chunk c+1 the host thread copies sub-chunk c's
    // staging into the caller's (pageable) memory.  One stream on purpose: with a second active stream every
    // half-step launch of this latency-bound kernel was measured 1.5 us slower (5.8 -> 7.3 us).
    // Everything is ordered by events; nothing is allocated on the way.
    // A destination in device memory (run_device): chain k's run record points at its part of the caller's array, so the
    // launch that makes a stored step writes it to its final place -- the full-step and the half-step kernels alike, and
    // the captured graphs as they are (they read the record from memory).
    int run_mover(int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step, bool to_device) override
    {
        return xchg.active() ? run_split(n_saved, interval, chain_out, accepted_per_step) : run_whole(n_saved, interval, chain_out, accepted_per_step, to_device);
    }
    int run_chains() const override { return K; }
    RunFacts run_facts() const override
    {
        RunFacts f = {};
        f.mover = Mover::Stretch;
        f.communicator = xchg.active();
        f.sharded = shard_count != n;
        f.half_done = (half_steps & 1) != 0;
        return f;
    }
    void state_abandoned() override { records_valid = false; }

    // The start of a run on the device: the per-step counters cleared, the control records at step 0 of the run, the rows
    // marked as moved for the full-step kernels, the launch arguments.  split_record: the one run record of a split run
    // (a whole-ensemble run uploads a record per sub-chunk).
    int begin_run(size_t acc_entries, const RunInfo* split_record)
    {
        if (acc_entries) HIP_TRY(hipMemsetAsync(d_acc, 0, sizeof(uint32_t) * acc_entries, stream));
        run_touched = true;  // from here on an error leaves the device ahead of the host's bookkeeping
        if (int rc = write_ctl(half_steps, 0)) return rc;  // step_in_run = 0, stream position from the host-side half-step count
        records_valid = false;  // (until this call has finished: an error on the way leaves them unknown)
        run_info_idle = false;
        if (split_record) HIP_TRY(hipMemcpyAsync(d_run, split_record, sizeof(RunInfo), hipMemcpyHostToDevice, stream));
        if (full_fn)
        {
            for (int k = 0; k < K; ++k)
                hipLaunchKernelGGL(mark_rows_moved_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, stream, nacc_of(k), W, kRowMovedBit);
            HIP_TRY(hipGetLastError());
        }
        enq_step = half_steps >> 1;
        run_step = 0;
        args_red = make_args(0);
        args_blk = make_args(1);
        return MCMCPP_HIP_OK;
    }

    // The end of a run that succeeded: the host's bookkeeping moves on, the per-step accepted counts go to the caller, the
    // two host timings.  records_left: did the last launch leave the draw records of the next ensemble step behind (full-step
    // launches: with partner2)?
    using TimePoint = std::chrono::steady_clock::time_point;
    int finish_run(int64_t total, double gpu_ms, bool records_left, uint32_t* accepted_per_step, TimePoint tp1, TimePoint tp2)
    {
        last_ms = gpu_ms;
        last_launches = full_fn ? total : 2 * total;  // (a launch steps all chains)
        half_steps += 2 * (uint64_t)total;
        steps_since_reset += (uint64_t)total;
        records_valid = records_left;
        records_step = half_steps >> 1;
        records_partner2 = full_fn != nullptr;  // (read only while records_valid)
        if (accepted_per_step) HIP_TRY(hipMemcpy(accepted_per_step, d_acc, sizeof(uint32_t) * (size_t)total * K, hipMemcpyDeviceToHost));
        host_enqueue_ms = std::chrono::duration<double, std::milli>(tp2 - tp1).count();
        return MCMCPP_HIP_OK;
    }

    // a sub-chunk whose staging half still has to reach chain_out: wait for its copy, hand it out (every chain), announce it
    int hand_out_staged(char* chain_out, const ChainPlan& cp, size_t step_bytes, StoredRange staged, int buf)
    {
        if (staged.to == staged.from) return MCMCPP_HIP_OK;
        HIP_TRY(hipEventSynchronize(ev_copied[buf]));
        for (int k = 0; k < K; ++k)
        {
            const SubchunkCopy c = subchunk_copy(step_bytes, cp.sub_saved, cp.n_saved, staged.from, staged.to - staged.from, k);
            std::memcpy(chain_out + c.dst, (const char*)h_stage[buf] + c.src, c.bytes);
        }
        publish_stored(staged.to);
        return MCMCPP_HIP_OK;
    }

    // to_device: chain_out is device memory of this device (the entry has checked it)
    int run_whole(int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step, bool to_device)
    {
        const int64_t total = n_saved * (int64_t)interval;

        // how the stored steps reach the caller (run_plan.hpp): sub-chunks through staging, or -- full-step kernels -- the
        // launches forward them to pinned host memory themselves (trickle_stored_step): a ring on the device with a twin in
        // pinned host memory, no copy engine, no gap in the launch sequence
        const size_t step_bytes = sizeof(T) * (size_t)W * D;
        const ChainRequest want = {step_bytes, K, n_saved, interval, chain_out != nullptr, accepted_per_step != nullptr, full_fn != nullptr,
                                   chain_subchunk_bytes, plan.graph_steps, knobs.trickle, knobs.pinned_direct, to_device};
        // chain_out in pinned host memory (mcmcpp_hip_host_alloc: the facade's Chain blocks): the launches forward stored
        // steps straight into their final place -- no pinned twin of the device ring, no host copy
        void* direct_stage = pinned_question_matters(want) ? device_view_of_pinned(chain_out, step_bytes * (size_t)n_saved * K) : nullptr;
        const ChainPlan cp = plan_chain(want, direct_stage != nullptr);
        int rc = ensure_run_buffers(cp.acc_entries, cp.half_bytes, cp.ring_bytes, cp.need_host_ring);
        if (rc) return rc;
        if (tempering && (rc = prepare_tempering())) return rc;
        if ((rc = begin_run(cp.acc_entries, nullptr))) return rc;
        if ((rc = ensure_graphs())) return rc;

        const TimePoint tp1 = std::chrono::steady_clock::now();
        double launch_ms = 0.0;  // GPU time of the step launches alone (downloads excluded)
        if (cp.mode == ChainMode::Trickle)
            rc = run_trickle(n_saved, interval, (char*)chain_out, accepted_per_step != nullptr, step_bytes, cp, &launch_ms, (char*)direct_stage);
        else if (cp.mode == ChainMode::Device)
            rc = run_into_device_chain(n_saved, interval, (char*)chain_out, accepted_per_step != nullptr, step_bytes, cp, &launch_ms);
        StoredRange pending = {0, 0};  // sub-chunk whose staging still has to reach chain_out
        int pending_buf = 0;
        for (int64_t c = 0; c < cp.n_sub && rc == MCMCPP_HIP_OK; ++c)
        {
            const int buf = (int)(c & 1);
            const StoredRange sub = cp.subchunk(c);
            for (int k = 0; k < K; ++k)
            {
                // (several chains: one record each; the upload slots rotate per sub-chunk as for one chain)
                RunInfo* ri = K > 1 ? &h_pinned->chain_run[c % 4][k] : &h_pinned->run[c % 4];
                // chain k's stored steps of this sub-chunk: the k-th run of sub_saved steps of the device half
                *ri = run_info_of_run(chain_out ? (char*)d_chain[buf].get() + subchunk_chain_offset(step_bytes, cp.sub_saved, k) : nullptr,
                                      accepted_per_step ? d_acc + (size_t)k * (size_t)total : nullptr, interval, step_bytes);
                ri->chain_slot_base = -sub.from;
                HIP_TRY(hipMemcpyAsync(run_of(k), ri, sizeof(RunInfo), hipMemcpyHostToDevice, stream));
            }
            // the events of slot c%4 were last used by sub-chunk c-4, which has long been waited for
            HIP_TRY(hipEventRecord(ev_t0[c & 3], stream));
            rc = enqueue_steps((sub.to - sub.from) * interval);
            if (rc) break;
            HIP_TRY(hipEventRecord(ev_t1[c & 3], stream));
            if (c >= 3)
            {
                float ms = 0.f;
                HIP_TRY(hipEventSynchronize(ev_t1[(c - 3) & 3]));
                HIP_TRY(hipEventElapsedTime(&ms, ev_t0[(c - 3) & 3], ev_t1[(c - 3) & 3]));
                launch_ms += ms;
            }
            if (chain_out)
            {
                // the staging buffer is free: its previous content (sub-chunk c-2) was copied out below
                // (the whole device half in one copy: with several chains, chain k's steps sit sub_saved steps apart)
                HIP_TRY(hipMemcpyAsync(h_stage[buf], d_chain[buf], subchunk_half_used(step_bytes, cp.sub_saved, sub.to - sub.from, K), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipEventRecord(ev_copied[buf], stream));
                if ((rc = hand_out_staged((char*)chain_out, cp, step_bytes, pending, pending_buf))) return rc;
                pending = sub;
                pending_buf = buf;
            }
        }
        const TimePoint tp2 = std::chrono::steady_clock::now();
        if (rc) return rc;
        if ((rc = hand_out_staged((char*)chain_out, cp, step_bytes, pending, pending_buf))) return rc;
        if ((rc = bring_ensemble_home())) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        for (int64_t c = (cp.n_sub > 3 ? cp.n_sub - 3 : 0); c < cp.n_sub; ++c)
        {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev_t0[c & 3], ev_t1[c & 3]));
            launch_ms += ms;
        }
        exchange_us_per_step = 0.0;
        // the last launch left the records of the next ensemble step behind -- unless the records were made ahead in
        // batches, which leaves the two-buffer records alone
        // (the device-side RunInfo still points to run-scoped buffers; half_step_async replaces it before it launches)
        return finish_run(total, launch_ms, plan.batch_draws == 0, accepted_per_step, tp1, tp2);
    }

    // ---- one ensemble split over the ranks of an RCCL communicator (BASELINE config 5) -----------------
    // Stands in for ParallelEnsembleSampler::runMCMC with threadCount workers (ParallelEnsembleSampler.h:285-291) and the
    // controller's mid-step / end-step barriers (Threading/RedBlkCtrlerSpinLock.h:240-322).  Every rank holds the full
    // replica of the positions and updates its slice; launches AND exchanges are enqueued on the launch stream by this
    // host thread, nothing waits for the device until the end (stored steps excepted, a staging buffer at a time).
    //   full-step kernels (slices of up to full_step_max_walkers / 2 walkers per colour): ONE exchange per ensemble
    //     step.  A black walker's group repeats the red update of its partner wherever that one lives, so a rank needs
    //     nothing from the others inside a step; afterwards the updated rows and log-posteriors of both colours are
    //     all-gathered (in place: every rank's slice sits where the gather puts it) into the buffer the step wrote.  The
    //     repeated updates read the red draw records of ALL walkers, which fill_draws_kernel makes per step (the
    //     records of a rank's own walkers are also left behind by its draw wavefronts: same bits).
    //   half-step kernels (larger slices): the reference's scheme, one exchange of the updated colour per half-step.
    // The random stream is addressed by the global walker index, so the trajectory does not depend on the number of ranks.
    // The exchanges themselves, the communicator and every buffer only a split run uses are xchg's (split_exchange.hpp); the
    // schedule of a run is SplitWindow's (run_plan.hpp).  Here are the step launches and the order of things.

    // Rank-local preparation of a split run: argument and state checks, staging and counter buffers.  Whatever fails here
    // fails on this rank only -- the caller agrees on it with the other ranks (agree_on_status) before the first launch.
    int prepare_split(int64_t n_saved, int32_t interval, void* chain_out, int64_t* stage_slots_out)
    {
        if (int rc = refuse_run(n_saved, interval, false)) return rc;
        const int64_t total = n_saved * (int64_t)interval;
        const size_t step_bytes = sizeof(T) * (size_t)W * D;
        // stored steps: device -> pinned staging on the launch stream, handed to the caller a staging buffer at a time
        // (the same number of slots on every rank, whether it stores or not: every rank must cut its run into the same chunks)
        const int64_t stage_slots = split_stage_slots(step_bytes, n_saved);
        if (int rc = xchg.prepare_run(chain_out && total > 0 ? step_bytes * (size_t)stage_slots : 0)) return rc;
        *stage_slots_out = stage_slots;
        // (the per-step accepted counts are always kept on the device and all-reduced at the end of a split run, whether this
        //  rank's caller wants them or not: a collective must not depend on one rank's arguments)
        return ensure_run_buffers(total > 0 ? (size_t)total : 0, 0, 0);
    }

    // what SplitWindow (run_plan.hpp) plans a run of `total` steps from
    SplitRequest split_request(int64_t total, int32_t interval, bool any_rank_stores, bool stores, int64_t stage_slots) const
    {
        SplitRequest q = {};
        q.total = total, q.interval = interval, q.any_rank_stores = any_rank_stores, q.stores = stores, q.stage_slots = stage_slots;
        q.compact = plan.compact_exchange, q.cap_full = xchg.cap_full(), q.cap_learned = xchg.cap_learned;
        q.comm_compact_cap = knobs.comm_compact_cap, q.comm_compact_chunk = knobs.comm_compact_chunk;
        q.full_step = full_fn != nullptr, q.comm_world = cfg.comm_world, q.shard_count = shard_count, q.dims = D, q.elem_size = sizeof(T);
        q.block_bytes = &mcmcpp::xblock_bytes;
        return q;
    }

    // what a split run carries from step to step besides the handle's own counters
    struct SplitRun
    {
        HalfStepArgs<T> fill_red;  // full-step scheme: the red draw records of ALL walkers, made per step
        U128 red_base;             // engine state in front of the red half-step of the coming ensemble step
        int unreduced = 0;         // steps whose per-wavefront accepted counts are still to be summed
    };

    // (the per-wavefront accepted counts are summed once per partial_slots steps, and at the end of a chunk)
    void reduce_accepted_if_due(SplitRun& r, bool last_of_chunk)
    {
        if (++r.unreduced == plan.partial_slots || last_of_chunk)
        {
            launch_accepted_reduce(d_partials, plan.partial_slots, plan.partial_waves, r.unreduced, ctl_after((int64_t)run_step + 1), d_run, stream, K);
            r.unreduced = 0;
        }
    }

    // the position buffer that holds the ensemble behind the steps enqueued in this run so far
    bool ensemble_in_alt() const { return full_fn && (run_step & 1); }

    // One ensemble step of a split run with its exchange(s), blocks of `cap` slots; sample >= 0: its (red) exchange is timed
    int enqueue_split_step(SplitRun& r, uint32_t cap, int sample, bool last_of_chunk)
    {
        const int parity = (int)(enq_step & 1), pos_parity = (int)(run_step & 1);
        if (full_fn)
        {
            r.fill_red.draw_parity = parity;
            launch_fill_draws(r.fill_red, r.red_base, nullptr, stream);
            enqueue_step(parity, pos_parity);
            reduce_accepted_if_due(r, last_of_chunk);
            HIP_TRY(hipGetLastError());
            if (int rc = xchg.exchange(!pos_parity, 0, 2, cap, sample)) return rc;  // (the step wrote the buffer it did not read)
            r.red_base = apply(half_jump, apply(half_jump, r.red_base));
        }
        else
        {
            args_red.draw_parity = parity;
            args_blk.draw_parity = parity;
            half_fn(args_red, plan.grid_blocks_for(args_red.shard_count), stream);
            HIP_TRY(hipGetLastError());
            if (int rc = xchg.exchange(false, 0, 1, cap, sample)) return rc;
            half_fn(args_blk, plan.grid_blocks_for(args_blk.shard_count), stream);
            reduce_accepted_if_due(r, last_of_chunk);
            HIP_TRY(hipGetLastError());
            if (int rc = xchg.exchange(false, 1, 1, cap, -1)) return rc;
        }
        enq_step += 1;
        run_step += 1;
        return MCMCPP_HIP_OK;
    }

    // Behind the roll-back of an overflowed chunk: the stream, the control record and the host's counters in front of step
    // `step` of the run that started at half-step half_steps0; the repeated chunk starts at buffer 0 like a run does
    int reposition_split(SplitRun& r, uint64_t half_steps0, int64_t step, int32_t interval)
    {
        records_valid = false;
        if (int rc = write_ctl(half_steps0 + 2 * (uint64_t)step, (uint64_t)step, interval)) return rc;
        enq_step = (half_steps0 >> 1) + (uint64_t)step;
        run_step = 0;
        r.red_base = engine_state_before(half_steps0 + 2 * (uint64_t)step);
        return MCMCPP_HIP_OK;
    }

    // One ensemble over the ranks of a communicator.  The run proceeds in CHUNKS of steps; the host waits for the device
    // only at the end of a chunk, and only when it has a reason to: stored steps to hand out (a staging buffer's worth), or
    // -- exchanging moved rows only -- the overflow flag to look at.  A chunk whose blocks overflowed is rolled back to the
    // snapshot taken in front of it and repeated with blocks that hold a whole slice; the slot bound of the following
    // chunks is what the last one needed, plus an eighth.  SplitWindow (run_plan.hpp) keeps that schedule.
    int run_split(int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step)
    {
        host_enqueue_ms = exchange_us_per_step = 0.0;
        xchg_bytes_per_step = 0.0;
        xchg_rollbacks = 0;
        // ---- prepare, and agree with the other ranks
        int64_t stage_slots = 0;
        const int prep = prepare_split(n_saved, interval, chain_out, &stage_slots);
        const int64_t total = (n_saved > 0 && interval > 0) ? n_saved * (int64_t)interval : 0;
        bool any_rank_stores = false;
        int rc = xchg.agree_on_status(prep, total, interval, chain_out != nullptr, &any_rank_stores);
        if (rc) return rc;
        if (total == 0) return MCMCPP_HIP_OK;

        // ---- begin the run
        const size_t step_bytes = sizeof(T) * (size_t)W * D;
        h_pinned->run[0] = run_info_of_run(nullptr, d_acc, interval, step_bytes);  // (no chain: stored steps are copied from the replica after the exchange)
        if ((rc = begin_run((size_t)total, &h_pinned->run[0]))) return rc;
        const uint64_t half_steps0 = half_steps;  // (the member moves on when the run has succeeded)
        SplitRun r;
        r.red_base = engine_state_before(half_steps0);  // (what write_ctl put into the control record)
        r.fill_red = make_args(0);
        r.fill_red.shard_begin = 0;
        r.fill_red.shard_count = n;
        SplitWindow win(split_request(total, interval, any_rank_stores, chain_out != nullptr, stage_slots));
        if ((rc = xchg.begin_run())) return rc;
        HIP_TRY(hipEventRecord(ev_t0[0], stream));
        const auto tp1 = std::chrono::steady_clock::now();

        while (!win.done())
        {
            // ---- a chunk (every rank cuts alike): snapshot, the steps, the end of the chunk
            if ((rc = xchg.begin_chunk(ensemble_in_alt(), win.cap))) return rc;
            for (int64_t s = win.first(); s < win.end(); ++s)
            {
                if ((rc = enqueue_split_step(r, win.cap, win.take_sample(s), s + 1 == win.end()))) return rc;
                if (win.stores_step(s))
                    HIP_TRY(hipMemcpyAsync(xchg.stage() + step_bytes * (size_t)win.take_stage_slot(), ensemble_in_alt() ? d_pos_alt : d_pos, step_bytes, hipMemcpyDeviceToHost, stream));
            }
            XStats seen = {};
            if (plan.compact_exchange)
            {
                if ((rc = xchg.read_stats(&seen))) return rc;
                if (seen.overflow)
                {
                    // Some block of some exchange of this chunk was too small: whatever the chunk computed rests on a
                    // replica that missed rows.  Back to the snapshot and once more with blocks nothing can overflow.
                    // Every rank reads the same gathered headers, so every rank takes this branch together.
                    const int64_t again_from = win.chunk_overflowed();
                    if ((rc = xchg.rollback())) return rc;
                    if ((rc = reposition_split(r, half_steps0, again_from, interval))) return rc;
                    continue;
                }
            }
            win.chunk_held(seen.max_count);
            xchg.cap_learned = win.cap_learned;
            // ---- stored steps leave where the window says so
            const StoredRange out = win.hand_out();
            if (out.to > out.from)
            {
                HIP_TRY(hipStreamSynchronize(stream));
                std::memcpy((char*)chain_out + step_bytes * (size_t)out.from, xchg.stage(), step_bytes * (size_t)(out.to - out.from));
                publish_stored(out.to);
            }
        }
        const auto tp2 = std::chrono::steady_clock::now();

        // ---- the end of the run
        if ((rc = bring_ensemble_home())) return rc;
        HIP_TRY(hipEventRecord(ev_t1[0], stream));
        if ((rc = xchg.finish_run(d_acc, total))) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        float run_ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&run_ms, ev_t0[0], ev_t1[0]));
        if ((rc = xchg.exchange_us_per_step(win.samples, &exchange_us_per_step))) return rc;
        xchg_bytes_per_step = win.bytes_per_step();
        xchg_rollbacks = win.rollbacks;
        xchg_cap_slots = win.cap_slots();
        // (full-step scheme: the next run re-primes, the red records of other ranks' walkers are per step anyway)
        return finish_run(total, run_ms, full_fn == nullptr, accepted_per_step, tp1, tp2);
    }

    // The two blocks the host loops of run_trickle and run_into_device_chain share (ChunkWindow, run_plan.hpp): the next
    // chunk of `now` steps, enqueued between the two events of its slot ...
    int enqueue_chunk(ChunkWindow& win, int64_t now)
    {
        const int e = win.event_slot(win.next_chunk);
        HIP_TRY(hipEventRecord(ev_t0[e], stream));
        if (const int rc = enqueue_steps(now)) return rc;
        HIP_TRY(hipEventRecord(ev_t1[e], stream));
        win.enqueued(now);
        return MCMCPP_HIP_OK;
    }
    // ... and the wait for the oldest chunk in flight, whose GPU time joins *launch_ms
    int wait_for_oldest_chunk(const ChunkWindow& win, double* launch_ms)
    {
        const int e = win.event_slot(win.oldest);
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(ev_t1[e]));
        HIP_TRY(hipEventElapsedTime(&ms, ev_t0[e], ev_t1[e]));
        *launch_ms += ms;
        return MCMCPP_HIP_OK;
    }

    // The chain path of the full-step kernels: the launches forward stored steps into the pinned ring (or into chain_out
    // itself, `direct_stage`), the host enqueues chunks of steps, stays one chunk ahead of the one it waits for and copies
    // out whatever has become complete.  TrickleWindow (run_plan.hpp) keeps the schedule; the HIP calls and copies are here.
    int run_trickle(int64_t n_saved, int32_t interval, char* chain_out, bool want_accepted, size_t step_bytes, const ChainPlan& cp, double* launch_ms,
                    char* direct_stage)
    {
        const int64_t total = n_saved * (int64_t)interval;
        // chain k: its own ring of stored steps on the device (and, unless the launches forward into chain_out itself,
        // its own twin in pinned memory); in the caller's memory chain k is the k-th run of n_saved steps
        const size_t ring_bytes = step_bytes * (size_t)cp.ring, out_bytes = step_bytes * (size_t)n_saved;
        for (int k = 0; k < K; ++k)
        {
            RunInfo* ri = &h_pinned->chain_run[0][k];
            *ri = run_info_of_run((char*)d_ring + ring_bytes * (size_t)k, want_accepted ? d_acc + (size_t)k * (size_t)total : nullptr, interval, step_bytes);
            ri->stage = cp.direct ? (void*)(direct_stage + out_bytes * (size_t)k) : (void*)((char*)h_ring + ring_bytes * (size_t)k);
            ri->slot_mask = cp.ring - 1;
            ri->slice_bytes = cp.slice_bytes;
            HIP_TRY(hipMemcpyAsync(run_of(k), ri, sizeof(RunInfo), hipMemcpyHostToDevice, stream));
        }

        TrickleWindow win(n_saved, interval, cp);
        // pinned ring -> the caller's memory (forwarded into chain_out itself, they are where they belong already)
        auto copy_out = [&](StoredRange r, bool quick) {
            if (cp.direct) return;
            for (int64_t s = r.from; s < r.to; ++s)
                for (int k = 0; k < K; ++k)
                {
                    char* dst = chain_out + out_bytes * (size_t)k + step_bytes * (size_t)s;
                    const char* src = (char*)h_ring + ring_bytes * (size_t)k + step_bytes * (size_t)win.ring_slot(s);
                    if (quick)
                        parallel_memcpy(dst, src, step_bytes);  // nothing left to overlap with: be quick
                    else
                        std::memcpy(dst, src, step_bytes);
                }
        };
        auto process_oldest = [&]() -> int {
            if (const int rc = wait_for_oldest_chunk(win, launch_ms)) return rc;
            copy_out(win.process_oldest(), win.all_enqueued());
            publish_stored(win.copied);
            return MCMCPP_HIP_OK;
        };
        while (!win.all_enqueued())
        {
            const int64_t now = win.next_length();
            while (win.must_process_oldest_before(now))
            {
                const int rc = process_oldest();
                if (rc) return rc;
            }
            if (const int rc = enqueue_chunk(win, now)) return rc;
        }
        // What the launches do not forward: the run's last stored step.  Its download is queued now, behind the last
        // launch, so that it runs while the host still copies out the steps before it.
        for (int k = 0; k < K; ++k)
        {
            const size_t off = ring_bytes * (size_t)k + step_bytes * (size_t)win.ring_slot(n_saved - 1);
            char* dst = cp.direct ? chain_out + out_bytes * (size_t)k + step_bytes * (size_t)(n_saved - 1) : (char*)h_ring + off;
            HIP_TRY(hipMemcpyAsync(dst, (char*)d_ring + off, step_bytes, hipMemcpyDeviceToHost, stream));
        }
        while (win.in_flight())
        {
            const int rc = process_oldest();
            if (rc) return rc;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        copy_out(win.tail(), true);  // (exactly one: every earlier one has been forwarded and copied above)
        publish_stored(win.copied);
        return MCMCPP_HIP_OK;
    }

    // The chain path of a device destination: one run record per chain for the whole run, then chunks of steps; a finished
    // chunk only tells wait_stored how far the stored steps have come.  DeviceWindow (run_plan.hpp) keeps the schedule.
    int run_into_device_chain(int64_t n_saved, int32_t interval, char* device_chain, bool want_accepted, size_t step_bytes, const ChainPlan& cp, double* launch_ms)
    {
        const int64_t total = n_saved * (int64_t)interval;
        for (int k = 0; k < K; ++k)
        {
            RunInfo* ri = &h_pinned->chain_run[0][k];
            // (chain_slot_base 0, slots never reused, nothing forwarded: run_info_of_run's record as it is)
            *ri = run_info_of_run(device_chain + device_chain_offset(step_bytes, n_saved, k), want_accepted ? d_acc + (size_t)k * (size_t)total : nullptr, interval, step_bytes);
            HIP_TRY(hipMemcpyAsync(run_of(k), ri, sizeof(RunInfo), hipMemcpyHostToDevice, stream));
        }
        DeviceWindow win(n_saved, interval, cp);
        auto process_oldest = [&]() -> int {
            if (const int rc = wait_for_oldest_chunk(win, launch_ms)) return rc;
            publish_stored(win.process_oldest().to);
            return MCMCPP_HIP_OK;
        };
        while (!win.all_enqueued())
        {
            while (win.must_process_oldest_first())
                if (const int rc = process_oldest()) return rc;
            const int64_t now = win.next_length();
            if (const int rc = enqueue_chunk(win, now)) return rc;
        }
        while (win.in_flight())
            if (const int rc = process_oldest()) return rc;
        return MCMCPP_HIP_OK;
    }

    // Device-visible address of [p, p + bytes) when that range is pinned host memory (hipHostMalloc / mcmcpp_hip_host_alloc),
    // nullptr for pageable memory.
    void* device_view_of_pinned(void* p, size_t bytes)
    {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeHost || at.devicePointer == nullptr)
        {
            (void)hipGetLastError();  // (pageable memory is reported as an error)
            return nullptr;
        }
        hipPointerAttribute_t last;
        if (hipPointerGetAttributes(&last, (char*)p + bytes - 1) != hipSuccess || last.type != hipMemoryTypeHost)
        {
            (void)hipGetLastError();
            return nullptr;
        }
        return at.devicePointer;
    }

    int get_state(void* pos, void* logp, uint32_t* n_accept) override
    {
        if (!have_state) return fail(MCMCPP_HIP_E_STATE, "get_state: no walker state (set_state has not been called, or a run failed half way)");
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
        if (pos) HIP_TRY(hipMemcpy(pos, d_pos, sizeof(T) * (size_t)W * D * K, hipMemcpyDeviceToHost));
        for (int k = 0; k < K; ++k)
        {
            if (logp) HIP_TRY(hipMemcpy((T*)logp + (size_t)k * W, logp_of(k), sizeof(T) * (size_t)W, hipMemcpyDeviceToHost));
            if (n_accept) HIP_TRY(hipMemcpy(n_accept + (size_t)k * W, nacc_of(k), sizeof(uint32_t) * (size_t)W, hipMemcpyDeviceToHost));
        }
        if (n_accept)
            for (size_t w = 0; w < (size_t)W * K; ++w) n_accept[w] &= ~kRowMovedBit;  // (the top bit is the full-step kernels' bookkeeping)
        return MCMCPP_HIP_OK;
    }

    int seek(uint64_t steps_done) override
    {
        if (!have_state) return fail(MCMCPP_HIP_E_STATE, "seek: set_state has not been called");
        if (steps_done > (~0ULL >> 2)) return fail(MCMCPP_HIP_E_ARG, "seek: step count out of range");
        HIP_TRY(hipSetDevice(device));
        half_steps = 2 * steps_done;
        records_valid = false;
        return write_ctl(half_steps, 0);  // repositions the stream and re-primes the draw records of the next two half-steps
    }

    int reset_counters() override
    {
        HIP_TRY(hipSetDevice(device));
        for (int k = 0; k < K; ++k) HIP_TRY(hipMemsetAsync(nacc_of(k), 0, sizeof(uint32_t) * (size_t)W, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        steps_since_reset = 0;
        return MCMCPP_HIP_OK;
    }

    int get_counters(uint64_t* accepted, uint64_t* steps, uint64_t* ties, uint64_t* redraws) override
    {
        if (int rc = read_counters(nullptr, steps, ties, redraws)) return rc;
        if (accepted)
        {
            std::vector<uint32_t> a((size_t)W);
            uint64_t s = 0;
            for (int k = 0; k < K; ++k)
            {
                HIP_TRY(hipMemcpy(a.data(), nacc_of(k), sizeof(uint32_t) * (size_t)W, hipMemcpyDeviceToHost));
                for (int c = 0; c < 2; ++c)
                    for (int i = 0; i < shard_count; ++i) s += a[(size_t)c * n + shard_begin + i] & ~kRowMovedBit;
            }
            *accepted = s;
        }
        return MCMCPP_HIP_OK;
    }

    int calc_logp(const void* pos, int64_t count, void* out) override { return kernel_calc_logp(calc_fn, d_params, pos, count, out); }

    // Per-chain calculator parameters (ChainGeometry).  The first block set moves the parameters out of the arena (sized for
    // one block) into [K][chain_params_stride], every row a copy of the create-time block; the step launches then carry the
    // new pointers and the stride, so the cached graphs, which froze the old ones into their nodes, are dropped.  Later blocks
    // are rewritten in place, ordered on the launch stream: the graphs read them from memory.
    int set_chain_params(int32_t chain, const void* params, int32_t len) override
    {
        if (int rc = chain_params_supported("set_chain_params")) return rc;
        if (chain < 0 || chain >= K) return fail(MCMCPP_HIP_E_ARG, "set_chain_params: chain %d outside 0..%d", chain, K - 1);
        if (cfg.calc_params_len == 0) return fail(MCMCPP_HIP_E_ARG, "set_chain_params: calculator %d takes no parameters", cfg.calc_id);
        if (len != cfg.calc_params_len)
            return fail(MCMCPP_HIP_E_ARG, "set_chain_params: len %d, but the handle's calculator takes %d parameters", len, cfg.calc_params_len);
        if (!params) return fail(MCMCPP_HIP_E_ARG, "set_chain_params: params is NULL");
        mcmcpp_hip_config c = cfg;
        c.calc_params = params;
        std::string why;
        if (int rc = check_config(&c, why)) return fail(rc, "set_chain_params: %s", why.c_str());
        HIP_TRY(hipSetDevice(device));
        const CalcParams<T> p = calc_params_host<T>(c, d_params_padded != nullptr);
        const size_t prm_row = (p.prm.size() + 255 / sizeof(T)) & ~(size_t)(255 / sizeof(T));  // (the padded P^T 256-byte aligned)
        if (!d_chain_params)
        {
            const size_t stride = prm_row + p.pad.size();
            if (stride > (size_t)INT32_MAX) return fail(MCMCPP_HIP_E_ARG, "set_chain_params: %zu elements per chain are too many", stride);
            DeviceBuffer<T> rows;
            if (rows.alloc(sizeof(T) * stride * (size_t)K) != hipSuccess)
                return fail(MCMCPP_HIP_E_NOMEM, "set_chain_params: cannot allocate %zu bytes of per-chain parameters", sizeof(T) * stride * (size_t)K);
            HIP_TRY(hipStreamSynchronize(stream));
            drop_graphs();
            for (int k = 0; k < K; ++k)
            {
                T* const row = rows + stride * (size_t)k;
                HIP_TRY(hipMemcpyAsync(row, d_params, sizeof(T) * p.prm.size(), hipMemcpyDeviceToDevice, stream));
                if (d_params_padded) HIP_TRY(hipMemcpyAsync(row + prm_row, d_params_padded, sizeof(T) * p.pad.size(), hipMemcpyDeviceToDevice, stream));
            }
            d_params = rows;
            if (d_params_padded) d_params_padded = rows + prm_row;
            d_chain_params = std::move(rows);
            chain_params_stride = (int)stride;
        }
        T* const row = d_chain_params + (size_t)chain_params_stride * (size_t)chain;
        HIP_TRY(hipMemcpyAsync(row, p.prm.data(), sizeof(T) * p.prm.size(), hipMemcpyHostToDevice, stream));
        if (!p.pad.empty()) HIP_TRY(hipMemcpyAsync(row + prm_row, p.pad.data(), sizeof(T) * p.pad.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }

    int calc_logp_chain(int32_t chain, const void* pos, int64_t count, void* out) override
    {
        if (int rc = chain_params_supported("calc_logp_chain")) return rc;
        if (chain < 0 || chain >= K) return fail(MCMCPP_HIP_E_ARG, "calc_logp_chain: chain %d outside 0..%d", chain, K - 1);
        const T* prm = d_chain_params ? d_chain_params + (size_t)chain_params_stride * (size_t)chain : d_params;
        return kernel_calc_logp(calc_fn, prm, pos, count, out);
    }

    // calc_logp_chain on rows that are in device memory already (a stored device chain), into device memory
    int calc_logp_device(int32_t chain, const void* pos, int64_t count, void* out) override
    {
        if (chain < 0 || chain >= K) return fail(MCMCPP_HIP_E_ARG, "calc_logp_device: chain %d outside 0..%d", chain, K - 1);
        const T* prm = d_chain_params ? d_chain_params + (size_t)chain_params_stride * (size_t)chain : d_params;
        return kernel_calc_logp_device(calc_fn, prm, pos, count, out);
    }

    // One replica-exchange round among the K chains (replica_plan.hpp has the rule).  It works on the home state between
    // runs: d_pos and logp_of(k)[0..W).  Two launches (ReplicaRound::enqueue): the cross evaluations of all pairs (chain k's
    // parameters on chain k + 1's rows and the other way round), then the swaps.  The step streams, half_steps and n_accept stay
    // as they are; so do the draw records left by the last run: they hold draws and partner indices, nothing of a walker's
    // row (DrawRec), and begin_run marks every row as moved for the full-step kernels.
    int exchange_chains(uint64_t round, uint64_t* proposed, uint64_t* accepted, uint64_t* near_ties) override
    {
        if (int rc = chain_params_supported("exchange_chains")) return rc;
        if (K < 2) return fail(MCMCPP_HIP_E_ARG, "exchange_chains: the handle has one chain (num_chains must be at least 2)");
        if (round >= kReplicaMaxRound) return fail(MCMCPP_HIP_E_ARG, "exchange_chains: round %llu is out of range (rounds are below 2^40)", (unsigned long long)round);
        if (!have_state) return fail(MCMCPP_HIP_E_STATE, "exchange_chains: no walker state (set_state has not been called, or a run failed half way)");
        for (int k = 0; k + 1 < K; ++k)
        {
            if (proposed) proposed[k] = 0;
            if (accepted) accepted[k] = 0;
            if (near_ties) near_ties[k] = 0;
        }
        const int pairs = replica_pairs(K, round);
        if (pairs == 0) return MCMCPP_HIP_OK;
        HIP_TRY(hipSetDevice(device));
        if (int rc = ensure_replica("exchange_chains")) return rc;
        if (int rc = rounds.clear_counts(stream)) return rc;
        if (int rc = rounds.enqueue(replica_ensemble(false, 0u), round, stream)) return rc;
        ReplicaCounts counts[kReplicaCountRecords];
        if (int rc = rounds.read_counts(counts, stream)) return rc;
        for (int j = 0; j < pairs; ++j)
        {
            const int ka = replica_lower_chain(round, j);
            if (proposed) proposed[ka] = (uint64_t)W;
            if (accepted) accepted[ka] = counts[ka].accepted;
            if (near_ties) near_ties[ka] = counts[ka].near_ties;
        }
        return MCMCPP_HIP_OK;
    }

    // The ratios of normalising constants between neighbouring chains, from stored steps (evidence.hip): the refusals of
    // exchange_chains that concern the handle; the walker state is neither needed nor touched
    int evidence_ratios(EvidenceRequest q) override
    {
        if (int rc = chain_params_supported(q.what)) return rc;
        if (K < 2) return fail(MCMCPP_HIP_E_ARG, "%s: the handle has one chain (num_chains must be at least 2)", q.what);
        q.dtype = sizeof(T) == 8 ? MCMCPP_HIP_F64 : MCMCPP_HIP_F32;
        q.device = device, q.K = K, q.W = W, q.D = D;
        return evidence_compute(*this, q);
    }
    // The bridge estimate of the same ratios (bridge.hip): the same refusals
    int evidence_bridge(BridgeRequest b) override
    {
        if (int rc = chain_params_supported(b.q.what)) return rc;
        if (K < 2) return fail(MCMCPP_HIP_E_ARG, "%s: the handle has one chain (num_chains must be at least 2)", b.q.what);
        b.q.dtype = sizeof(T) == 8 ? MCMCPP_HIP_F64 : MCMCPP_HIP_F32;
        b.q.device = device, b.q.K = K, b.q.W = W, b.q.D = D;
        return bridge_compute(*this, b);
    }
    // All K log-normalising constants in one joint solve (mbar.hip): the same refusals
    int evidence_mbar(MbarRequest m) override
    {
        if (int rc = chain_params_supported(m.q.what)) return rc;
        if (K < 2) return fail(MCMCPP_HIP_E_ARG, "%s: the handle has one chain (num_chains must be at least 2)", m.q.what);
        m.q.dtype = sizeof(T) == 8 ? MCMCPP_HIP_F64 : MCMCPP_HIP_F32;
        m.q.device = device, m.q.K = K, m.q.W = W, m.q.D = D;
        return mbar_compute(*this, m);
    }
    // The evidence of one chain's target by a bridge to a fitted Gaussian (gaussian_bridge.hip): one chain will do
    int evidence_gaussian(GaussianBridgeRequest g) override
    {
        if (int rc = chain_params_supported(g.q.what)) return rc;
        return gaussian_evidence(g, K);
    }

    // A run with its replica-exchange rounds inside the launch sequence (temper_plan.hpp has the schedule).  It is a run like
    // any other -- run_entry, run_whole, whichever way the stored steps travel -- whose enqueue_steps cuts the step launches at
    // the exchange points and puts a round's two launches there (ReplicaRound::enqueue).  The counters of the rounds stay on the device
    // until the run is over.
    int run_tempered(int64_t n_saved, int32_t interval, int64_t exchange_every, uint64_t first_round, void* chain, uint32_t* accepted_per_step,
                     uint64_t* proposed, uint64_t* accepted, uint64_t* near_ties, uint64_t* rounds_done, bool to_device) override
    {
        if (int rc = chain_params_supported("run_tempered")) return rc;
        TemperSchedule s = {};
        s.total = n_saved > 0 && interval >= 1 ? n_saved * (int64_t)interval : 0;  // (bad arguments: the run refuses them below)
        s.every = exchange_every, s.first_round = first_round, s.K = K;
        const TemperRefusal refusal = temper_refusal(s);
        if (refusal != TemperRefusal::None) return fail(MCMCPP_HIP_E_ARG, "run_tempered: %s", temper_refusal_text(refusal));
        temper = s;
        tempering = true;
        const int rc = Host::run_entry(n_saved, interval, chain, accepted_per_step, to_device);
        tempering = false;
        if (rc) return rc;
        ReplicaCounts counts[kReplicaCountRecords] = {};
        if (temper_rounds(s) > 0 && rounds.read_counts(counts, stream)) return MCMCPP_HIP_E_HIP;
        for (int k = 0; k + 1 < K; ++k)
        {
            if (proposed) proposed[k] = (uint64_t)W * (uint64_t)temper_rounds_pairing(s, k);
            if (accepted) accepted[k] = counts[k].accepted;
            if (near_ties) near_ties[k] = counts[k].near_ties;
        }
        if (rounds_done) *rounds_done = (uint64_t)temper_rounds(s);
        return MCMCPP_HIP_OK;
    }

    int half_step_async(int32_t color, int64_t save_slot) override
    {
        if (K > 1) return fail(MCMCPP_HIP_E_UNSUPPORTED, "half_step_async: not with several chains per handle");
        if (!have_state) return fail(MCMCPP_HIP_E_STATE, "half_step_async: set_state has not been called");
        if (color != (int)(half_steps & 1)) return fail(MCMCPP_HIP_E_ARG, "half_step_async: colour %d out of order", color);
        if (save_slot >= 0 && (!bound_chain || save_slot >= bound_slots))
            return fail(MCMCPP_HIP_E_ARG, "half_step_async: save_slot outside the bound device chain");
        HIP_TRY(hipSetDevice(device));
        // A run whose launches read records made ahead (fill_batch) leaves the two-buffer records where an earlier step put
        // them: a step that starts here makes its own.  (Every other way to this point has left this step's records behind.)
        if (color == 0 && plan.batch_draws > 0 && !(records_valid && records_step == (half_steps >> 1)))
        {
            const int rc = write_ctl(half_steps, 0);
            if (rc) return rc;
        }
        if (!run_info_idle)
        {
            const int rc = upload_idle_run_info();
            if (rc) return rc;
        }
        HalfStepArgs<T> a = make_args(color, (int)((half_steps >> 1) & 1));
        a.use_ctl_save = 0;
        a.partials = nullptr;
        a.direct_save_slot = save_slot;
        half_fn(a, plan.grid_blocks_for(shard_count), stream);
        HIP_TRY(hipGetLastError());
        half_steps += 1;
        if (color == 1) steps_since_reset += 1;
        // the two launches of a step leave the next step's records of this handle's shard behind (without partner2)
        records_valid = color == 1 && shard_count == n;
        records_step = half_steps >> 1;
        records_partner2 = false;
        return MCMCPP_HIP_OK;
    }

    int bind_device_chain(void* chain, int64_t slots) override
    {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
        bound_chain = chain;
        bound_slots = chain ? slots : 0;
        return upload_idle_run_info();
    }

    int shard_span(int32_t color, int64_t* off, int64_t* cnt) override
    {
        if (color != 0 && color != 1) return fail(MCMCPP_HIP_E_ARG, "shard_span: colour must be 0 or 1");
        if (off) *off = ((int64_t)(color ? n : 0) + shard_begin) * D;
        if (cnt) *cnt = (int64_t)shard_count * D;
        return MCMCPP_HIP_OK;
    }

private:
    // per-chain parameters: one whole ensemble per chain on this device, in buffers of the handle's own
    int chain_params_supported(const char* what)
    {
        if (shard_count != n || shard_begin != 0) return fail(MCMCPP_HIP_E_UNSUPPORTED, "%s: not for a sharded handle", what);
        if (cfg.comm_world >= 1) return fail(MCMCPP_HIP_E_UNSUPPORTED, "%s: not for a handle with a communicator", what);
        if (!own_pos) return fail(MCMCPP_HIP_E_UNSUPPORTED, "%s: not for a handle with caller-owned positions", what);
        return MCMCPP_HIP_OK;
    }

    // the scratch of a round and the launcher of its cross evaluations: once per handle, by the first round or tempered run
    int ensure_replica(const char* what)
    {
        return rounds.ensure(this, what, table->replica_cross[ilog2(lpw)][ilog2(epl / Vec16<T>::N)], cfg.seed, cfg.stream, W, D);
    }

    // in front of the first launch of a tempered run: the scratch of its rounds, the run's counters zeroed
    int prepare_tempering()
    {
        if (int rc = ensure_replica("run_tempered")) return rc;
        return rounds.clear_counts(stream);
    }

    // what a round works on: the home buffers, or (alt) the second position buffer and log-posterior half
    ReplicaEnsemble<T> replica_ensemble(bool alt, uint32_t moved_bit) const
    {
        ReplicaEnsemble<T> e = {};
        e.pos = alt ? d_pos_alt : d_pos, e.logp = d_logp + (alt ? W : 0);
        e.logp_stride_bytes = logp_chain_stride_bytes<T>(n);
        e.nacc_behind_logp_bytes = sizeof(T) * (size_t)(alt ? W : 2 * W);  // (nacc_of(k) = logp_of(k) + 2 W)
        e.moved_bit = moved_bit;
        e.params = d_params, e.params_chain_stride = chain_params_stride;
        e.K = K, e.W = W, e.D = D, e.vec_ok = vec_ok;
        const long long per_block = (long long)(64 / lpw) * kWavesPerBlock;
        e.cross_grid = (unsigned)((W + per_block - 1) / per_block);
        return e;
    }

    // the instantiated graphs (their kernel nodes hold the launch arguments of the time of capture); the stream is idle
    void drop_graphs() { graph_cache.clear(); }

    int hip_rc(hipError_t e, const char* what)
    {
        if (e == hipSuccess) return MCMCPP_HIP_OK;
        return fail(MCMCPP_HIP_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    }

    // An odd number of full steps leaves the ensemble in the second buffer: bring it (and the control record) home, so
    // that everything outside run() only ever knows the first
    int bring_ensemble_home()
    {
        if (!full_fn || !(run_step & 1)) return MCMCPP_HIP_OK;
        HIP_TRY(hipMemcpyAsync(d_pos, d_pos_alt, sizeof(T) * (size_t)W * D * K, hipMemcpyDeviceToDevice, stream));
        for (int k = 0; k < K; ++k)
        {
            HIP_TRY(hipMemcpyAsync(logp_of(k), logp_of(k) + W, sizeof(T) * (size_t)W, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(ctl_of(k), ctl_of(k) + 1, sizeof(StepCtl), hipMemcpyDeviceToDevice, stream));
        }
        return MCMCPP_HIP_OK;
    }

    // RunInfo used outside run(): the chain bound for half_step_async (if any), no per-step counters
    int upload_idle_run_info()
    {
        RunInfo ri = idle_run_info();
        ri.chain = bound_chain;
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(d_run, &ri, sizeof ri, hipMemcpyHostToDevice));
        run_info_idle = true;
        return MCMCPP_HIP_OK;
    }

    // chain k's calculator parameters: its own block, or the one all chains share
    const T* params_of(int k) const { return d_chain_params ? d_chain_params + (size_t)chain_params_stride * (size_t)k : d_params; }

    // chain k's arrays (ChainGeometry; k = 0: the arrays themselves)
    T* logp_of(int k) const { return logp_of_chain<T>(d_logp, n, k); }
    uint32_t* nacc_of(int k) const { return reinterpret_cast<uint32_t*>(logp_of(k) + 2 * (size_t)W); }
    StepCtl* ctl_of(int k) const { return ctl_of_chain(d_ctl, k); }
    RunInfo* run_of(int k) const { return ctl_of_chain(d_run, k); }

    HalfStepArgs<T> make_args(int color, int parity) const
    {
        HalfStepArgs<T> a = make_args(color);
        a.draw_parity = parity;
        return a;
    }

    HalfStepArgs<T> make_args(int color) const
    {
        HalfStepArgs<T> a = stretch_args<T>(cfg, vec_ok, inc, half_jump);
        a.pos = d_pos;
        a.logp = d_logp;
        a.n_accept = d_nacc;
        a.ctl_in = d_ctl + color;
        a.ctl_out = d_ctl + (1 - color);
        a.run = d_run;
        a.diag = d_diag;
        a.jump_lo = d_jump_lo;
        a.jump_hi = d_jump_hi;
        a.task_jump = d_task_jump;
        a.calc_params = d_params;
        a.draws = d_draws;
        a.color = color;
        a.shard_begin = shard_begin;
        a.shard_count = shard_count;
        a.passes = plan.passes;
        a.partials = d_partials;
        a.partial_slots = plan.partial_slots;
        a.partial_waves = plan.partial_waves;
        a.draw_parity = 0;
        a.pos_alt = d_pos_alt;
        a.logp_alt = d_logp + W;
        a.pos_parity = 0;
        a.calc_params_padded = d_params_padded;
        a.chains = K;
        a.params_chain_stride = chain_params_stride;
        a.draw_wave = plan.half_draw_wave;
        return a;
    }

    // the engine state of chain k in front of half-step h (a half-step draws 3 numbers per walker of its colour)
    U128 engine_state_before(uint64_t h, int k = 0) const
    {
        return apply(pcg_jump(inc, (unsigned __int128)3 * (unsigned)n * (unsigned __int128)h), state0_of[k]);
    }

    // device StepCtl[0] <- {stream position of half-step `at`, counters}; `at` must be even (the host's half_steps, or -- a
    // chunk of a split run being repeated -- where that chunk starts)
    // step_in_run > 0 (such a chunk): the counters the kernels keep instead of dividing follow
    int write_ctl(uint64_t at, uint64_t step_in_run, int32_t interval = 1)
    {
        // the draw records of the next red and the next black half-step (afterwards the launches keep them going):
        // unless the launches of the previous call left exactly these behind
        const bool refill = !(records_valid && records_step == (at >> 1) && (!full_fn || records_partner2));
        for (int k = 0; k < K; ++k)
        {
            StepCtl* c = K > 1 ? &h_pinned->chain_ctl[k] : &h_pinned->ctl;
            c->state = engine_state_before(at, k);
            const U128 state1 = apply(half_jump, c->state);
            c->state2 = apply(half_jump, state1);
            c->half_step = at;
            c->step_in_run = step_in_run;
            c->chain_slot = (long long)(step_in_run / (uint64_t)interval);
            c->save_phase = (uint32_t)(step_in_run % (uint64_t)interval);
            c->partial_slot = (uint32_t)(step_in_run % (uint64_t)plan.partial_slots);
            HIP_TRY(hipMemcpyAsync(ctl_of(k) + (at & 1), c, sizeof(StepCtl), hipMemcpyHostToDevice, stream));
            if (refill)
            {
                const int parity = (int)((at >> 1) & 1);  // the buffer the coming ensemble step reads
                HalfStepArgs<T> fr = make_args(0, parity), fb = make_args(1, parity);
                fr.draws = fb.draws = d_draws + draws_chain_offset(k, n);  // (the chain's own records; the tables are shared)
                launch_fill_draws(fr, c->state, nullptr, stream);
                launch_fill_draws(fb, state1, full_fn ? &c->state : nullptr, stream);
                HIP_TRY(hipGetLastError());
            }
        }
        if (refill)
        {
            records_valid = true;
            records_step = at >> 1;
            records_partner2 = full_fn != nullptr;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }

    // pos_parity: which position buffer a full-step launch reads (ensemble steps enqueued in this run() & 1)
    // batch_slot >= 0: the step's draw records are record set batch_slot of d_draws_batch, made ahead (fill_batch)
    void enqueue_step(int parity, int pos_parity, int batch_slot = -1)
    {
        if (full_fn)
        {
            HalfStepArgs<T>& a = args_red;
            a.draw_parity = parity;
            a.pos_parity = pos_parity;
            a.ctl_in = d_ctl + pos_parity;
            a.ctl_out = d_ctl + (1 - pos_parity);
            a.draw_wave = plan.full_draw_wave;
            if (batch_slot >= 0)
            {
                a.draw_wave = 2;
                a.draw_parity = 0;
                a.draws = d_draws_batch + (size_t)batch_slot * 2 * (size_t)n;
            }
            full_fn(a, plan.full_grid_blocks_for(a.shard_count), stream);
            a.draws = d_draws;
            return;
        }
        args_red.draw_parity = parity;
        args_blk.draw_parity = parity;
        half_fn(args_red, plan.grid_blocks_for(args_red.shard_count), stream);
        half_fn(args_blk, plan.grid_blocks_for(args_blk.shard_count), stream);
    }

    // the draw records of `count` ensemble steps from the one that reads position buffer pos_parity on (its control
    // record is what the launch before it left behind, or write_ctl)
    void fill_batch(int pos_parity, int count)
    {
        HalfStepArgs<T> a = args_red;
        a.draws = d_draws;
        launch_fill_draws_batch(a, d_ctl + pos_parity, d_step_jump, d_draws_batch, count, stream);
    }

    // `steps` ensemble steps from record-buffer parity start_parity / position-buffer parity pos_parity on
    void enqueue_step_sequence(int steps, int start_parity, int pos_parity)
    {
        for (int s = 0; s < steps; ++s)
        {
            if (plan.batch_draws > 0)
            {
                if (s % plan.batch_draws == 0) fill_batch((pos_parity + s) & 1, steps - s < plan.batch_draws ? steps - s : plan.batch_draws);
                enqueue_step(0, (pos_parity + s) & 1, s % plan.batch_draws);
            }
            else
                enqueue_step((start_parity + s) & 1, (pos_parity + s) & 1);
        }
    }

    // hipGraph of `steps` ensemble steps followed by the accepted-count reduction (cached per step count:
    // graph_steps for the bulk, one graph per distinct remainder)
    // (the record-buffer parity of every node is frozen into the graph, hence one graph per starting parity)
    int graph_for(int steps, int start_parity, int pos_parity, hipGraphExec_t* out)
    {
        const size_t key = (size_t)steps * 4 + (size_t)start_parity * 2 + (size_t)pos_parity;
        if (graph_cache.size() <= key) graph_cache.resize(key + 1);
        if (!graph_cache[key])
        {
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
            enqueue_step_sequence(steps, start_parity, pos_parity);
            launch_accepted_reduce(d_partials, plan.partial_slots, plan.partial_waves, steps, ctl_after(pos_parity + steps), d_run, stream, K);
            HIP_TRY(hipStreamEndCapture(stream, &g));
            HIP_TRY(hipGraphInstantiate(graph_cache[key].replace(), g, nullptr, nullptr, 0));
            HIP_TRY(hipGraphDestroy(g));
        }
        *out = graph_cache[key];
        return MCMCPP_HIP_OK;
    }

    int ensure_graphs()
    {
        if (plan.graph_steps < 1) return MCMCPP_HIP_OK;
        hipGraphExec_t ex;
        return graph_for(plan.graph_steps, (int)(enq_step & 1), 0, &ex);
    }

    // the control record the last launch of a step sequence leaves behind: the half-step pair always ends in [0],
    // full-step launches alternate with the position buffers
    const StepCtl* ctl_after(int64_t pos_parity_after) const { return d_ctl + (full_fn ? (pos_parity_after & 1) : 0); }

    // enqueue `steps` ensemble steps on the launch stream; a tempered run: in pieces that end at the exchange points, each
    // followed by its round (plain launches between the replays)
    int enqueue_steps(int64_t steps)
    {
        if (!tempering) return enqueue_step_launches(steps);
        while (steps > 0)
        {
            const TemperPiece piece = temper_next_piece(temper, (int64_t)run_step, steps);
            if (int rc = enqueue_step_launches(piece.steps)) return rc;
            if (piece.round_follows)
                if (int rc = rounds.enqueue(replica_ensemble(ensemble_in_alt(), full_fn ? kRowMovedBit : 0u), piece.round, stream)) return rc;
            steps -= piece.steps;
        }
        return MCMCPP_HIP_OK;
    }

    // `steps` ensemble steps: graph replays, or plain launches when graphs are off
    int enqueue_step_launches(int64_t steps)
    {
        // enq_step: ensemble steps enqueued since set_state/seek (its low bit selects the record buffer)
        int64_t left = steps;
        if (plan.graph_steps >= 1)
        {
            hipGraphExec_t ex = nullptr;
            while (left >= plan.graph_steps)
            {
                int rc = graph_for(plan.graph_steps, (int)(enq_step & 1), (int)(run_step & 1), &ex);
                if (rc) return rc;
                HIP_TRY(hipGraphLaunch(ex, stream));
                left -= plan.graph_steps;
                enq_step += (uint64_t)plan.graph_steps;
                run_step += (uint64_t)plan.graph_steps;
            }
            if (left > 0)
            {
                // one replay for the remainder
                int rc = graph_for((int)left, (int)(enq_step & 1), (int)(run_step & 1), &ex);
                if (rc) return rc;
                HIP_TRY(hipGraphLaunch(ex, stream));
                enq_step += (uint64_t)left;
                run_step += (uint64_t)left;
            }
        }
        else
        {
            for (; left > 0; --left)
            {
                enqueue_step_sequence(1, (int)(enq_step & 1), (int)(run_step & 1));
                launch_accepted_reduce(d_partials, plan.partial_slots, plan.partial_waves, 1, ctl_after((int64_t)run_step + 1), d_run, stream, K);
                enq_step += 1;
                run_step += 1;
            }
            HIP_TRY(hipGetLastError());
        }
        return MCMCPP_HIP_OK;
    }

    // persistent per-run buffers, grown on demand: per-step accepted counters, the two halves of the device
    // chain and their pinned staging twins
    int ensure_run_buffers(size_t acc_entries, size_t half_bytes, size_t ring_bytes, bool need_host_ring = true)
    {
        if (grow(d_ring, ring_bytes, stream)) return fail(MCMCPP_HIP_E_NOMEM, "run: cannot allocate %zu bytes of device chain", ring_bytes);
        if (need_host_ring && grow(h_ring, ring_bytes, stream))
            return fail(MCMCPP_HIP_E_NOMEM, "run: cannot allocate %zu bytes of pinned staging", ring_bytes);
        if (grow(d_acc, sizeof(uint32_t) * acc_entries, stream)) return fail(MCMCPP_HIP_E_NOMEM, "run: cannot allocate %zu accepted counters", acc_entries);
        if (half_bytes > 0 && ev_copied[0] == nullptr)
        {
            for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreateWithFlags(ev_copied[k].replace(), hipEventDisableTiming));
        }
        for (int k = 0; k < 2; ++k)
        {
            if (grow(d_chain[k], half_bytes, stream)) return fail(MCMCPP_HIP_E_NOMEM, "run: cannot allocate %zu bytes of device chain", half_bytes);
            if (grow(h_stage[k], half_bytes, stream)) return fail(MCMCPP_HIP_E_NOMEM, "run: cannot allocate %zu bytes of pinned staging", half_bytes);
        }
        return MCMCPP_HIP_OK;
    }

    mcmcpp_hip_config cfg;
    Knobs knobs;
    const LaunchTable<T>* table = nullptr;
    StepPlan plan;  // which kernels step this handle, their launch geometry and what follows from it (step_plan.hpp)
    typename LaunchTable<T>::HalfStepFn half_fn = nullptr;
    typename LaunchTable<T>::HalfStepFn full_fn = nullptr;  // non-null: run() steps with one launch per ensemble step
    T* d_pos_alt = nullptr;
    uint64_t run_step = 0;                                  // ensemble steps enqueued in the current run()
    typename LaunchTable<T>::CalcFn calc_fn = nullptr;
    int shard_begin = 0, shard_count = 0;
    size_t chain_subchunk_bytes = 0;
    Event ev_copied[2];
    DeviceBuffer<char> arena;  // one device allocation holding everything a step launch touches (see carve)
    size_t arena_used = 0;
    DeviceBuffer<char> d_ring;  // full-step chain path: device ring of stored steps
    PinnedBuffer<char> h_ring;  // and its pinned host twin
    DeviceBuffer<T> d_chain[2];
    PinnedBuffer<char> h_stage[2];
    DeviceBuffer<uint32_t> d_acc;
    bool own_pos = false;
    Event ev_t0[4], ev_t1[4];
    T *d_params = nullptr, *d_params_padded = nullptr;  // (row 0 of d_chain_params once a chain has parameters of its own)
    DeviceBuffer<T> d_chain_params;  // [K][chain_params_stride] per-chain parameters (set_chain_params), or empty: shared
    int chain_params_stride = 0;
    StepCtl* d_ctl = nullptr;
    RunInfo* d_run = nullptr;
    DrawRec<T>* d_draws = nullptr;
    DeviceBuffer<DrawRec<T>> d_draws_batch;  // [batch_draws][2][n]: records made ahead of the matrix-core full-step launches
    DeviceBuffer<Affine128> d_step_jump;     // [batch_draws]
    uint32_t* d_partials = nullptr;
    Affine128 *d_jump_lo = nullptr, *d_jump_hi = nullptr, *d_task_jump = nullptr;  // behind d_draws: see JumpTables
    // which ensemble step the draw records on the device belong to, if known, and whether the black ones carry partner2
    bool records_valid = false, records_partner2 = false, run_info_idle = false;
    uint64_t records_step = 0;
    PinnedBuffer<PinnedScratch> h_pinned;
    U128 inc;
    U128 state0_of[kMaxChains];  // per chain (seed + k)
    int K = 1;                   // independent ensembles stepped by one launch
    Affine128 half_jump;
    HalfStepArgs<T> args_red, args_blk;
    std::vector<GraphExec> graph_cache;  // [steps] -> instantiated graph
    uint64_t half_steps = 0, enq_step = 0;
    void* bound_chain = nullptr;
    int64_t bound_slots = 0;
    // replica exchange: the scratch of a round (exchange_chains, run_tempered); a tempered run's schedule while it is in hand
    ReplicaRound<T> rounds;
    bool tempering = false;
    TemperSchedule temper = {};
    // a rank of a split ensemble: the communicator and everything only split runs use (declared last: it goes first, the
    // communicator in front of every buffer)
    SplitExchange<T> xchg;
};

int check_config(const mcmcpp_hip_config* c, std::string& err)
{
    char buf[256];
#define BAD(...)                              \
    do                                        \
    {                                         \
        snprintf(buf, sizeof buf, __VA_ARGS__); \
        err = buf;                            \
        return MCMCPP_HIP_E_ARG;              \
    } while (0)
    if (!c) BAD("config is NULL");
    if (c->struct_size != sizeof(mcmcpp_hip_config)) BAD("struct_size %u != %zu (ABI mismatch)", c->struct_size, sizeof(mcmcpp_hip_config));
    if (c->dtype != MCMCPP_HIP_F64 && c->dtype != MCMCPP_HIP_F32) BAD("dtype must be MCMCPP_HIP_F64 or MCMCPP_HIP_F32");
    if (c->num_params < 1 || c->num_params > 1024) BAD("num_params must be in 1..1024");
    // EnsembleSampler.h:207-208
    if (c->num_walkers < 2 || (c->num_walkers & 1)) BAD("num_walkers must be even");
    if (c->num_walkers <= 2 * c->num_params) BAD("num_walkers must exceed 2*num_params");
    switch (c->calc_id)
    {
    case MCMCPP_HIP_CALC_ISO_GAUSSIAN:
        if (c->calc_params_len != 0) BAD("IsoGaussian takes no parameters");
        break;
    case MCMCPP_HIP_CALC_DENSE_GAUSSIAN:
        if (!c->calc_params || c->calc_params_len != c->num_params * c->num_params) BAD("DenseGaussian needs D*D parameters");
        break;
    case MCMCPP_HIP_CALC_ROSENBROCK:
        if (!c->calc_params || c->calc_params_len != 3) BAD("Rosenbrock needs 3 parameters (a, b, c)");
        break;
    case MCMCPP_HIP_CALC_SKEWED_GAUSSIAN_2D:
        if (!c->calc_params || c->calc_params_len != 1 || c->num_params != 2) BAD("SkewedGaussian2D needs D == 2 and 1 parameter");
        break;
    case MCMCPP_HIP_CALC_BATCH:
        if (c->calc_params_len != 0) BAD("the batch target takes no parameters (the callback's user pointer carries them)");
        if (c->mover != MCMCPP_HIP_MOVER_STRETCH) BAD("the batch target steps with StretchMove only (no differential evolution)");
        if (c->num_chains > 1) BAD("the batch target runs one ensemble per handle (num_chains must be 0 or 1)");
        if (c->shard_begin != 0 || c->shard_count != 0) BAD("the batch target runs the whole ensemble (no shards)");
        if (c->comm_world >= 1 || c->comm || c->comm_id) BAD("the batch target runs on one device (no communicator)");
        break;
    default:
    {
        RegisteredCalc r;
        if (c->calc_id < MCMCPP_HIP_CALC_USER_BASE || !registered_calc(c->calc_id, &r)) BAD("unknown calc_id %d", c->calc_id);
        if (r.params_len >= 0 && c->calc_params_len != r.params_len) BAD("calculator %d takes %d parameters", c->calc_id, r.params_len);
        if (c->calc_params_len < 0 || (c->calc_params_len > 0 && !c->calc_params)) BAD("calc_params missing");
    }
    }
    if (c->shard_begin < 0 || c->shard_count < 0) BAD("negative shard bounds");
    if (c->mover != MCMCPP_HIP_MOVER_STRETCH && c->mover != MCMCPP_HIP_MOVER_DIFFERENTIAL_EVOLUTION) BAD("unknown mover %u", c->mover);
    if (c->comm_world < 0) BAD("comm_world must not be negative");
    if (c->num_chains < 0) BAD("num_chains must not be negative");
    if (c->num_chains > 1 && c->mover != MCMCPP_HIP_MOVER_STRETCH) BAD("several chains per handle: StretchMove only");
    if (c->mover == MCMCPP_HIP_MOVER_DIFFERENTIAL_EVOLUTION && (c->shard_count != 0 || c->device_positions || c->comm_world >= 1))
        BAD("the differential-evolution mover runs one whole ensemble per handle (no shards, no caller-owned position buffer)");
    if (c->gw_alpha_num < 0 || c->gw_alpha_den < 0 || ((c->gw_alpha_num == 0) != (c->gw_alpha_den == 0)))
        BAD("gw_alpha_num/gw_alpha_den must both be positive (or both 0 for the default 2/1)");
    if (c->gw_alpha_num > 0 && c->gw_alpha_num <= c->gw_alpha_den) BAD("the stretch scale alpha must exceed 1");
#undef BAD
    return MCMCPP_HIP_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------
extern "C"
{
int mcmcpp_hip_abi_version(void) { return MCMCPP_HIP_ABI_VERSION; }

int mcmcpp_hip_register_calculator(int32_t calc_id, const void* table_f64, const void* table_f32, int32_t params_len)
{
    if (calc_id < MCMCPP_HIP_CALC_USER_BASE || (!table_f64 && !table_f32) || params_len < -1)
    {
        g_create_error = "register_calculator: calc_id must be >= MCMCPP_HIP_CALC_USER_BASE with at least one table";
        return MCMCPP_HIP_E_ARG;
    }
    const uint32_t a64 = table_f64 ? static_cast<const LaunchTable<double>*>(table_f64)->abi : kLaunchTableAbi;
    const uint32_t a32 = table_f32 ? static_cast<const LaunchTable<float>*>(table_f32)->abi : kLaunchTableAbi;
    if (a64 != kLaunchTableAbi || a32 != kLaunchTableAbi)
    {
        g_create_error = "register_calculator: the plug-in was built against other headers";
        return MCMCPP_HIP_E_ARG;
    }
    RegisteredCalc r;
    r.f64 = table_f64;
    r.f32 = table_f32;
    r.params_len = params_len;
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    g_registry[calc_id] = r;
    return MCMCPP_HIP_OK;
}

int mcmcpp_hip_create(const mcmcpp_hip_config* cfg, mcmcpp_hip_sampler** out)
{
    if (!out)
    {
        g_create_error = "out is NULL";
        return MCMCPP_HIP_E_ARG;
    }
    *out = nullptr;
    int rc = check_config(cfg, g_create_error);
    if (rc) return rc;
    int irc = MCMCPP_HIP_OK;
    mcmcpp_hip_sampler* h = cfg->mover == MCMCPP_HIP_MOVER_DIFFERENTIAL_EVOLUTION ? mcmcpp::make_de_sampler(*cfg, &irc)
                            : cfg->calc_id == MCMCPP_HIP_CALC_BATCH               ? mcmcpp::make_batch_sampler(*cfg, &irc)
                                                                                  : make_handle<Sampler>(*cfg, &irc);
    if (!h) return MCMCPP_HIP_E_NOMEM;
    if (irc)
    {
        g_create_error = h->error;
        delete h;
        return irc;
    }
    *out = h;
    return MCMCPP_HIP_OK;
}

void mcmcpp_hip_destroy(mcmcpp_hip_sampler* h)
{
    if (!h) return;
    // an asynchronous run still uses the arena, streams, graphs and the communicator the destructor releases: let it end first
    if (h->async_worker.joinable()) h->async_worker.join();
    h->async_active = false;
    delete h;
}

const char* mcmcpp_hip_last_error(const mcmcpp_hip_sampler* h)
{
    if (!h) return g_create_error.c_str();
    return h->refused ? h->refused : h->error.c_str();
}

#define NEED_H \
    if (!h) return MCMCPP_HIP_E_ARG
// between run_async and run_wait the handle belongs to its worker thread: only wait_stored (and destroy, which joins) may be called
#define NOT_WHILE_ASYNC(name) \
    if (h->async_active) return h->refuse("mcmcpp_hip_" name ": an asynchronous run is in progress (only wait_stored may be called before run_wait)"); \
    h->refused = nullptr

int mcmcpp_hip_set_batch_calculator(mcmcpp_hip_sampler* h, mcmcpp_hip_batch_logp_fn fn, void* user, void* device_proposals,
                                    void* device_logp)
{
    NEED_H;
    NOT_WHILE_ASYNC("set_batch_calculator");
    return h->set_batch_calculator(fn, user, device_proposals, device_logp);
}
int mcmcpp_hip_set_state(mcmcpp_hip_sampler* h, const void* positions, const void* logp)
{
    NEED_H;
    NOT_WHILE_ASYNC("set_state");
    return h->set_state(positions, logp);
}
int mcmcpp_hip_set_chain_params(mcmcpp_hip_sampler* h, int32_t chain, const void* params, int32_t len)
{
    NEED_H;
    NOT_WHILE_ASYNC("set_chain_params");
    return h->set_chain_params(chain, params, len);
}
int mcmcpp_hip_calc_logp_chain(mcmcpp_hip_sampler* h, int32_t chain, const void* pos, int64_t count, void* out)
{
    NEED_H;
    NOT_WHILE_ASYNC("calc_logp_chain");
    return h->calc_logp_chain(chain, pos, count, out);
}
int mcmcpp_hip_exchange_chains(mcmcpp_hip_sampler* h, uint64_t round, uint64_t* proposed, uint64_t* accepted, uint64_t* near_ties)
{
    NEED_H;
    NOT_WHILE_ASYNC("exchange_chains");
    return h->exchange_chains(round, proposed, accepted, near_ties);
}
int mcmcpp_hip_run_tempered(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, int64_t exchange_every, uint64_t first_round, void* chain_out,
                            uint32_t* accepted_per_step, uint64_t* proposed, uint64_t* accepted, uint64_t* near_ties, uint64_t* rounds_done)
{
    NEED_H;
    NOT_WHILE_ASYNC("run_tempered");
    return h->run_tempered(n_saved, interval, exchange_every, first_round, chain_out, accepted_per_step, proposed, accepted, near_ties, rounds_done, false);
}
int mcmcpp_hip_run_tempered_device(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, int64_t exchange_every, uint64_t first_round, void* device_chain,
                                   uint32_t* accepted_per_step, uint64_t* proposed, uint64_t* accepted, uint64_t* near_ties, uint64_t* rounds_done)
{
    NEED_H;
    NOT_WHILE_ASYNC("run_tempered_device");
    return h->run_tempered(n_saved, interval, exchange_every, first_round, device_chain, accepted_per_step, proposed, accepted, near_ties, rounds_done, true);
}
int mcmcpp_hip_evidence_ratios(mcmcpp_hip_sampler* h, const void* const* steps, int64_t n_steps, int64_t slice_interval, double* log_ratio, double* mcse, double* ess,
                               double* kish, double* max_u, int64_t* nonfinite, double* log_ratio_total, double* mcse_total, int64_t* num_draws)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_ratios");
    return h->evidence_ratios(mcmcpp::EvidenceRequest{"evidence_ratios", steps, nullptr, false, 0, n_steps, slice_interval,
                                                      mcmcpp::EvidenceOutputs{log_ratio, mcse, ess, kish, max_u, nonfinite, log_ratio_total, mcse_total, num_draws}});
}
int mcmcpp_hip_evidence_ratios_device(mcmcpp_hip_sampler* h, const void* device_steps, int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval,
                                      double* log_ratio, double* mcse, double* ess, double* kish, double* max_u, int64_t* nonfinite, double* log_ratio_total,
                                      double* mcse_total, int64_t* num_draws)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_ratios_device");
    return h->evidence_ratios(mcmcpp::EvidenceRequest{"evidence_ratios_device", nullptr, device_steps, true, chain_stride_steps, n_steps, slice_interval,
                                                      mcmcpp::EvidenceOutputs{log_ratio, mcse, ess, kish, max_u, nonfinite, log_ratio_total, mcse_total, num_draws}});
}
int mcmcpp_hip_evidence_bridge(mcmcpp_hip_sampler* h, const void* const* steps, int64_t n_steps, int64_t slice_interval, double* log_ratio, double* mcse,
                               double* overlap, double* ess, int64_t* passes, int64_t* converged, int64_t* nonfinite, double* log_ratio_total, double* mcse_total,
                               int64_t* num_draws)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_bridge");
    return h->evidence_bridge(mcmcpp::BridgeRequest{mcmcpp::EvidenceRequest{"evidence_bridge", steps, nullptr, false, 0, n_steps, slice_interval, mcmcpp::EvidenceOutputs{}},
                                                    mcmcpp::BridgeOutputs{log_ratio, mcse, overlap, ess, passes, converged, nonfinite, log_ratio_total, mcse_total, num_draws}});
}
int mcmcpp_hip_evidence_bridge_device(mcmcpp_hip_sampler* h, const void* device_steps, int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval,
                                      double* log_ratio, double* mcse, double* overlap, double* ess, int64_t* passes, int64_t* converged, int64_t* nonfinite,
                                      double* log_ratio_total, double* mcse_total, int64_t* num_draws)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_bridge_device");
    return h->evidence_bridge(
        mcmcpp::BridgeRequest{mcmcpp::EvidenceRequest{"evidence_bridge_device", nullptr, device_steps, true, chain_stride_steps, n_steps, slice_interval, mcmcpp::EvidenceOutputs{}},
                              mcmcpp::BridgeOutputs{log_ratio, mcse, overlap, ess, passes, converged, nonfinite, log_ratio_total, mcse_total, num_draws}});
}
int mcmcpp_hip_evidence_mbar(mcmcpp_hip_sampler* h, const void* const* steps, int64_t n_steps, int64_t slice_interval, double* log_z, double* cov, double* log_ratio,
                             double* mcse, double* ess, int64_t* nonfinite, double* log_ratio_total, double* mcse_total, int64_t* passes, int64_t* converged,
                             int64_t* num_draws)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_mbar");
    return h->evidence_mbar(mcmcpp::MbarRequest{mcmcpp::EvidenceRequest{"evidence_mbar", steps, nullptr, false, 0, n_steps, slice_interval, mcmcpp::EvidenceOutputs{}},
                                                mcmcpp::MbarOutputs{log_z, cov, log_ratio, mcse, ess, nonfinite, log_ratio_total, mcse_total, passes, converged, num_draws}});
}
int mcmcpp_hip_evidence_mbar_device(mcmcpp_hip_sampler* h, const void* device_steps, int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval, double* log_z,
                                    double* cov, double* log_ratio, double* mcse, double* ess, int64_t* nonfinite, double* log_ratio_total, double* mcse_total,
                                    int64_t* passes, int64_t* converged, int64_t* num_draws)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_mbar_device");
    return h->evidence_mbar(
        mcmcpp::MbarRequest{mcmcpp::EvidenceRequest{"evidence_mbar_device", nullptr, device_steps, true, chain_stride_steps, n_steps, slice_interval, mcmcpp::EvidenceOutputs{}},
                            mcmcpp::MbarOutputs{log_z, cov, log_ratio, mcse, ess, nonfinite, log_ratio_total, mcse_total, passes, converged, num_draws}});
}
int mcmcpp_hip_evidence_gaussian(mcmcpp_hip_sampler* h, int32_t chain, const void* const* steps, int64_t n_steps, int64_t slice_interval, const double* mean,
                                 const double* chol, uint64_t seed, uint64_t stream, double* log_evidence, double* mcse, double* overlap, double* ess, int64_t* passes,
                                 int64_t* converged, int64_t* nonfinite, int64_t* num_draws, void* proposals, double* log_q)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_gaussian");
    return h->evidence_gaussian(mcmcpp::GaussianBridgeRequest{
        mcmcpp::EvidenceRequest{"evidence_gaussian", steps, nullptr, false, 0, n_steps, slice_interval, mcmcpp::EvidenceOutputs{}}, chain, mean, chol, seed, stream,
        mcmcpp::GaussianBridgeOutputs{log_evidence, mcse, overlap, ess, passes, converged, nonfinite, num_draws, proposals, log_q}});
}
int mcmcpp_hip_evidence_gaussian_device(mcmcpp_hip_sampler* h, int32_t chain, const void* device_steps, int64_t n_steps, int64_t slice_interval, const double* mean,
                                        const double* chol, uint64_t seed, uint64_t stream, double* log_evidence, double* mcse, double* overlap, double* ess,
                                        int64_t* passes, int64_t* converged, int64_t* nonfinite, int64_t* num_draws, void* proposals, double* log_q)
{
    NEED_H;
    NOT_WHILE_ASYNC("evidence_gaussian_device");
    return h->evidence_gaussian(mcmcpp::GaussianBridgeRequest{
        mcmcpp::EvidenceRequest{"evidence_gaussian_device", nullptr, device_steps, true, 0, n_steps, slice_interval, mcmcpp::EvidenceOutputs{}}, chain, mean, chol, seed,
        stream, mcmcpp::GaussianBridgeOutputs{log_evidence, mcse, overlap, ess, passes, converged, nonfinite, num_draws, proposals, log_q}});
}
int mcmcpp_hip_run(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step)
{
    NEED_H;
    NOT_WHILE_ASYNC("run");
    return h->run(n_saved, interval, chain_out, accepted_per_step);
}
int mcmcpp_hip_run_device(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* device_chain, uint32_t* accepted_per_step)
{
    NEED_H;
    NOT_WHILE_ASYNC("run_device");
    return h->run_device(n_saved, interval, device_chain, accepted_per_step);
}
int mcmcpp_hip_calc_logp_device(mcmcpp_hip_sampler* h, int32_t chain, const void* device_positions, int64_t count, void* device_logp_out)
{
    NEED_H;
    NOT_WHILE_ASYNC("calc_logp_device");
    return h->calc_logp_device(chain, device_positions, count, device_logp_out);
}
// run_async / run_device_async: the run on the handle's worker thread
static int start_async_run(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step, bool to_device)
{
    NEED_H;
    if (h->async_active)
        return h->refuse(to_device ? "mcmcpp_hip_run_device_async: the previous asynchronous run has not been waited for (mcmcpp_hip_run_wait)"
                                   : "mcmcpp_hip_run_async: the previous asynchronous run has not been waited for (mcmcpp_hip_run_wait)");
    h->refused = nullptr;
    {
        std::lock_guard<std::mutex> lock(h->async_mutex);
        h->async_stored = 0;
        h->async_done = false;
        h->async_rc = MCMCPP_HIP_OK;
    }
    h->async_active = true;
    try
    {
        h->async_worker = std::thread([=]() {
            const int rc = to_device ? h->run_device(n_saved, interval, chain_out, accepted_per_step) : h->run(n_saved, interval, chain_out, accepted_per_step);
            {
                std::lock_guard<std::mutex> lock(h->async_mutex);
                h->async_rc = rc;
                h->async_done = true;
                if (rc == MCMCPP_HIP_OK && chain_out) h->async_stored = n_saved;  // (whatever the sampler announced on the way)
            }
            h->async_cv.notify_all();
        });
    }
    catch (...)
    {
        h->async_active = false;
        h->async_done = true;
        return h->fail(MCMCPP_HIP_E_NOMEM, "run_async: cannot start the worker thread");
    }
    return MCMCPP_HIP_OK;
}
int mcmcpp_hip_run_async(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step)
{
    return start_async_run(h, n_saved, interval, chain_out, accepted_per_step, false);
}
int mcmcpp_hip_run_device_async(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* device_chain, uint32_t* accepted_per_step)
{
    return start_async_run(h, n_saved, interval, device_chain, accepted_per_step, true);
}
int mcmcpp_hip_wait_stored(mcmcpp_hip_sampler* h, int64_t count)
{
    NEED_H;
    if (!h->async_active) return h->fail(MCMCPP_HIP_E_STATE, "wait_stored: no asynchronous run in progress");
    std::unique_lock<std::mutex> lock(h->async_mutex);
    h->async_cv.wait(lock, [&]() { return h->async_stored >= count || h->async_done; });
    if (h->async_stored >= count) return MCMCPP_HIP_OK;
    return h->async_rc != MCMCPP_HIP_OK ? h->async_rc : MCMCPP_HIP_E_ARG;  // the run ended without storing that many steps
}
int mcmcpp_hip_run_wait(mcmcpp_hip_sampler* h)
{
    NEED_H;
    if (!h->async_active) return h->fail(MCMCPP_HIP_E_STATE, "run_wait: no asynchronous run in progress");
    if (h->async_worker.joinable()) h->async_worker.join();
    h->async_active = false;
    h->refused = nullptr;
    return h->async_rc;
}
void* mcmcpp_hip_host_alloc(uint64_t bytes)
{
    void* p = nullptr;
    // (portable: usable from every device of the process, whichever one happens to be current on the calling thread --
    //  the facade's Chain obtains blocks on a helper thread that has never selected a device)
    if (hipHostMalloc(&p, bytes ? (size_t)bytes : 64, hipHostMallocPortable) != hipSuccess)
    {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void mcmcpp_hip_host_free(void* p) { mcmcpp::free_pinned(p); }
int mcmcpp_hip_get_state(mcmcpp_hip_sampler* h, void* positions, void* logp, uint32_t* n_accept)
{
    NEED_H;
    NOT_WHILE_ASYNC("get_state");
    return h->get_state(positions, logp, n_accept);
}
int mcmcpp_hip_seek(mcmcpp_hip_sampler* h, uint64_t ensemble_steps_done)
{
    NEED_H;
    NOT_WHILE_ASYNC("seek");
    return h->seek(ensemble_steps_done);
}
int mcmcpp_hip_reset_counters(mcmcpp_hip_sampler* h)
{
    NEED_H;
    NOT_WHILE_ASYNC("reset_counters");
    return h->reset_counters();
}
int mcmcpp_hip_get_counters(mcmcpp_hip_sampler* h, uint64_t* accepted, uint64_t* ensemble_steps, uint64_t* near_ties,
                            uint64_t* redraws)
{
    NEED_H;
    NOT_WHILE_ASYNC("get_counters");
    return h->get_counters(accepted, ensemble_steps, near_ties, redraws);
}
int mcmcpp_hip_calc_logp(mcmcpp_hip_sampler* h, const void* positions, int64_t count, void* logp_out)
{
    NEED_H;
    NOT_WHILE_ASYNC("calc_logp");
    return h->calc_logp(positions, count, logp_out);
}
int mcmcpp_hip_last_run_timing(mcmcpp_hip_sampler* h, double* gpu_ms, int64_t* step_launches)
{
    NEED_H;
    return h->last_run_timing(gpu_ms, step_launches);
}
int mcmcpp_hip_last_run_host_timing(mcmcpp_hip_sampler* h, double* enqueue_ms, double* wall_ms, double* exchange_us_per_step)
{
    NEED_H;
    if (enqueue_ms) *enqueue_ms = h->host_enqueue_ms;
    if (wall_ms) *wall_ms = h->host_wall_ms;
    if (exchange_us_per_step) *exchange_us_per_step = h->exchange_us_per_step;
    return MCMCPP_HIP_OK;
}
int mcmcpp_hip_last_run_exchange(mcmcpp_hip_sampler* h, double* bytes_per_step, int64_t* repeated_chunks, int64_t* block_slots)
{
    NEED_H;
    if (bytes_per_step) *bytes_per_step = h->xchg_bytes_per_step;
    if (repeated_chunks) *repeated_chunks = h->xchg_rollbacks;
    if (block_slots) *block_slots = h->xchg_cap_slots;
    return MCMCPP_HIP_OK;
}
int mcmcpp_hip_comm_unique_id(void* id_out)
{
    if (!id_out)
    {
        g_create_error = "comm_unique_id: id_out is NULL";
        return MCMCPP_HIP_E_ARG;
    }
    std::string why;
    const Rccl* r = Rccl::get(&why);
    if (!r)
    {
        g_create_error = why;
        return MCMCPP_HIP_E_COMM;
    }
    ncclUniqueId id;
    const ncclResult_t rc = r->GetUniqueId(&id);
    if (rc != ncclSuccess)
    {
        g_create_error = std::string("ncclGetUniqueId failed: ") + r->GetErrorString(rc);
        return MCMCPP_HIP_E_COMM;
    }
    std::memcpy(id_out, &id, sizeof id);
    return MCMCPP_HIP_OK;
}
int mcmcpp_hip_half_step_async(mcmcpp_hip_sampler* h, int32_t color, int64_t save_slot)
{
    NEED_H;
    NOT_WHILE_ASYNC("half_step_async");
    return h->half_step_async(color, save_slot);
}
int mcmcpp_hip_bind_device_chain(mcmcpp_hip_sampler* h, void* device_chain, int64_t slots)
{
    NEED_H;
    NOT_WHILE_ASYNC("bind_device_chain");
    return h->bind_device_chain(device_chain, slots);
}
void* mcmcpp_hip_device_positions(mcmcpp_hip_sampler* h) { return h ? h->device_positions() : nullptr; }
int mcmcpp_hip_shard_span(mcmcpp_hip_sampler* h, int32_t color, int64_t* offset_elems, int64_t* count_elems)
{
    NEED_H;
    NOT_WHILE_ASYNC("shard_span");
    return h->shard_span(color, offset_elems, count_elems);
}
int mcmcpp_hip_synchronize(mcmcpp_hip_sampler* h)
{
    NEED_H;
    NOT_WHILE_ASYNC("synchronize");
    return h->synchronize();
}
}
