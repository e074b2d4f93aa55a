// split_exchange.hpp -- the exchange side of a handle that is one rank of a split ensemble (BASELINE config 5): the RCCL
// communicator and every buffer only split runs use, and the operations Sampler::run_split (mcmcpp_hip.hip) enqueues
// between its step launches.  Everything goes onto the handle's launch stream; nothing here waits for the device except
// agree_on_status and read_stats, which say so.  Stepping stays with the sampler, the schedule of a run with SplitWindow
// (run_plan.hpp), the geometry of the moved-rows kernels with exchange_plan.hpp.
//
// Two schemes.  Whole slices: every exchange all-gathers the slices of the updated colour(s) in place (every rank's slice
// sits where the gather puts it).  Moved rows only (StepPlan::compact_exchange, exchange_kernels.hpp): pack -> one
// all-gather of equal blocks of `cap` slots -> scatter into the replica; a block that was too small raises the overflow
// flag of the statistics record, and the sampler rolls the chunk back to the snapshot taken in front of it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "exchange_kernels.hpp"
#include "rccl_dyn.hpp"
#include "run_plan.hpp"
#include "sampler_base.hpp"

#define NCCL_TRY(expr)                                                                                          \
    do                                                                                                          \
    {                                                                                                           \
        ncclResult_t r_ = (expr);                                                                               \
        if (r_ != ncclSuccess) return fail(MCMCPP_HIP_E_COMM, "%s failed: %s", #expr, rccl->GetErrorString(r_)); \
    } while (0)

namespace mcmcpp
{
// What the exchanges work on: the sampler's replica of the ensemble and where this rank's slice lies in it.  The sampler
// fills it in once its buffers exist; it owns all of them.
template <class T>
struct SplitReplica
{
    mcmcpp_hip_sampler* owner = nullptr;  // carries the error message of a failed call
    int device = -1;
    hipStream_t stream = nullptr;
    int W = 0, D = 0, n = 0, shard_begin = 0, shard_count = 0;
    bool full_step = false;  // full-step kernels: two position and log-posterior buffers, one exchange per ensemble step
    bool compact = false;    // the exchanges carry moved rows only
    T *pos = nullptr, *pos_alt = nullptr, *logp = nullptr;  // (the second log-posterior buffer is logp + W)
    uint32_t* nacc = nullptr;
    Diag* diag = nullptr;
};

template <class T>
class SplitExchange : SplitReplica<T>
{
    using R = SplitReplica<T>;
    using R::owner, R::device, R::stream, R::W, R::D, R::n, R::shard_begin, R::shard_count, R::full_step, R::compact, R::pos, R::pos_alt, R::logp, R::nacc, R::diag;

public:
    SplitExchange() = default;
    SplitExchange(const SplitExchange&) = delete;
    SplitExchange& operator=(const SplitExchange&) = delete;
    // (the handle has quiesced its stream; the buffers free themselves behind this)
    ~SplitExchange()
    {
        if (own_comm && comm && rccl) (void)rccl->CommDestroy(comm);
    }

    bool active() const { return comm != nullptr; }
    uint32_t cap_learned = 0;  // moved rows: the slot bound the last run ended with (SplitWindow learns it)

    // the caller's communicator, or one of the handle's own from the caller's id (no communicator configured: nothing)
    int open(mcmcpp_hip_sampler* owner_, const mcmcpp_hip_config& c)
    {
        owner = owner_;
        if (c.comm_world < 1) return MCMCPP_HIP_OK;
        rank = c.comm_rank;
        world = c.comm_world;
        std::string why;
        rccl = Rccl::get(&why);
        if (!rccl) return fail(MCMCPP_HIP_E_COMM, "%s", why.c_str());
        if (c.comm)
        {
            comm = static_cast<ncclComm_t>(c.comm);
            int cnt = -1, rk = -1;
            NCCL_TRY(rccl->CommCount(comm, &cnt));
            NCCL_TRY(rccl->CommUserRank(comm, &rk));
            if (cnt != c.comm_world || rk != c.comm_rank)
                return fail(MCMCPP_HIP_E_ARG, "the communicator is rank %d of %d, the config says %d of %d", rk, cnt, c.comm_rank, c.comm_world);
        }
        else
        {
            ncclUniqueId id;
            static_assert(sizeof(id) == MCMCPP_HIP_COMM_ID_BYTES, "mcmcpp_hip.h states the size of an RCCL id");
            std::memcpy(&id, c.comm_id, sizeof id);
            NCCL_TRY(rccl->CommInitRank(&comm, c.comm_world, id, c.comm_rank));
            own_comm = true;
        }
        return MCMCPP_HIP_OK;
    }

    // a block of the compact exchange that holds every walker of an exchange
    static uint32_t cap_full_of(bool full_step_, int shard_count_) { return (uint32_t)((full_step_ ? 2 : 1) * shard_count_); }
    uint32_t cap_full() const { return cap_full_of(full_step, shard_count); }

    // the buffers of a rank, sized by the replica (no communicator: none)
    int allocate(const SplitReplica<T>& replica)
    {
        static_cast<R&>(*this) = replica;
        if (!active()) return MCMCPP_HIP_OK;
        HIP_TRY(d_status.alloc(8 * sizeof(uint64_t)));
        HIP_TRY(h_words.alloc(sizeof(HostWords)));
        if (compact)
        {
            snap.logp = sizeof(T) * (size_t)W * D;
            snap.nacc = snap.logp + sizeof(T) * (size_t)W;
            snap.diag = snap.nacc + sizeof(uint32_t) * (size_t)W;
            HIP_TRY(d_xblocks.alloc(xblock_bytes<T>(cap_full(), D) * (size_t)world));
            HIP_TRY(d_seen.alloc(sizeof(uint32_t) * (size_t)W));
            HIP_TRY(d_xstats.alloc(sizeof(XStats)));
            HIP_TRY(d_snap.alloc(snap.diag + sizeof(Diag)));
        }
        return MCMCPP_HIP_OK;
    }

    // what a run needs beyond that: the pinned staging of `stage_bytes` of stored steps (0: this rank stores nothing), the
    // events around the sampled exchanges
    int prepare_run(size_t stage_bytes)
    {
        if (grow(h_stage, stage_bytes, stream)) return fail(MCMCPP_HIP_E_NOMEM, "run: cannot allocate %zu bytes of pinned staging", stage_bytes);
        if (ev_x.empty())
        {
            ev_x.resize(2 * kSplitMaxSamples);
            for (Event& e : ev_x) HIP_TRY(hipEventCreate(e.replace()));
        }
        return MCMCPP_HIP_OK;
    }
    char* stage() const { return h_stage; }

    // Every rank learns the worst status among the ranks (and that all were asked for the same number of steps) before any
    // of them launches or exchanges anything: a rank that failed its preparation would otherwise leave the others waiting
    // in their first all-gather for good.  One small all-reduce and one stream synchronisation per run.
    int agree_on_status(int local_rc, int64_t total, int32_t interval, bool stores, bool* any_rank_stores)
    {
        uint64_t* out = h_words->status_out;
        const uint64_t* back = h_words->status_back;
        out[0] = (uint64_t)local_rc;
        out[1] = (uint64_t)total;
        out[2] = ~(uint64_t)total;
        out[3] = (uint64_t)(uint32_t)interval;
        out[4] = ~(uint64_t)(uint32_t)interval;
        out[5] = stores ? 1u : 0u;  // (stored steps are handed out a staging buffer at a time: where the chunks of the run end)
        const std::string mine = owner->error;
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemcpyAsync(d_status, out, 6 * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        NCCL_TRY(rccl->AllReduce(d_status, d_status, 6, ncclUint64, ncclMax, comm, stream));
        HIP_TRY(hipMemcpyAsync(h_words->status_back, d_status, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (local_rc != MCMCPP_HIP_OK)
        {
            owner->error = mine;
            return local_rc;
        }
        if (back[0] != 0) return fail((int)back[0], "run: the preparation of another rank of the split ensemble failed (code %d); nothing was launched", (int)back[0]);
        if (back[1] != ~back[2] || back[3] != ~back[4])
            return fail(MCMCPP_HIP_E_ARG, "run: the ranks of the split ensemble were asked for different numbers of steps or intervals; nothing was launched");
        *any_rank_stores = back[5] != 0;
        return MCMCPP_HIP_OK;
    }

    // the start of a run, behind the sampler's: moved rows with two buffers -- a remote walker's row must be current in BOTH
    // (the scatter keeps it so from here on)
    int begin_run()
    {
        if (!(compact && full_step)) return MCMCPP_HIP_OK;
        HIP_TRY(hipMemcpyAsync(pos_alt, pos, sizeof(T) * (size_t)W * D, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(logp + W, logp, sizeof(T) * (size_t)W, hipMemcpyDeviceToDevice, stream));
        return MCMCPP_HIP_OK;
    }

    // The start of a chunk that exchanges moved rows (whole slices: nothing): everything a repeated try must find as this one
    // found it goes to the snapshot (in_alt: the second buffers hold the ensemble now), the exchange starts from nothing seen.
    int begin_chunk(bool in_alt, uint32_t cap)
    {
        if (!compact) return MCMCPP_HIP_OK;
        if (int rc = snapshot(in_alt ? pos_alt : pos, in_alt ? logp + W : logp)) return rc;
        return exchange_reset(cap);
    }

    // Colours [c0, c0 + k) of this rank's slice, as the step that left the ensemble in the first (in_alt: second) buffers
    // updated them, reach every rank.  sample >= 0: the exchange is timed by the events of that sample slot.
    int exchange(bool in_alt, int c0, int k, uint32_t cap, int sample)
    {
        T* cur_pos = in_alt ? pos_alt : pos;
        T* cur_logp = in_alt ? logp + W : logp;
        if (sample >= 0) HIP_TRY(hipEventRecord(ev_x[2 * sample], stream));
        int rc;
        if (compact)
            rc = full_step ? exchange_compact(cur_pos, in_alt ? pos : pos_alt, cur_logp, in_alt ? logp : logp + W, c0, k, cap)
                           : exchange_compact(cur_pos, nullptr, cur_logp, nullptr, c0, k, cap);
        else
            rc = exchange_rows(cur_pos, full_step ? cur_logp : nullptr, c0, k);  // (the half-step scheme gathers the log-posteriors at the end)
        if (rc) return rc;
        if (sample >= 0) HIP_TRY(hipEventRecord(ev_x[2 * sample + 1], stream));
        return MCMCPP_HIP_OK;
    }

    // The end of a chunk of moved rows: the statistics of its exchanges.  Waits for the stream.
    int read_stats(XStats* out)
    {
        XStats* hx = &h_words->xstats;
        HIP_TRY(hipMemcpyAsync(hx, d_xstats, sizeof(XStats), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        *out = *hx;
        return MCMCPP_HIP_OK;
    }

    // the snapshot back -- into both buffers, so that the repeated chunk may start at the first like a run does
    int rollback()
    {
        HIP_TRY(hipMemcpyAsync(pos, d_snap, snap.logp, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(logp, d_snap + snap.logp, sizeof(T) * (size_t)W, hipMemcpyDeviceToDevice, stream));
        if (full_step)
        {
            HIP_TRY(hipMemcpyAsync(pos_alt, d_snap, snap.logp, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(logp + W, d_snap + snap.logp, sizeof(T) * (size_t)W, hipMemcpyDeviceToDevice, stream));
        }
        HIP_TRY(hipMemcpyAsync(nacc, d_snap + snap.nacc, sizeof(uint32_t) * (size_t)W, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(diag, d_snap + snap.diag, sizeof(Diag), hipMemcpyDeviceToDevice, stream));
        return MCMCPP_HIP_OK;
    }

    // The end of a run: every rank ends it with the whole ensemble's log-posteriors and accepted counters (get_state is then
    // the same on all ranks), and with the ensemble-wide accepted counts per step
    int finish_run(uint32_t* d_acc, int64_t total)
    {
        NCCL_TRY(rccl->GroupStart());
        for (int c = 0; c < 2; ++c)
        {
            if (!full_step && !compact)  // (the exchanges of the other schemes carry the log-posteriors along)
                NCCL_TRY(rccl->AllGather(logp + (size_t)c * n + shard_begin, logp + (size_t)c * n, (size_t)shard_count, RcclType<T>::value, comm, stream));
            NCCL_TRY(rccl->AllGather(nacc + (size_t)c * n + shard_begin, nacc + (size_t)c * n, (size_t)shard_count, ncclUint32, comm, stream));
        }
        NCCL_TRY(rccl->AllReduce(d_acc, d_acc, (size_t)total, ncclUint32, ncclSum, comm, stream));
        NCCL_TRY(rccl->GroupEnd());
        return MCMCPP_HIP_OK;
    }

    // microseconds of exchanges per ensemble step, from the `samples` timed ones (the stream is idle)
    int exchange_us_per_step(int samples, double* us)
    {
        float ms = 0.f;
        double sum = 0.0;
        for (int k = 0; k < samples; ++k)
        {
            HIP_TRY(hipEventElapsedTime(&ms, ev_x[2 * k], ev_x[2 * k + 1]));
            sum += ms;
        }
        // (half-step scheme: the sampled exchange is the red one, the black one moves as much)
        *us = samples ? sum / samples * 1e3 * (full_step ? 1.0 : 2.0) : 0.0;
        return MCMCPP_HIP_OK;
    }

private:
    template <class... A>
    int fail(int code, const char* fmt, A... a)
    {
        return owner->fail(code, fmt, a...);
    }

    // whole slices: the updated rows (and, with logp_buf, log-posteriors) of colours [first_color, first_color + colors)
    int exchange_rows(T* pos_buf, T* logp_buf, int first_color, int colors)
    {
        NCCL_TRY(rccl->GroupStart());
        for (int c = first_color; c < first_color + colors; ++c)
        {
            T* half = pos_buf + (size_t)c * n * D;
            NCCL_TRY(rccl->AllGather(half + (size_t)shard_begin * D, half, (size_t)shard_count * D, RcclType<T>::value, comm, stream));
            if (logp_buf)
            {
                T* lh = logp_buf + (size_t)c * n;
                NCCL_TRY(rccl->AllGather(lh + shard_begin, lh, (size_t)shard_count, RcclType<T>::value, comm, stream));
            }
        }
        NCCL_TRY(rccl->GroupEnd());
        return MCMCPP_HIP_OK;
    }

    // moved rows: pack -> one all-gather of `world` equal blocks of `cap` slots -> scatter into the replica (both position
    // buffers when `other_pos` is given).  Colours [color0, color0 + colors) of this rank's slice.
    int exchange_compact(T* cur_pos, T* other_pos, T* cur_logp, T* other_logp, int color0, int colors, uint32_t cap)
    {
        const size_t bb = xblock_bytes<T>(cap, D);
        char* own = d_xblocks + bb * (size_t)rank;
        hipLaunchKernelGGL(exchange_pack_kernel<T>, dim3(exchange_pack_blocks(colors * shard_count)), dim3(kPackThreads), 0, stream, (const T*)cur_pos, (const T*)cur_logp,
                           (const uint32_t*)nacc, d_seen, own, cap, n, D, shard_begin, shard_count, color0, colors);
        HIP_TRY(hipGetLastError());
        NCCL_TRY(rccl->AllGather(own, d_xblocks, bb, ncclInt8, comm, stream));
        const XScatterGrid grid = exchange_scatter_grid(cap, D, sizeof(T), world);
        hipLaunchKernelGGL(exchange_scatter_kernel<T>, dim3(grid.x, grid.y), dim3(kScatterThreads), 0, stream,
                           d_xblocks, bb, cap, world, rank, D, cur_pos, other_pos, cur_logp, other_logp, d_xstats);
        HIP_TRY(hipGetLastError());
        return MCMCPP_HIP_OK;
    }

    // (seen counters of the own slice <- accepted counters; statistics and the own block's count <- 0)
    int exchange_reset(uint32_t cap)
    {
        hipLaunchKernelGGL(exchange_sync_seen_kernel, dim3(exchange_sync_seen_blocks(shard_count)), dim3(kSyncSeenThreads), 0, stream, (const uint32_t*)nacc, d_seen, n,
                           shard_begin, shard_count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(d_xstats, 0, sizeof(XStats), stream));
        HIP_TRY(hipMemsetAsync(d_xblocks + xblock_bytes<T>(cap, D) * (size_t)rank, 0, sizeof(XBlockHeader), stream));
        return MCMCPP_HIP_OK;
    }

    // d_snap <- cur_pos, cur_logp (the buffers that hold the ensemble now), the accepted counters, the diagnostics
    int snapshot(const T* cur_pos, const T* cur_logp)
    {
        HIP_TRY(hipMemcpyAsync(d_snap, cur_pos, snap.logp, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_snap + snap.logp, cur_logp, sizeof(T) * (size_t)W, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_snap + snap.nacc, nacc, sizeof(uint32_t) * (size_t)W, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_snap + snap.diag, diag, sizeof(Diag), hipMemcpyDeviceToDevice, stream));
        return MCMCPP_HIP_OK;
    }

    // pinned words on their way to the device and back; a slot is rewritten only behind the synchronisation that read it
    struct HostWords
    {
        uint64_t status_out[6];   // agree_on_status: the words every rank all-reduces
        uint64_t status_back[6];  // ... and what comes back
        XStats xstats;            // the exchange statistics of the chunk in hand
    };

    const Rccl* rccl = nullptr;
    ncclComm_t comm = nullptr;
    bool own_comm = false;
    int rank = 0, world = 0;
    DeviceBuffer<uint64_t> d_status;  // the status words the ranks agree on
    PinnedBuffer<HostWords> h_words;
    PinnedBuffer<char> h_stage;       // pinned staging of stored steps
    std::vector<Event> ev_x;          // events around a sample of exchanges
    // moved rows only
    DeviceBuffer<char> d_xblocks;     // [world][block]: this rank's block and, behind the all-gather, everybody's
    DeviceBuffer<uint32_t> d_seen;    // [W]: a walker's accepted counter as of the last exchange (own slice)
    DeviceBuffer<XStats> d_xstats;
    DeviceBuffer<char> d_snap;        // positions | log-posteriors | counters | diagnostics in front of the chunk in hand
    struct { size_t logp, nacc, diag; } snap = {};  // byte offsets into d_snap (the positions are at 0)
};
}  // namespace mcmcpp
