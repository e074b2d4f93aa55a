// run_plan.hpp -- how a run() delivers its stored steps and cuts itself into chunks: ring size, chunk lengths, when the host
// must wait, where a sub-chunk lands in the caller's array, what a destination in device memory changes (run_device: no ring,
// no staging, what wait_stored may hear), the pieces of a differential-evolution run and the sub-chunks of a batch run, where
// a split run cuts so that every rank cuts alike, and the slot bound of its exchange blocks.  Pure functions and a few small
// value types over plain numbers: ChainPlan, PiecePlan, and the windows that keep the state of a run's host loop --
// ChunkWindow (what the next two share), DeviceWindow, TrickleWindow, and SplitWindow, the whole schedule of a split run
// (chunks, slot bound, roll-backs, staging, sampled exchanges, statistics).  No HIP header: this file compiles with the
// host compiler alone, and tests/test_run_plan.py, tests/test_device_chain_plan.py and tests/test_run_entry.py check the
// schedules there, case by case and over simulated runs.  The samplers keep every HIP and RCCL call and ask here for the
// numbers.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mcmcpp
{
// Stored steps per sub-chunk of a run: what `budget` bytes of device chain hold, at most an eighth of the run (the last
// host copy, which nothing overlaps, stays short, and a run_async caller sees progress), at least one
inline int64_t stored_steps_per_subchunk(size_t budget, size_t stored_step_bytes, int64_t n_saved)
{
    int64_t s = (int64_t)(budget / stored_step_bytes);
    const int64_t eighth = (n_saved + 7) / 8;
    if (s > eighth) s = eighth;
    if (s < 1) s = 1;
    return s;
}

// ---- chain delivery of a whole-ensemble run (Sampler::run_whole) -------------------------------------------------------
// Nothing: no chain_out, the steps run as one sub-chunk.  Subchunks: device chain halves -> pinned staging -> chain_out.
// Trickle: the full-step launches forward stored steps themselves (trickle_stored_step) through a ring of `ring` slots on
// the device -- into its pinned twin, or, when chain_out is pinned memory, straight into their final place (`direct`).
// Device: the destination is the caller's device memory (run_device).  The launch that makes a stored step writes it to its
// final place: no ring, no staging, no sub-chunks, nothing forwarded, whichever kernels step the handle.
enum class ChainMode { Nothing, Subchunks, Trickle, Device };

struct ChainRequest
{
    size_t step_bytes;       // one stored step of one chain
    int chains;              // K
    int64_t n_saved;
    int32_t interval;
    bool chain_out, want_accepted;
    bool full_step;          // a full-step kernel steps the handle
    size_t subchunk_bytes;   // MCMCPP_HIP_CHAIN_SUBCHUNK_MB in bytes
    int graph_steps;         // StepPlan::graph_steps
    long trickle, pinned_direct;  // the knobs
    bool device_dest;        // chain_out is device memory of the handle's device (run_device)
};

inline ChainMode chain_mode(const ChainRequest& r)
{
    if (!r.chain_out) return ChainMode::Nothing;
    if (r.device_dest) return ChainMode::Device;
    return r.full_step && r.step_bytes % 16 == 0 && r.trickle != 0 ? ChainMode::Trickle : ChainMode::Subchunks;
}
// Is it worth asking the runtime whether chain_out is pinned memory?  (The answer goes into plan_chain.)
inline bool pinned_question_matters(const ChainRequest& r) { return chain_mode(r) == ChainMode::Trickle && r.pinned_direct != 0; }

struct StoredRange { int64_t from, to; };  // stored steps [from, to)

struct ChainPlan
{
    int64_t n_saved;
    ChainMode mode;
    bool direct;                      // Trickle, straight into a pinned chain_out
    int64_t sub_saved, n_sub;         // stored steps per sub-chunk, sub-chunks (Trickle: none)
    int64_t ring, chunk_steps;        // Trickle: ring slots (a power of two); Trickle, Device: ensemble steps per chunk
    size_t acc_entries, half_bytes, ring_bytes;  // ensure_run_buffers
    bool need_host_ring;
    int64_t slice_bytes;              // RunInfo::slice_bytes: what one launch forwards of a stored step, low bit = direct

    // the stored steps of sub-chunk c
    StoredRange subchunk(int64_t c) const
    {
        const int64_t first = c * sub_saved;
        return {first, n_saved - first < sub_saved ? n_saved : first + sub_saved};
    }
};

inline ChainPlan plan_chain(const ChainRequest& r, bool chain_out_pinned)
{
    ChainPlan p = {};
    p.n_saved = r.n_saved;
    p.mode = chain_mode(r);
    p.direct = pinned_question_matters(r) && chain_out_pinned;
    p.sub_saved = r.chain_out && p.mode != ChainMode::Device ? stored_steps_per_subchunk(r.subchunk_bytes, r.step_bytes * (size_t)r.chains, r.n_saved) : r.n_saved;
    if (p.mode == ChainMode::Device)
    {
        // Nothing has to be handed out, so a chunk only bounds how far the host enqueues ahead and how often wait_stored
        // hears of progress: a graph replay's worth of steps, in whole intervals (a chunk ends on a stored step), at least one
        int64_t per_chunk = (r.graph_steps > 0 ? r.graph_steps : 64) / (int64_t)r.interval;
        if (per_chunk < 1) per_chunk = 1;
        p.chunk_steps = per_chunk * r.interval;
    }
    else if (p.mode == ChainMode::Trickle)
    {
        p.ring = 4;
        while (p.ring < 64 && (size_t)(2 * p.ring) * r.step_bytes <= 2 * r.subchunk_bytes) p.ring *= 2;
        // the host enqueues one chunk ahead of the one it waits for: stored steps of two chunks are in flight
        int64_t per_chunk = (r.graph_steps > 0 ? r.graph_steps : 64) / (int64_t)r.interval;
        if (!p.direct && per_chunk > (p.ring - 2) / 2) per_chunk = (p.ring - 2) / 2;
        if (per_chunk < 1) per_chunk = 1;
        p.chunk_steps = per_chunk * r.interval;
        p.ring_bytes = r.step_bytes * (size_t)p.ring * (size_t)r.chains;
        p.slice_bytes = (int64_t)(((r.step_bytes + (size_t)r.interval - 1) / (size_t)r.interval + 15) / 16 * 16) | (p.direct ? 1 : 0);
    }
    else
    {
        p.n_sub = (r.n_saved + p.sub_saved - 1) / p.sub_saved;
        if (r.chain_out) p.half_bytes = r.step_bytes * (size_t)p.sub_saved * (size_t)r.chains;
    }
    p.acc_entries = r.want_accepted ? (size_t)(r.n_saved * (int64_t)r.interval) * (size_t)r.chains : 0;
    p.need_host_ring = !p.direct && p.mode != ChainMode::Device;
    return p;
}

// ---- a device destination (run_device) ---------------------------------------------------------------------------------
// Chain k's stored steps are the k-th run of n_saved steps of the caller's array, as in host memory
inline size_t device_chain_offset(size_t step_bytes, int64_t n_saved, int k) { return step_bytes * (size_t)n_saved * (size_t)k; }

// What the two windows below share: a run of n_saved * interval ensemble steps is enqueued in chunks, a chunk's end is kept
// until its completion has been processed, and the chunks' events rotate over four slots.
struct ChunkWindow
{
    int64_t n_saved, interval, chunk_steps;
    int64_t enq = 0;                     // ensemble steps enqueued
    int64_t chunk_end[4] = {0, 0, 0, 0};
    int64_t next_chunk = 0, oldest = 0;  // chunks enqueued / chunks whose completion has been processed

    ChunkWindow(int64_t n_saved_, int64_t interval_, int64_t chunk_steps_) : n_saved(n_saved_), interval(interval_), chunk_steps(chunk_steps_) {}

    int64_t total() const { return n_saved * interval; }
    bool all_enqueued() const { return enq == total(); }
    bool in_flight() const { return next_chunk > oldest; }
    static int event_slot(int64_t chunk) { return (int)(chunk & 3); }
    void enqueued(int64_t now)
    {
        enq += now;
        chunk_end[event_slot(next_chunk)] = enq;
        ++next_chunk;
    }
};

// Stored step k is written, whole, by the launches of ensemble step (k + 1) * interval - 1: it is complete in the caller's
// array when that step has finished.  The host enqueues chunks of steps, at most two in flight (the chunks' events rotate
// over four slots), and announces what a finished chunk completed.  Nothing is left behind the final synchronisation.
struct DeviceWindow : ChunkWindow
{
    int64_t announced = 0;  // stored steps announced to wait_stored

    DeviceWindow(int64_t n_saved_, int64_t interval_, const ChainPlan& p) : ChunkWindow(n_saved_, interval_, p.chunk_steps) {}

    int64_t next_length() const { return total() - enq < chunk_steps ? total() - enq : chunk_steps; }
    bool must_process_oldest_first() const { return next_chunk - oldest >= 2; }
    // the oldest chunk has finished: the stored steps it completed
    StoredRange process_oldest()
    {
        const StoredRange r = {announced, chunk_end[event_slot(oldest)] / interval};
        announced = r.to;
        ++oldest;
        return r;
    }
};

// ---- the trickle window (Sampler::run_trickle) -------------------------------------------------------------------------
// Stored step k is complete in the pinned ring when ensemble step (k + 2) * interval - 1 has finished (every launch forwards
// 1/interval of the previous stored step), and its ring slot is overwritten from step (k + ring + 1) * interval on.  The
// host enqueues chunks of steps, stays one chunk ahead of the one it waits for, hands out whatever has become complete and
// never lets the launches run into a slot it has not copied yet.  The run's last stored step has no launches behind it:
// it is fetched at the end (tail).
struct TrickleWindow : ChunkWindow
{
    int64_t ring;
    bool direct;
    int64_t copied = 0;  // stored steps handed to the caller

    TrickleWindow(int64_t n_saved_, int64_t interval_, const ChainPlan& p) : ChunkWindow(n_saved_, interval_, p.chunk_steps), ring(p.ring), direct(p.direct) {}

    int64_t ring_slot(int64_t stored_step) const { return stored_step & (ring - 1); }

    int64_t next_length() const
    {
        int64_t now = (total() - enq < chunk_steps) ? total() - enq : chunk_steps;
        // The stored steps that become complete with the LAST chunk are copied out with nothing left to overlap: the
        // run ends with a chunk of one interval, so that this tail is one stored step instead of a chunk's worth
        // (11.80 -> 11.55 ms per 2 000 steps at C2)
        if (!direct && now == total() - enq && now > interval) now -= interval;
        return now;
    }
    // at most two chunks in flight, and no launch may forward into a ring slot that is still to be copied out
    // (forwarding into the final place needs no such care: a device slot is reused ring + 1 stored steps after it
    //  was written, its forwarding is over one stored step after)
    bool must_process_oldest_before(int64_t now) const
    {
        return in_flight() && (next_chunk - oldest >= 2 || (!direct && enq + now > (copied + ring + 1) * interval));
    }
    // the oldest chunk has finished: the stored steps that are fully forwarded now and were not handed out before
    StoredRange process_oldest()
    {
        const int64_t complete = chunk_end[event_slot(oldest)] / interval - 1;
        const StoredRange r = {copied, complete > copied ? complete : copied};
        copied = r.to;
        ++oldest;
        return r;
    }
    // behind the final synchronisation: what the launches did not forward (exactly one stored step, the last)
    StoredRange tail()
    {
        const StoredRange r = {copied, n_saved};
        copied = n_saved;
        return r;
    }
};

// ---- the sub-chunk path ------------------------------------------------------------------------------------------------
// staging -> the caller's memory, stored steps [first, first + count) of chain k: chain k's steps are n_saved steps apart
// in the caller's array, sub_saved steps apart in the staging buffer
inline size_t subchunk_chain_offset(size_t step_bytes, int64_t sub_saved, int k) { return step_bytes * (size_t)sub_saved * (size_t)k; }
struct SubchunkCopy { size_t dst, src, bytes; };
inline SubchunkCopy subchunk_copy(size_t step_bytes, int64_t sub_saved, int64_t n_saved, int64_t first, int64_t count, int k)
{
    return {step_bytes * ((size_t)n_saved * (size_t)k + (size_t)first), subchunk_chain_offset(step_bytes, sub_saved, k), step_bytes * (size_t)count};
}
// bytes of a device chain half in use by a sub-chunk of `now` stored steps (the whole half goes to staging in one copy)
inline size_t subchunk_half_used(size_t step_bytes, int64_t sub_saved, int64_t now, int chains)
{
    return step_bytes * (size_t)sub_saved * (size_t)(chains - 1) + step_bytes * (size_t)now;
}

// ---- the pieces of a differential-evolution run and of a batch run (DeSampler::run_mover, BatchSampler::run_mover) --------
// Both movers step a run a piece at a time and wait for the device behind every piece: its stored steps (and, DE, its
// accepted counters) leave through buffers of the piece's size.  A destination in device memory needs no chain buffer.
struct PiecePlan
{
    int64_t n_saved;
    int64_t piece_saved, n_pieces;    // stored steps per piece (the last may be shorter); pieces (none for a run of nothing)
    size_t chain_bytes, acc_entries;  // what to grow: the device chain of a host destination, the accepted counters

    StoredRange piece(int64_t c) const
    {
        const int64_t first = c * piece_saved;
        return {first, n_saved - first < piece_saved ? n_saved : first + piece_saved};
    }
};
inline PiecePlan pieces_of(int64_t n_saved, int64_t piece_saved)
{
    PiecePlan p = {};
    p.n_saved = n_saved;
    p.piece_saved = piece_saved;
    p.n_pieces = n_saved > 0 ? (n_saved + piece_saved - 1) / piece_saved : 0;
    return p;
}

// DE: a piece is at most 256 MiB of the handle's device chain and 64 MiB of accepted counters, at least one stored step.
// (Bounds of device buffers the handle keeps; split_stage_slots' 256 MiB bounds pinned host memory and is its own number.)
// A device destination has no chain buffer, so only the counters cut it: without them it is one piece.
constexpr size_t kDePieceChainBytes = (size_t)256 << 20, kDePieceCounterBytes = (size_t)64 << 20;
inline PiecePlan plan_de_pieces(size_t step_bytes, int64_t n_saved, int32_t interval, bool chain, bool device_dest, bool want_accepted)
{
    const bool host_chain = chain && !device_dest;
    int64_t piece = n_saved;
    if (want_accepted)
    {
        const int64_t fit = (int64_t)(kDePieceCounterBytes / ((size_t)interval * sizeof(uint32_t)));
        if (piece > fit) piece = fit < 1 ? 1 : fit;
    }
    if (host_chain)
    {
        const int64_t fit = (int64_t)(kDePieceChainBytes / step_bytes);
        if (piece > fit) piece = fit < 1 ? 1 : fit;
    }
    PiecePlan p = pieces_of(n_saved, piece);
    p.chain_bytes = host_chain ? (size_t)piece * step_bytes : 0;
    p.acc_entries = want_accepted ? (size_t)(piece * (int64_t)interval) : 0;
    return p;
}
// where a piece that starts at stored step `first` begins in the caller's device array (DE points its run record there)
inline size_t device_piece_offset(size_t step_bytes, int64_t first) { return step_bytes * (size_t)first; }

// Batch: the sub-chunks of a host chain (stored_steps_per_subchunk of `budget` bytes); one sub-chunk without a chain or into
// device memory.  The accepted counters are kept for the whole run.
inline PiecePlan plan_batch_pieces(size_t budget, size_t step_bytes, int64_t n_saved, int32_t interval, bool chain, bool device_dest, bool want_accepted)
{
    const bool host_chain = chain && !device_dest;
    const int64_t sub_saved = host_chain ? stored_steps_per_subchunk(budget, step_bytes, n_saved) : n_saved;
    PiecePlan p = pieces_of(n_saved, sub_saved);
    p.chain_bytes = host_chain ? step_bytes * (size_t)sub_saved : 0;
    p.acc_entries = want_accepted ? (size_t)(n_saved * (int64_t)interval) : 0;
    return p;
}
// RunInfo::chain_slot_base of a sub-chunk that starts at stored step `first`: the kernels count a run's stored steps from 0,
// the sub-chunk's chain (the handle's buffer, or the caller's whole device array with first = 0) starts at `first`
inline int64_t subchunk_slot_base(int64_t first) { return -first; }

// ---- split runs (Sampler::run_split) -----------------------------------------------------------------------------------
// Slots of the pinned staging of stored steps: 256 MiB worth, at least one, at most the run's.  The same number on every
// rank, whether it stores or not: the chunks of a run end where the staging buffer of the ranks that do store is full.
inline int64_t split_stage_slots(size_t step_bytes, int64_t n_saved)
{
    int64_t slots = (int64_t)(((size_t)256 << 20) / step_bytes);
    if (slots < 1) slots = 1;
    if (slots > n_saved) slots = n_saved;
    return slots;
}
// How far the chunk that starts at step s0 goes.  Exchanging moved rows only: 16 steps while the slot bound is being
// learned, compact_chunk otherwise (the host looks at the overflow flag at the end of a chunk).  Some rank stores: until
// the staging buffer is full.
inline int64_t split_chunk_length(int64_t total, int64_t s0, bool compact, bool learning, long compact_chunk, bool any_rank_stores, int32_t interval,
                                  int64_t stage_slots)
{
    int64_t len = total - s0;
    if (compact)
    {
        const int64_t want = learning ? 16 : compact_chunk;
        if (len > want) len = want;
    }
    if (any_rank_stores)
    {
        const int64_t fits = (s0 / interval + stage_slots) * (int64_t)interval - s0;  // steps until the staging buffer is full
        if (len > fits) len = fits;
    }
    return len;
}
// the slot bound MCMCPP_HIP_COMM_COMPACT_CAP sets, or 0: learned from the run
inline uint32_t split_cap_set(long knob_cap, uint32_t cap_full) { return knob_cap > 0 ? (uint32_t)(knob_cap < (long)cap_full ? knob_cap : (long)cap_full) : 0; }
// the slot bound of a run's first chunk (cap_full: a block that holds every walker of an exchange)
inline uint32_t split_first_cap(bool compact, uint32_t cap_set, uint32_t cap_learned, uint32_t cap_full)
{
    if (!compact) return cap_full;
    if (cap_set) return cap_set;
    return cap_learned > 0 && cap_learned < cap_full ? cap_learned : cap_full;
}
// the next chunk's bound: what the last one needed, plus an eighth and a little
inline uint32_t split_next_cap(uint32_t max_count, uint32_t cap_full)
{
    uint64_t want = (uint64_t)max_count + max_count / 8 + 64;
    want = (want + 63) & ~(uint64_t)63;
    return want < cap_full ? (uint32_t)want : cap_full;
}
// bytes this rank received in the exchanges of `len` steps: blocks of moved rows (one exchange per ensemble step with the
// full-step kernels, two otherwise) ...
inline double split_bytes_compact(int64_t len, bool full_step, int comm_world, size_t block_bytes)
{
    return (double)len * (double)(full_step ? 1 : 2) * (double)(comm_world - 1) * (double)block_bytes;
}
// ... or the other ranks' whole slices of both colours (the full-step scheme carries the log-posteriors along)
inline double split_bytes_whole(int64_t len, bool full_step, int comm_world, int shard_count, int dims, size_t elem_size)
{
    return (double)len * (double)(comm_world - 1) * (double)shard_count * 2.0 * (double)((size_t)dims + (full_step ? 1 : 0)) * elem_size;
}

// The schedule of one split run, as the host loop of Sampler::run_split plays it.  The run proceeds in chunks of steps; the
// host looks at the device only at the end of a chunk.  Exchanging moved rows only (`compact`), a chunk whose blocks
// overflowed is tried again from its first step with blocks of cap_full slots, and the bound of the following chunks is
// what the last one needed (split_next_cap) unless the knob sets it.  Stored steps go to a pinned staging buffer of
// stage_slots slots and leave it behind a chunk that held.  A sample of at most kSplitMaxSamples exchanges is timed.
// Every rank of a run builds the same window but for `stores`, and `stores` moves no chunk boundary.
constexpr int kSplitMaxSamples = 32;

struct SplitRequest
{
    int64_t total;               // ensemble steps of the run (> 0)
    int32_t interval;
    bool any_rank_stores, stores;  // some rank hands stored steps to its caller / this one does
    int64_t stage_slots;         // split_stage_slots
    bool compact;                // the exchanges carry moved rows only (StepPlan::compact_exchange)
    uint32_t cap_full;           // a block that holds every walker of an exchange
    long comm_compact_cap, comm_compact_chunk;  // the knobs
    uint32_t cap_learned;        // the bound the handle's last run ended with, or 0
    // what split_bytes_* need
    bool full_step;
    int comm_world, shard_count, dims;
    size_t elem_size;
    size_t (*block_bytes)(uint32_t cap, int dims, size_t elem_size);  // xblock_bytes (exchange_plan.hpp)
};

struct SplitWindow
{
    SplitRequest r;
    uint32_t cap_set, cap, cap_learned;  // the knob's bound or 0; the bound of the chunk in hand; the bound to keep for the next run
    bool learning;                       // first chunk of a run that knows no bound: short, whole-slice blocks
    int64_t sample_stride;
    int64_t s0 = 0, len = 0;             // the chunk in hand: its first step, its length
    int samples = 0, samples_before = 0; // exchanges sampled so far / in front of the chunk in hand
    int64_t staged = 0, handed = 0;      // stored steps copied to staging / handed to the caller
    double xbytes = 0.0;                 // bytes this rank received in the exchanges of the chunks that held
    int64_t rollbacks = 0;               // chunk tries that overflowed

    explicit SplitWindow(const SplitRequest& q)
        : r(q), cap_set(split_cap_set(q.comm_compact_cap, q.cap_full)), cap_learned(q.cap_learned), learning(q.compact && !cap_set && q.cap_learned == 0),
          sample_stride(q.total > kSplitMaxSamples ? q.total / kSplitMaxSamples : 1)
    {
        cap = split_first_cap(r.compact, cap_set, cap_learned, r.cap_full);
        len = chunk_length();
    }

    bool done() const { return s0 == r.total; }
    int64_t first() const { return s0; }
    int64_t end() const { return s0 + len; }

    // ---- the steps of the chunk in hand
    // the sample slot of step s's (red) exchange, or -1: the exchange is not timed
    int take_sample(int64_t s) { return samples < kSplitMaxSamples && s % sample_stride == 0 ? samples++ : -1; }
    bool stores_step(int64_t s) const { return r.stores && (s + 1) % r.interval == 0; }
    // the staging slot of the step that is stored next
    int64_t take_stage_slot() { return staged++ - handed; }

    // ---- the end of a try of the chunk in hand
    // Some block overflowed: the same steps again with blocks nothing can overflow; what the failed try sampled and staged is
    // forgotten.  Returns the step in front of which the stream and the counters have to be put back.
    int64_t chunk_overflowed()
    {
        ++rollbacks;
        samples = samples_before;
        staged = handed;
        cap = r.cap_full;
        return s0;
    }
    // The chunk held (max_count: the most moved walkers any rank packed in one of its exchanges; whole slices: unused): its
    // bytes count, the next chunk's bound is what this one needed, and the next chunk is in hand.
    void chunk_held(uint32_t max_count)
    {
        if (r.compact)
        {
            xbytes += split_bytes_compact(len, r.full_step, r.comm_world, r.block_bytes(cap, r.dims, r.elem_size));
            if (!cap_set) cap_learned = split_next_cap(max_count, r.cap_full);
            cap = cap_set ? cap_set : cap_learned;
            learning = false;
        }
        else
            xbytes += split_bytes_whole(len, r.full_step, r.comm_world, r.shard_count, r.dims, r.elem_size);
        s0 += len;
        samples_before = samples;
        len = chunk_length();
    }
    // Behind chunk_held: the staged steps the host hands to its caller now (it waits for the stream first), or none.  They
    // leave when the staging buffer is full, at the end of the run, and -- the host has waited for the chunk anyway -- behind
    // every chunk of moved rows.
    StoredRange hand_out()
    {
        const StoredRange out = {handed, staged > handed && (staged - handed == r.stage_slots || done() || r.compact) ? staged : handed};
        handed = out.to;
        return out;
    }

    // ---- the end of the run
    double bytes_per_step() const { return xbytes / (double)r.total; }
    int64_t cap_slots() const { return r.compact ? (int64_t)cap : 0; }

private:
    int64_t chunk_length() const { return split_chunk_length(r.total, s0, r.compact, learning, r.comm_compact_chunk, r.any_rank_stores, r.interval, r.stage_slots); }
};
}  // namespace mcmcpp
