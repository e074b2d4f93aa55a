// replica_round.hpp -- what a replica-exchange round among the chains of a handle needs on the host, and the one place that
// enqueues it: the cross evaluations of all pairs in one launch (replica_cross_kernel), the swaps in another
// (replica_swap_kernel).  Sampler::exchange_chains puts a round between runs, Sampler::enqueue_steps into the launch sequence
// of a tempered run (mcmcpp_hip.hip).  No decisions here: which chains pair up is replica_plan.hpp's, where the rounds of a
// run fall temper_plan.hpp's.
#pragma once

#include <cstring>
#include <vector>

#include "launch_table.hpp"
#include "replica_kernels.hpp"
#include "sampler_base.hpp"

namespace mcmcpp
{
// The ensemble as a round finds it.  The sampler fills it in; it owns every buffer named here.
template <class T>
struct ReplicaEnsemble
{
    T* pos;                         // [K][W][D]: the position buffer that holds the ensemble
    T* logp;                        // chain 0's log-posteriors in the half that goes with it
    size_t logp_stride_bytes;       // between two chains' log-posteriors
    size_t nacc_behind_logp_bytes;  // from a chain's `logp` to its n_accept
    uint32_t moved_bit;             // for a swapped walker's n_accept (kRowMovedBit inside a run of the full-step kernels, else 0)
    const T* params;                // chain 0's calculator parameters; chain k's lie params_chain_stride * k elements behind
    int params_chain_stride;
    int K, W, D, vec_ok;
    unsigned cross_grid;            // workgroups per cross evaluation: the grid of the calculator's `calc` launch
};

template <class T>
struct ReplicaRound
{
    typedef typename LaunchTable<T>::CrossFn CrossFn;
    static_assert(kReplicaMaxSlots * 2 == kMaxChains && kReplicaCountRecords == kMaxChains - 1, "a round has a slot for every second chain");

    mcmcpp_hip_sampler* owner = nullptr;  // carries the error message of a failed call
    CrossFn cross_fn = nullptr;
    DeviceBuffer<T> cross;                // [kReplicaMaxSlots][2][W] cross log-posteriors
    DeviceBuffer<ReplicaJump> table;      // the jump table of the exchange stream
    DeviceBuffer<ReplicaCounts> counts;   // [kReplicaCountRecords], by lower chain: a round between runs and a tempered run never overlap
    ReplicaU128 state0 = {}, inc = {};

    // once per handle, by the first round or tempered run (`what`: the caller a refusal names)
    int ensure(mcmcpp_hip_sampler* owner_, const char* what, CrossFn fn, uint64_t seed, uint64_t stream_id, int W, int D)
    {
        owner = owner_;
        if (!fn) return fail(MCMCPP_HIP_E_UNSUPPORTED, "%s: no cross-evaluation kernel for D=%d with this calculator", what, D);
        if (table) return MCMCPP_HIP_OK;
        replica_seed(seed, stream_id, &state0, &inc);
        std::vector<ReplicaJump> t((size_t)replica_table_entries(W));
        replica_fill_table(inc, W, t.data());
        const size_t cross_bytes = sizeof(T) * (size_t)kReplicaMaxSlots * 2 * (size_t)W;
        DeviceBuffer<ReplicaJump> new_table;
        if (new_table.alloc(sizeof(ReplicaJump) * t.size()) != hipSuccess || counts.alloc(sizeof(ReplicaCounts) * kReplicaCountRecords) != hipSuccess ||
            cross.alloc(cross_bytes) != hipSuccess)
            return fail(MCMCPP_HIP_E_NOMEM, "%s: cannot allocate the scratch of a round (%zu bytes)", what, cross_bytes);
        HIP_TRY(hipMemcpy(new_table, t.data(), sizeof(ReplicaJump) * t.size(), hipMemcpyHostToDevice));
        table = std::move(new_table);
        cross_fn = fn;
        return MCMCPP_HIP_OK;
    }

    int clear_counts(hipStream_t stream)
    {
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(ReplicaCounts) * kReplicaCountRecords, stream));
        return MCMCPP_HIP_OK;
    }

    // waits for the stream
    int read_counts(ReplicaCounts (&out)[kReplicaCountRecords], hipStream_t stream)
    {
        HIP_TRY(hipMemcpyAsync(out, counts, sizeof out, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return MCMCPP_HIP_OK;
    }

    // round `round` behind whatever the stream holds: two launches, the counts added to `counts` (a round without pairs: nothing)
    int enqueue(const ReplicaEnsemble<T>& e, uint64_t round, hipStream_t stream)
    {
        const int pairs = replica_pairs(e.K, round), k0 = replica_first_chain(round);
        if (pairs == 0) return MCMCPP_HIP_OK;
        const ReplicaShape shape = replica_shape(e.W, e.D, (int)sizeof(T), e.vec_ok, pairs);
        ReplicaSwapArgs<T> a;
        std::memset(&a, 0, sizeof a);
        a.pos = e.pos, a.logp = e.logp, a.cross = cross, a.table = table, a.counts = counts;
        a.logp_stride_bytes = e.logp_stride_bytes, a.nacc_behind_logp_bytes = e.nacc_behind_logp_bytes, a.moved_bit = e.moved_bit;
        a.W = e.W, a.D = e.D, a.first_chain = k0, a.lanes = shape.lanes, a.units = shape.units, a.vec_ok = e.vec_ok;
        for (int j = 0; j < pairs; ++j) a.base[j] = replica_slot_base(state0, inc, round, j, e.W);
        cross_fn(e.pos, cross, e.params, e.params_chain_stride, e.W, e.D, e.vec_ok, k0, pairs, e.cross_grid, stream);
        launch_replica_swap(a, shape, stream);
        HIP_TRY(hipGetLastError());
        return MCMCPP_HIP_OK;
    }

private:
    template <class... A>
    int fail(int code, const char* fmt, A... a)
    {
        return owner->fail(code, fmt, a...);
    }
};
}  // namespace mcmcpp
