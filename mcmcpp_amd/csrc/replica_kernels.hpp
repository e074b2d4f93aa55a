// replica_kernels.hpp -- the device side of a replica-exchange round (replica_plan.hpp): one launch decides and applies
// every swap of the round, between runs (exchange_chains) and inside a tempered run alike.  The cross log-posteriors are
// there already (replica_cross_kernel of stretch_kernel.hpp); replica_round.hpp enqueues the two launches.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "replica_plan.hpp"

namespace mcmcpp
{

// [lower chain of a pair]{accepted, near ties}
struct ReplicaCounts
{
    unsigned long long accepted, near_ties;
};
constexpr int kReplicaCountRecords = 2 * kReplicaMaxSlots - 1;  // a record per pair of neighbours among kMaxChains chains

// The buffers that hold the ensemble when the round is due: the home ones between runs, whichever are in use inside a run
template <class T>
struct ReplicaSwapArgs
{
    T* pos;                    // [K][W][D]: the position buffer in use
    T* logp;                   // chain 0's log-posteriors in use; chain k's lie logp_stride_bytes * k behind them
    const T* cross;            // [slots][2][W]: logp_a(x_b), logp_b(x_a) (replica_cross_kernel)
    const ReplicaJump* table;  // replica_fill_table
    ReplicaCounts* counts;     // [K - 1], by the lower chain of a pair: added to, never cleared here
    unsigned long long logp_stride_bytes;
    unsigned long long nacc_behind_logp_bytes;  // from a chain's `logp` to its n_accept
    uint32_t moved_bit;        // set in n_accept[w] of both chains for a swapped walker w (0: n_accept is not touched)
    int W, D, first_chain, lanes, units, vec_ok;
    ReplicaU128 base[kReplicaMaxSlots];  // the engine state in front of each slot's first draw
};

// one swap launch for a whole round (defined in replica.hip, the kernel's only translation unit)
void launch_replica_swap(const ReplicaSwapArgs<double>& a, const ReplicaShape& s, hipStream_t stream);
void launch_replica_swap(const ReplicaSwapArgs<float>& a, const ReplicaShape& s, hipStream_t stream);

#if defined(MCMCPP_DEFINE_REPLICA_KERNEL)
struct alignas(16) ReplicaPiece
{
    uint32_t v[4];
};

template <class U>
__device__ __forceinline__ void replica_swap_rows(U* a, U* b, int units, int sub, int lanes)
{
    for (int i = sub; i < units; i += lanes)
    {
        const U va = a[i], vb = b[i];
        a[i] = vb;
        b[i] = va;
    }
}

// blockIdx.y: pair slot; a group of a.lanes lanes owns walker w of both chains of the pair (nobody else touches the two rows,
// the two log-posteriors or the two n_accept words: the swap is race-free in place).  Every lane of a group repeats the
// group's decision: no cross-lane traffic in front of the row loads.
// In the middle of a run of the full-step kernels a swapped walker's row in the other position buffer is then out of date:
// the walker gets moved_bit (kRowMovedBit) in both chains' n_accept, and the next launch writes the row whatever it decides.
// Half-step kernels have one buffer, and between runs begin_run marks every row: both pass moved_bit = 0.
template <class T>
__global__ void __launch_bounds__(kReplicaBlockThreads) replica_swap_kernel(const ReplicaSwapArgs<T> a)
{
    const int slot = (int)blockIdx.y;
    const int lanes = a.lanes;
    const int group = (int)threadIdx.x / lanes, sub = (int)threadIdx.x % lanes;
    const long long w_ll = (long long)blockIdx.x * (kReplicaBlockThreads / lanes) + group;
    const bool live = w_ll < (long long)a.W;
    const int ka = a.first_chain + 2 * slot, kb = ka + 1;
    bool accept = false, tie = false;
    if (live)
    {
        const int w = (int)w_ll;
        char* const mine_a = reinterpret_cast<char*>(a.logp) + (size_t)ka * a.logp_stride_bytes;
        char* const mine_b = reinterpret_cast<char*>(a.logp) + (size_t)kb * a.logp_stride_bytes;
        T* const lpa = reinterpret_cast<T*>(mine_a) + w;
        T* const lpb = reinterpret_cast<T*>(mine_b) + w;
        const T lp_ab = a.cross[((size_t)slot * 2 + 0) * (size_t)a.W + w];
        const T lp_ba = a.cross[((size_t)slot * 2 + 1) * (size_t)a.W + w];
        const uint64_t draw = replica_draw(a.table, a.base[slot], w);
        accept = replica_accept(draw, (double)*lpa, (double)*lpb, (double)lp_ab, (double)lp_ba, &tie);
        if (accept)
        {
            T* const xa = a.pos + ((size_t)ka * a.W + w) * (size_t)a.D;
            T* const xb = a.pos + ((size_t)kb * a.W + w) * (size_t)a.D;
            if (a.vec_ok)
                replica_swap_rows(reinterpret_cast<ReplicaPiece*>(xa), reinterpret_cast<ReplicaPiece*>(xb), a.units, sub, lanes);
            else
                replica_swap_rows(xa, xb, a.units, sub, lanes);
            if (sub == 0)
            {
                *lpa = lp_ab;
                *lpb = lp_ba;
                if (a.moved_bit)
                {
                    // (n_accept lies a.nacc_behind_logp_bytes behind the chain's log-posteriors in use: ChainGeometry)
                    uint32_t* const na = reinterpret_cast<uint32_t*>(mine_a + a.nacc_behind_logp_bytes) + w;
                    uint32_t* const nb = reinterpret_cast<uint32_t*>(mine_b + a.nacc_behind_logp_bytes) + w;
                    *na |= a.moved_bit;
                    *nb |= a.moved_bit;
                }
            }
        }
    }
    // counts: one lane per group votes, one lane per wavefront adds (integer sums: the order does not matter)
    const unsigned long long acc_votes = __ballot(live && sub == 0 && accept);
    const unsigned long long tie_votes = __ballot(live && sub == 0 && tie);
    if ((threadIdx.x & 63u) == 0)
    {
        if (acc_votes) atomicAdd(&a.counts[ka].accepted, (unsigned long long)__popcll(acc_votes));
        if (tie_votes) atomicAdd(&a.counts[ka].near_ties, (unsigned long long)__popcll(tie_votes));
    }
}

#endif  // MCMCPP_DEFINE_REPLICA_KERNEL

}  // namespace mcmcpp
