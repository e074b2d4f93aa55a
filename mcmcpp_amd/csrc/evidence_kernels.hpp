// evidence_kernels.hpp -- what evidence.hip (mcmcpp_hip_evidence_ratios) and bridge.hip (mcmcpp_hip_evidence_bridge) share on
// the device: the differences u of a chunk of draws, with what the host needs to know of them.
//   * evidence_diff_kernel: thread = a draw of the chunk: u = (double)logp_other - (double)logp_own, stored at the draw's place
//     of the buffer [N]; the block's largest u that is neither NaN nor +inf (as a key whose unsigned order is the
//     doubles' order, -0 below +0) and its counts of non-finite u and of NaN or +inf among them, first in LDS, then one
//     integer atomic each per block: a maximum and two integer sums, which no order of arrival changes (evidence_note_u, which
//     the differences kernel of gaussian_bridge.hip calls too).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include "evidence_plan.hpp"

namespace mcmcpp
{
// per (d, p) in flight: the running maximum's key (0: none yet), the non-finite u, the NaN or +inf among them
struct EvidenceState
{
    unsigned long long max_key, nonfinite, bad;
};

__host__ __device__ inline unsigned long long evidence_key(double u)
{
    unsigned long long b;
    memcpy(&b, &u, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
inline double evidence_key_value(unsigned long long key)
{
    const unsigned long long b = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFULL) : ~key;
    double u;
    memcpy(&u, &b, 8);
    return u;
}

// What a block of a differences kernel does with its u (every thread of the block calls it; `live`: the thread has a draw):
// the block's maximum and counts first in LDS, then one integer atomic each on *state
__device__ inline void evidence_note_u(double u, bool live, EvidenceState* __restrict__ state)
{
    __shared__ unsigned long long s_max, s_nonfinite, s_bad;
    if (threadIdx.x == 0) s_max = 0, s_nonfinite = 0, s_bad = 0;
    __syncthreads();
    if (live)
    {
        const bool nan = u != u, pinf = u == __builtin_inf(), ninf = u == -__builtin_inf();
        if (nan || pinf || ninf) atomicAdd(&s_nonfinite, 1ULL);
        if (nan || pinf)
            atomicAdd(&s_bad, 1ULL);
        else
            atomicMax(&s_max, evidence_key(u));
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        if (s_max) atomicMax(&state->max_key, s_max);
        if (s_nonfinite) atomicAdd(&state->nonfinite, s_nonfinite);
        if (s_bad) atomicAdd(&state->bad, s_bad);
    }
}

template <class T>
__global__ void __launch_bounds__(kEvidenceThreads)
evidence_diff_kernel(const T* __restrict__ lp_other, const T* __restrict__ lp_own, long long count, double* __restrict__ u_out, EvidenceState* __restrict__ state)
{
    const long long i = (long long)blockIdx.x * kEvidenceThreads + threadIdx.x;
    double u = 0.0;
    if (i < count)
    {
        u = (double)lp_other[i] - (double)lp_own[i];
        u_out[i] = u;
    }
    evidence_note_u(u, i < count, state);
}
}  // namespace mcmcpp
