// evidence_plan.hpp -- the host's decisions of evidence.hip (mcmcpp_hip_evidence_ratios, include/mcmcpp_hip.h): how pairs and
// directions are numbered, with which rungs' parameters the draws of a rung are evaluated, the steps of a chunk, and the launch
// shapes of the two kernels -- as pure functions of plain numbers.  No HIP header: this file compiles with the host compiler
// alone, and tests/test_evidence_plan.py checks it there.  evidence.hip turns a plan into launches and buffer sizes; it holds
// no threshold of its own.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rhat_plan.hpp"

namespace mcmcpp
{
constexpr int kEvidenceThreads = 256;  // threads per block of both kernels
constexpr int kEvidenceTile = 1024;    // draws of a slice the weights kernel stages at a time (kEvidenceThreads * 4)

// Pair p is the rungs (p, p + 1).  Direction 0 (stepping stone) takes the draws of rung p + 1, direction 1 those of rung p.
// Every output is [2][K - 1], d-major.
inline int evidence_pairs(int K) { return K - 1; }
inline int evidence_index(int K, int d, int p) { return d * (K - 1) + p; }
inline int evidence_draws_rung(int d, int p) { return d == 0 ? p + 1 : p; }  // whose draws
inline int evidence_other_rung(int d, int p) { return d == 0 ? p : p + 1; }  // u = logp_other(x) - logp_own(x)

// What is done with the draws of rung k: evals[0] = k itself (its own log-posterior, evaluated once and shared by both pairs
// the rung belongs to), then the lower neighbour (for d = 0 of pair k - 1) and the upper one (for d = 1 of pair k), where
// they exist: at most three calculator launches per chunk.  uses[j]: the (d, p) that evals[1 + j] serves.
struct EvidenceRung
{
    int n_evals = 0, evals[3] = {0, 0, 0};
    int n_uses = 0, use_d[2] = {0, 0}, use_p[2] = {0, 0};
};
inline EvidenceRung evidence_rung(int K, int k)
{
    EvidenceRung r;
    r.evals[r.n_evals++] = k;
    if (k > 0)
    {
        r.evals[r.n_evals++] = k - 1;
        r.use_d[r.n_uses] = 0, r.use_p[r.n_uses] = k - 1, ++r.n_uses;
    }
    if (k + 1 < K)
    {
        r.evals[r.n_evals++] = k + 1;
        r.use_d[r.n_uses] = 1, r.use_p[r.n_uses] = k, ++r.n_uses;
    }
    return r;
}

// Steps of a chunk (MCMCPP_HIP_EVIDENCE_CHUNK_MB): what is uploaded at a time of host steps, and what one calculator launch
// evaluates.  The calculator reads rows that follow each other, so of a device chain of which only every slice-th step is used
// a chunk is one step, read where it lies.
inline long long evidence_steps_per_chunk(size_t chunk_bytes, size_t step_bytes, bool on_device, long long slice)
{
    if (on_device && slice > 1) return 1;
    return rhat_steps_per_chunk(chunk_bytes, step_bytes);
}

// The difference kernel over `count` draws of a chunk: one thread a draw
inline long long evidence_diff_blocks(long long count) { return (count + kEvidenceThreads - 1) / kEvidenceThreads; }
inline bool evidence_grid_fits(long long count) { return evidence_diff_blocks(count) <= kRhatGridXMax; }

// The weights kernel over the N draws of a (d, p): block t takes slice t of sum_fixed (rhat_slice_len(N) draws, the last may
// be short) in tiles of kEvidenceTile; partial sums [slices][2]: of e, of e e.
struct EvidenceWeightsPlan
{
    long long slen = 0;
    int slices = 0, tiles_per_slice = 0;
    unsigned blocks = 0;
};
inline EvidenceWeightsPlan evidence_weights_plan(long long N)
{
    EvidenceWeightsPlan p;
    p.slen = rhat_slice_len(N);
    p.slices = rhat_slices(N);
    p.tiles_per_slice = (int)(((N < p.slen ? N : p.slen) + kEvidenceTile - 1) / kEvidenceTile);
    p.blocks = (unsigned)p.slices;
    return p;
}
// draws [first, first + count) of slice t
RHAT_HD void evidence_slice_span(long long N, long long slen, int t, long long* first, long long* count)
{
    *first = (long long)t * slen;
    *count = N - *first < slen ? N - *first : slen;
}
}  // namespace mcmcpp
