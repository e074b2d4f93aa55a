// replica_plan.hpp -- the replica-exchange rule among the K chains of one handle (parallel tempering), defined once.
//
// K ensembles run on a ladder of targets (chain k's parameter block flattens the target of chain 0); between runs a
// round proposes to exchange the states of neighbouring chains.  This header is the only place that knows
//   which chains a round pairs            round r pairs (k, k + 1) for k = r (mod 2), k + 1 < K; pair slot j = k >> 1
//   which walkers                         walker w of chain k with walker w of chain k + 1, every w in 0..W-1
//   where the draw comes from             one pcg64 engine seeded (seed, 2^64 - 1 - stream): an increment no step stream of
//                                         the handle has (those differ in seed only); draw (r * 8 + j) * W + w, whatever K is
//                                         and whatever was accepted
//   the decision                          replica_accept below, always in double
//   the launch shape and the jump table   of the kernel that applies it (replica_kernels.hpp)
//
// Plain C++ (no HIP header), like canonical.hpp and fast_log.hpp: a CPU test compiles the very lines the kernel runs
// (tests/cpp/replica_plan_cases.cpp).
#pragma once

#include <stdint.h>

#include "canonical.hpp"
#include "fast_log.hpp"
#include "tie_eps.h"

namespace mcmcpp
{

constexpr int kReplicaMaxSlots = 8;                     // pair slots of a round: kMaxChains / 2
constexpr uint64_t kReplicaMaxRound = 1ULL << 40;       // rounds 0 .. 2^40 - 1: the stream position then fits in 64 bits
constexpr int kReplicaBlockThreads = 256;               // a workgroup of the swap kernel
constexpr int kReplicaLaneEntries = 64;                 // lane table: the draws 1 .. 64 behind a base state

// ---- pairs of a round ------------------------------------------------------------------------------------------------
MCMCPP_HD int replica_first_chain(uint64_t round) { return (int)(round & 1u); }
// pairs (k, k + 1) with k = round (mod 2) and k + 1 < K
MCMCPP_HD int replica_pairs(int K, uint64_t round)
{
    const int k0 = replica_first_chain(round);
    return K - k0 >= 2 ? (K - k0) / 2 : 0;
}
MCMCPP_HD int replica_slot_of(int k) { return k >> 1; }
MCMCPP_HD int replica_lower_chain(uint64_t round, int slot) { return replica_first_chain(round) + 2 * slot; }

// ---- the random stream -------------------------------------------------------------------------------------------------
// pcg64 (setseq_xsl_rr_128_64) once more, without the HIP header pcg128.hpp needs: 128-bit values as two words
struct ReplicaU128
{
    uint64_t lo, hi;
};
struct ReplicaJump  // state -> mult * state + plus (mod 2^128)
{
    ReplicaU128 mult, plus;
};
MCMCPP_HD uint64_t replica_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
MCMCPP_HD ReplicaU128 replica_mul(ReplicaU128 a, ReplicaU128 b)
{
    ReplicaU128 r;
    r.lo = a.lo * b.lo;
    r.hi = replica_mulhi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo;
    return r;
}
MCMCPP_HD ReplicaU128 replica_add(ReplicaU128 a, ReplicaU128 b)
{
    ReplicaU128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u);
    return r;
}
MCMCPP_HD ReplicaU128 replica_apply(const ReplicaJump& f, ReplicaU128 s) { return replica_add(replica_mul(f.mult, s), f.plus); }
MCMCPP_HD ReplicaU128 replica_multiplier()
{
    ReplicaU128 m;
    m.hi = 2549297995355413924ULL, m.lo = 4865540595714422341ULL;
    return m;
}
// XSL-RR 128 -> 64 of the post-step state
MCMCPP_HD uint64_t replica_output(ReplicaU128 s)
{
    const uint64_t x = s.hi ^ s.lo;
    const unsigned rot = (unsigned)(s.hi >> 58);
    return (x >> rot) | (x << ((0u - rot) & 63u));
}
// the stream the exchange draws from: the handle's stream counted down from the top
MCMCPP_HD uint64_t replica_stream_of(uint64_t handle_stream) { return 0xFFFFFFFFFFFFFFFFULL - handle_stream; }
// engine(seed, stream): inc = (stream << 1) | 1, state = (seed + inc) * M + inc
inline void replica_seed(uint64_t seed, uint64_t handle_stream, ReplicaU128* state, ReplicaU128* inc)
{
    const uint64_t stream = replica_stream_of(handle_stream);
    inc->hi = stream >> 63, inc->lo = (stream << 1) | 1u;
    ReplicaU128 s;
    s.hi = 0, s.lo = seed;
    *state = replica_add(replica_mul(replica_add(s, *inc), replica_multiplier()), *inc);
}
// coefficients of `delta` engine steps (Brown's arbitrary-stride algorithm)
inline ReplicaJump replica_jump(ReplicaU128 inc, uint64_t delta)
{
    ReplicaU128 cur_mult = replica_multiplier(), cur_plus = inc, one;
    one.hi = 0, one.lo = 1;
    ReplicaJump acc;
    acc.mult = one;
    acc.plus.hi = acc.plus.lo = 0;
    while (delta > 0)
    {
        if (delta & 1u)
        {
            acc.mult = replica_mul(acc.mult, cur_mult);
            acc.plus = replica_add(replica_mul(acc.plus, cur_mult), cur_plus);
        }
        cur_plus = replica_mul(replica_add(cur_mult, one), cur_plus);
        cur_mult = replica_mul(cur_mult, cur_mult);
        delta >>= 1;
    }
    return acc;
}
// stream position (raw outputs consumed before it) of the draw of (round, slot, walker); round < kReplicaMaxRound
MCMCPP_HD uint64_t replica_draw_position(uint64_t round, int slot, int W, int w)
{
    return (round * (uint64_t)kReplicaMaxSlots + (uint64_t)slot) * (uint64_t)W + (uint64_t)w;
}
// the engine state a slot's walkers start from: the state in front of the slot's first draw
inline ReplicaU128 replica_slot_base(ReplicaU128 state0, ReplicaU128 inc, uint64_t round, int slot, int W)
{
    return replica_apply(replica_jump(inc, replica_draw_position(round, slot, W, 0)), state0);
}
// The two-level jump table, built once per handle: entries [0, 64) are the lane stride (entry i: i + 1 engine steps, the
// state whose output is draw i), entries [64, 64 + ceil(W / 64)) the wavefront stride (entry 64 + m: 64 m steps).
MCMCPP_HD int replica_table_entries(int W) { return kReplicaLaneEntries + (W + kReplicaLaneEntries - 1) / kReplicaLaneEntries; }
inline void replica_fill_table(ReplicaU128 inc, int W, ReplicaJump* out)
{
    for (int i = 0; i < kReplicaLaneEntries; ++i) out[i] = replica_jump(inc, (uint64_t)i + 1);
    for (int m = 0; m < replica_table_entries(W) - kReplicaLaneEntries; ++m) out[kReplicaLaneEntries + m] = replica_jump(inc, (uint64_t)kReplicaLaneEntries * (uint64_t)m);
}
// walker w's raw draw from its slot's base state
MCMCPP_HD uint64_t replica_draw(const ReplicaJump* table, ReplicaU128 base, int w)
{
    const ReplicaU128 wave = replica_apply(table[kReplicaLaneEntries + (w >> 6)], base);
    return replica_output(replica_apply(table[w & 63], wave));
}

// ---- the decision ------------------------------------------------------------------------------------------------------
// Chains a = k and b = k + 1 hold x_a and x_b.  lp_aa = logp_a(x_a) and lp_bb = logp_b(x_b) are the stored log-posteriors,
// lp_ab = logp_a(x_b) and lp_ba = logp_b(x_a) the cross evaluations.  The Metropolis ratio of exchanging the two states on
// the product target is exp((lp_ab - lp_aa) + (lp_ba - lp_bb)); ln U is the stretch accept's own -Exp(1) variate.  No
// special cases: -inf, +inf and NaN are decided by the comparison alone (a NaN delta rejects, a +inf delta accepts), and a
// near tie is counted only where the margin is finite.
MCMCPP_HD bool replica_accept(uint64_t draw, double lp_aa, double lp_bb, double lp_ab, double lp_ba, bool* near_tie)
{
    const double u = canonical(draw, double());
    const double lnU = fast_log(1.0 - u);
    const double delta = (lp_ab - lp_aa) + (lp_ba - lp_bb);
    const double margin = __builtin_fabs(lnU - delta);
    const double scale = __builtin_fabs(lnU) + __builtin_fabs(lp_aa) + __builtin_fabs(lp_bb) + __builtin_fabs(lp_ab) + __builtin_fabs(lp_ba);
    *near_tie = margin <= MCMCPP_TIE_EPS_F64 * scale && margin < __builtin_inf();
    return lnU < delta;
}

// ---- launch shape of the swap kernel -----------------------------------------------------------------------------------
// A walker pair is owned by a group of `lanes` lanes (a power of two, 1..64) that move the two rows in `units` pieces of
// `unit_bytes` each: 16-byte pieces where a row is a whole number of them and the buffers are 16-byte aligned (vec_ok),
// elements otherwise.  Short rows share a wavefront (D = 2 doubles: 64 walker pairs per wavefront); the longest rows
// (D = 1024) take a wavefront each and several trips.
struct ReplicaShape
{
    int lanes, units, unit_bytes, walkers_per_block;
    unsigned grid_x, grid_y;
};
MCMCPP_HD ReplicaShape replica_shape(int W, int D, int elem_size, int vec_ok, int pairs)
{
    ReplicaShape s;
    s.unit_bytes = vec_ok ? 16 : elem_size;
    s.units = D * elem_size / s.unit_bytes;
    int lanes = 1;
    while (lanes < s.units && lanes < 64) lanes <<= 1;
    s.lanes = lanes;
    s.walkers_per_block = kReplicaBlockThreads / lanes;
    s.grid_x = (unsigned)((W + s.walkers_per_block - 1) / s.walkers_per_block);
    s.grid_y = (unsigned)pairs;
    return s;
}

}  // namespace mcmcpp
