// ess_plan.hpp -- how ess.hip computes the multi-sequence effective sample size (include/mcmcpp_hip.h,
// mcmcpp_hip_effective_sample_size): the lag blocks, which steps of a (chain, half) a lag block walks with and without bounds
// checks, the rounds the lags are evaluated in under the two knobs, the grid of a round, and the host's part (gamma, rho, the
// window walk, tau and ess from the [lags][P] sums) -- as pure functions of plain numbers.  No HIP header: this file compiles
// with the host compiler alone, and tests/test_ess_plan.py checks it there.  ess.hip holds no threshold of its own.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdlib>

#include "rhat_plan.hpp"

namespace mcmcpp
{
// A lane keeps kEssLagBlock accumulators and kEssLagBlock converted samples, 2 VGPRs each, and kEssRowsInFlight rows' loads
// of both streams: 2 * 32 + 2 * 8 doubles = 160 VGPRs before any address or index (the compiler's figure for gfx950 is 248, no
// scratch: two wavefronts a SIMD).  Twice the block would leave one wavefront; half the block rereads every half twice as
// often.  With that many registers a lane has no room for a second element: one element a lane, of either type.
constexpr int kEssLagBlock = 32;
constexpr int kEssRowsInFlight = 8;
constexpr int kEssVector = 1;
constexpr int kEssWave = 64;
constexpr int kEssBlocksPerGroup = 4;  // the wavefronts of a workgroup take consecutive lag blocks of the same 64 elements: their rereads of a row hit the CU's cache
constexpr int kEssThreads = kEssWave * kEssBlocksPerGroup;
constexpr long long kEssDefaultFirstLags = 64;
constexpr size_t kEssDefaultWorkMb = 1024;

static_assert(kEssLagBlock % kEssRowsInFlight == 0 && kEssLagBlock % 2 == 0, "whole groups of rows, whole pairs of lags");

// ---- the window ----------------------------------------------------------------------------------------------------------
RHAT_HD long long ess_cap(long long L, long long max_lag) { return max_lag == 0 || max_lag > L - 1 ? L - 1 : max_lag; }
RHAT_HD long long ess_kmax(long long cap) { return (cap - 1) / 2; }
RHAT_HD long long ess_function_lags(long long n_functions, long long cap) { return n_functions < cap + 1 ? n_functions : cap + 1; }
// lags 0 .. 2 kmax + 1 for the window, the functions' lags; every one of them is <= cap
RHAT_HD long long ess_lags_needed(long long cap, long long n_functions)
{
    const long long w = 2 * ess_kmax(cap) + 2, f = ess_function_lags(n_functions, cap);
    return w > f ? w : f;
}
RHAT_HD long long ess_blocks(long long lags) { return (lags + kEssLagBlock - 1) / kEssLagBlock; }

// ---- which steps a lane walks for lag block [t0, t0 + B) of a sequence of L steps ---------------------------------------------
// s runs over [0, lead_end) in groups of B from 0; the groups that begin below full_end need no bounds check (every product
// e_s e_{s + t0 + j}, j < B, exists); the others check s + t0 + j < L
struct EssWalk
{
    long long lead_end, full_end;
};
RHAT_HD EssWalk ess_block_walk(long long L, long long t0)
{
    EssWalk w;
    w.lead_end = L > t0 ? L - t0 : 0;
    const long long last = L - t0 - 2LL * kEssLagBlock + 2;  // groups beginning at s0 < last: s0 + B - 1 + t0 + B - 1 <= L - 1
    w.full_end = last > 0 ? (last + kEssLagBlock - 1) / kEssLagBlock * kEssLagBlock : 0;
    return w;
}

// ---- rounds --------------------------------------------------------------------------------------------------------------
struct EssKnobs
{
    long long first_lags;
    size_t work_bytes;
};
inline EssKnobs ess_knobs_from_env()
{
    EssKnobs k{kEssDefaultFirstLags, chunk_bytes_from_env("MCMCPP_HIP_ESS_WORK_MB", kEssDefaultWorkMb)};
    if (const char* env = std::getenv("MCMCPP_HIP_ESS_FIRST_LAGS"))
    {
        const long long v = std::atoll(env);
        if (v >= 1 && v <= (1LL << 40)) k.first_lags = v;
    }
    return k;
}
// blocks of a round are at most this many, so that grid y stays within the launch limit
constexpr long long kEssMaxRoundBlocks = kRhatGridYMax * (long long)kEssBlocksPerGroup;
// lags of A ([lag][series] doubles) that fit the work buffer: whole blocks, one at the least
inline long long ess_round_capacity(size_t work_bytes, long long series)
{
    const long long fit = (long long)(work_bytes / 8 / (size_t)series) / kEssLagBlock * kEssLagBlock, most = kEssMaxRoundBlocks * kEssLagBlock;
    return fit < kEssLagBlock ? kEssLagBlock : (fit > most ? most : fit);
}
// lags of the round that begins at lag `done` (a multiple of B): the first covers first_lags and the functions' lags, each
// later one twice the one before; never more than the capacity, never past the blocks that hold the lags needed
inline long long ess_round_lags(long long done, long long previous, const EssKnobs& knobs, long long series, long long cap, long long n_functions)
{
    const long long total = ess_blocks(ess_lags_needed(cap, n_functions)) * kEssLagBlock, room = ess_round_capacity(knobs.work_bytes, series);
    long long want;
    if (done == 0)
    {
        const long long f = ess_function_lags(n_functions, cap);
        want = ess_blocks(knobs.first_lags > f ? knobs.first_lags : f) * kEssLagBlock;
    }
    else
        want = 2 * previous;
    if (want > room) want = room;
    if (want > total - done) want = total - done;
    return want;
}

// the lag kernel's grid for a round of `blocks` lag blocks over zs (chain, half) pairs of E elements
struct EssGrid
{
    unsigned x, y, z;
};
inline EssGrid ess_lag_grid(long long E, long long blocks, int zs)
{
    return EssGrid{(unsigned)((E + kEssWave - 1) / kEssWave), (unsigned)((blocks + kEssBlocksPerGroup - 1) / kEssBlocksPerGroup), (unsigned)zs};
}

// ---- the host's part -------------------------------------------------------------------------------------------------------
// gamma[t] = (S[t] / M) / L; rho[0] = 1, rho[t] = 1 - (within - gamma[t]) / varplus
inline double ess_gamma(double S, double M, double L) { return (S / M) / L; }
inline double ess_varplus(double within, double between, double L) { return (within * (L - 1.0)) / L + between; }
inline double ess_rho(long long t, double gamma, double within, double varplus) { return t == 0 ? 1.0 : 1.0 - (within - gamma) / varplus; }

// Geyer's initial monotone sequence over the pairs P_k = rho[2k] + rho[2k + 1], k <= kmax, of which lags [0, have) are known.
// state: 1 the window closed (a P_k, k >= 1, for which P_k >= 0 is false), 0 it ran to kmax, -1 it needs lags that are not known
struct EssWindow
{
    int state;
    long long pairs;
    double total;
};
template <class Rho>
inline EssWindow ess_walk_window(Rho&& rho, long long have, long long kmax)
{
    EssWindow w{0, 0, 0.0};
    double q = 0.0;
    for (long long k = 0; k <= kmax; ++k)
    {
        if (2 * k + 1 >= have)
        {
            w.state = -1;
            return w;
        }
        const double p = rho(2 * k) + rho(2 * k + 1);
        if (k >= 1 && !(p >= 0.0))
        {
            w.state = 1;
            return w;
        }
        q = k == 0 ? p : (p < q ? p : q);
        w.total = k == 0 ? q : w.total + q;
        w.pairs = k + 1;
    }
    return w;
}
// tau = -1 + 2 total, not below 1 / log10(N) (a NaN stays); ess = N / tau
inline double ess_tau(double total, double N)
{
    const double tau = -1.0 + 2.0 * total, floor_ = 1.0 / std::log10(N);
    return tau < floor_ ? floor_ : tau;
}
}  // namespace mcmcpp
