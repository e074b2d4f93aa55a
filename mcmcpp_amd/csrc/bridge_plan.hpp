// bridge_plan.hpp -- the host's decisions of bridge.hip (mcmcpp_hip_evidence_bridge, include/mcmcpp_hip.h): the shape of
// sum_tree, the buffers of raw u in flight, the launch shapes of the pass kernel and of the kernel that closes its slices, and the
// solver that turns passes into the root -- as pure functions of plain numbers and of a callable that evaluates one pass.  No
// HIP header: this file compiles with the host compiler alone, and tests/test_bridge_plan.py checks it there, with a host
// sum_tree and a host pass in place of the kernels.  bridge.hip turns a plan into launches and buffer sizes; it holds no
// threshold of its own.
//
// sum_tree(v, N), the header's words:
//   tiles of kBridgeTile = 1024 consecutive terms; the missing terms of the last tile are +0.  In a tile, lane t of 256 forms
//   ((v[2t] + v[2t+1]) + v[2t+512]) + v[2t+513] (two loads of 16 bytes); then for s = 128, 64, ..., 1: p_t = p_t + p_{t+s} for t < s;
//   the tile's sum is p_0.  Tile sums are added in ascending order from +0 within a slice of kBridgeSliceTiles = 64 tiles (the
//   last slice may be short); slice sums are added in ascending order from +0.
// The longest chain of dependent additions: 3 + 8 in a tile, 64 in a slice, ceil(N / 65536) over the slices.
#pragma once

#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "evidence_exp.hpp"
#include "evidence_plan.hpp"
#include "normal_score.hpp"

namespace mcmcpp
{
constexpr int kBridgeThreads = 256;     // threads per block of the pass kernel: a block is a tile
constexpr int kBridgeTile = 1024;       // terms of a tile (kBridgeThreads * 4)
constexpr int kBridgeSliceTiles = 64;   // tiles of a slice
constexpr int kBridgeBracketPasses = 1100, kBridgeNewtonPasses = 200;  // the solver's bounds
constexpr double kBridgeTolerance = 9.094947017729282e-13;            // 2^-40

// sigma(x) = 1 / (1 + exp(-x)), through evidence_exp with an argument that is never positive: one value in bits on host and device
MCMCPP_EE_HD double bridge_sigma(double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (x >= 0.0) return 1.0 / (1.0 + evidence_exp(-x));
    const double e = evidence_exp(x);
    return e / (1.0 + e);
}

// The shape of sum_tree over N terms, and the pass kernel's launch: grid (tiles, 2), a block a tile of one direction; the
// closing kernel is one block.  Tile sums [2][3][tiles], slice sums [2][3][slices] (S, Q and, on the final pass, the sum of h h).
struct BridgePlan
{
    long long tiles = 0;
    int slices = 0;
    unsigned grid_x = 0, grid_y = 2;
    size_t tile_sum_doubles = 0, slice_sum_doubles = 0;
};
inline BridgePlan bridge_plan(long long N)
{
    BridgePlan p;
    p.tiles = (N + kBridgeTile - 1) / kBridgeTile;
    p.slices = (int)((p.tiles + kBridgeSliceTiles - 1) / kBridgeSliceTiles);
    p.grid_x = (unsigned)p.tiles;
    p.tile_sum_doubles = 6 * (size_t)p.tiles;
    p.slice_sum_doubles = 6 * (size_t)p.slices;
    return p;
}
inline bool bridge_grid_fits(long long N) { return (N + kBridgeTile - 1) / kBridgeTile <= kRhatGridXMax; }
// tiles [first, first + count) of slice t
MCMCPP_EE_HD void bridge_slice_span(long long tiles, int t, long long* first, long long* count)
{
    *first = (long long)t * kBridgeSliceTiles;
    *count = tiles - *first < kBridgeSliceTiles ? tiles - *first : kBridgeSliceTiles;
}

// The raw u in flight, 8 N bytes each.  Rung k's draws give u(0, k - 1) and u(1, k); pair p is complete behind rung p + 1 and
// then still holds u(1, p) of the rung before: one buffer for direction 0, two that take turns for direction 1 -- of which a
// ladder of two rungs needs one.
inline int bridge_buffers(int K) { return K > 2 ? 3 : 2; }
inline int bridge_buffer_of(int d, int p) { return d == 0 ? 0 : 1 + (p & 1); }

// sum_tree on the host, in the kernel's order
inline double bridge_sum_tree(const double* v, long long N)
{
    const BridgePlan plan = bridge_plan(N);
    double total = 0.0;
    for (int sl = 0; sl < plan.slices; ++sl)
    {
        long long first, count;
        bridge_slice_span(plan.tiles, sl, &first, &count);
        double slice = 0.0;
        for (long long tile = first; tile < first + count; ++tile)
        {
            double p[kBridgeThreads];
            const long long base = tile * kBridgeTile;
            const auto at = [&](long long i) { return base + i < N ? v[base + i] : 0.0; };
            for (int t = 0; t < kBridgeThreads; ++t) p[t] = ((at(2 * t) + at(2 * t + 1)) + at(2 * t + 512)) + at(2 * t + 513);
            for (int s = kBridgeThreads / 2; s >= 1; s >>= 1)
                for (int t = 0; t < s; ++t) p[t] = p[t] + p[t + s];
            slice = slice + p[0];
        }
        total = total + slice;
    }
    return total;
}

// One pass at c: S_d = sum_tree(h_d), Q_d = sum_tree(h_d (1 - h_d)), and on the final pass H_d = sum_tree(h_d h_d)
struct BridgeSums
{
    double S[2] = {0.0, 0.0}, Q[2] = {0.0, 0.0}, H[2] = {0.0, 0.0};
};
struct BridgeRoot
{
    double c = 0.0;
    long long passes = 0;
    int converged = 0;
    BridgeSums at;  // the final pass's sums, at c
};

// The solver of the header.  eval(c, final, &sums) is one pass and returns 0, or a code that ends the solve.
template <class Eval>
int bridge_solve(Eval&& eval, BridgeRoot* out)
{
    BridgeRoot r;
    BridgeSums s;
    double c = 0.0, g = 0.0;
    const auto pass = [&](double at) -> int {
        if (int rc = eval(at, false, &s)) return rc;
        ++r.passes;
        g = s.S[0] - s.S[1];
        return 0;
    };
    const auto finish = [&](double at, int converged) -> int {
        if (int rc = eval(at, true, &r.at)) return rc;
        ++r.passes;
        r.c = at;
        r.converged = converged;
        *out = r;
        return 0;
    };
    if (int rc = pass(c)) return rc;
    if (g == 0.0) return finish(c, 1);
    const bool up = g > 0.0;  // the root lies above
    double lo = 0.0, hi = 0.0, step = 1.0;
    for (;;)
    {
        const double prev = c;
        c = up ? prev + step : prev - step;
        if (c > DBL_MAX) c = DBL_MAX;
        if (c < -DBL_MAX) c = -DBL_MAX;
        step = step + step;
        if (int rc = pass(c)) return rc;
        if (g == 0.0) return finish(c, 1);
        if ((g > 0.0) != up)
        {
            lo = up ? prev : c, hi = up ? c : prev;
            break;
        }
        if (r.passes >= kBridgeBracketPasses) return finish(c, 0);
    }
    for (int it = 0; it < kBridgeNewtonPasses; ++it)
    {
        const double mid = 0.5 * lo + 0.5 * hi;
        double next = mid;
        if (s.S[0] > 0.0 && s.S[1] > 0.0)  // a Newton step on ln S_0 - ln S_1, which is linear in c where the rungs barely overlap
        {
            const double f = normal_score_log(s.S[0]) - normal_score_log(s.S[1]), fp = -(s.Q[0] / s.S[0] + s.Q[1] / s.S[1]);
            if (fp != 0.0) next = c - f / fp;
        }
        if (!(lo < next && next < hi)) next = mid;
        if (next == lo || next == hi) return finish(c, 1);
        const double moved = next > c ? next - c : c - next, size = next < 0.0 ? -next : next;
        if (moved <= kBridgeTolerance * (size > 1.0 ? size : 1.0)) return finish(next, 1);
        c = next;
        if (int rc = pass(c)) return rc;
        if (g == 0.0) return finish(c, 1);
        if (g > 0.0)
            lo = c;
        else
            hi = c;
    }
    return finish(c, 0);
}
}  // namespace mcmcpp
