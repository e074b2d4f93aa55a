// quantile_plan.hpp -- how quantiles.hip selects order statistics and counts ranks: the digits a key is taken apart into, which
// counters of a pass live in LDS, how parameters and rank groups are tiled over blocks, how the samples of a chunk are cut into
// slices, and the steps of a chunk -- as pure functions of plain numbers.  No HIP header: this file compiles with the host
// compiler alone, and tests/test_quantile_plan.py checks it there over a grid of shapes.  quantiles.hip turns a plan into
// launches and buffer sizes; it holds no threshold of its own.
//
// A pass of the selection counts, per (parameter, rank group), the samples whose key starts with the group's prefix, by their
// next digit.  One block takes a slice of the samples and a tile of `tile` consecutive parameters, with all `groups` rank
// groups of each: tile x groups sets of 2^bits counters, and one prefix per set.
#pragma once

#include <cstddef>
#include <cstdint>

#include "hist_plan.hpp"

namespace mcmcpp
{
constexpr int kQuantPlanThreads = 256;       // threads per block of both kernels
constexpr int kQuantDigitBits = 8;           // 256 counters to a set: 63 sets in 64 KiB of LDS, 4 passes for fp32, 8 for fp64
constexpr int kQuantMaxRanks = 64;           // ranks of one call: the most rank groups of a parameter
constexpr int kQuantMaxParams = 1024;
constexpr int kQuantMinTile = 4;             // an LDS tile narrower than this (and than P) reads under 16 bytes of a row: global counters then
constexpr int kQuantQueryTile = 8;           // queries a thread of the rank kernel holds in registers at a time
constexpr long long kQuantGridXMax = 2147483647, kQuantGridYMax = 65535, kQuantGridZMax = 65535;

// the digits of a key of key_bits bits, most significant first; every bit belongs to exactly one
struct QuantDigit
{
    int shift, bits;
};
inline int quantile_passes(int key_bits, int digit_bits = kQuantDigitBits) { return (key_bits + digit_bits - 1) / digit_bits; }
inline QuantDigit quantile_digit(int key_bits, int pass, int digit_bits = kQuantDigitBits)
{
    const int top = key_bits - pass * digit_bits;  // bits still to take, this digit included
    const int bits = top < digit_bits ? top : digit_bits;
    return {top - bits, bits};
}

// steps per chunk: bounded by the chunk size and by 32-bit sample indexing (a device chain is read in place: pass the most
// a size_t holds and only the indexing bounds it)
inline long long quantile_steps_per_chunk(size_t chunk_bytes, size_t step_bytes, int W) { return hist_steps_per_chunk(chunk_bytes, step_bytes, W); }

struct QuantPlan
{
    unsigned n = 0;  // samples (rows of P values) of the chunk
    int key_bits = 0, digit_bits = 0, cells = 0, groups = 0;
    int lds = 0;               // counters (and prefixes) of a block in LDS; else global 64-bit atomics
    int tile = 0, ptiles = 0;  // parameters of a block; blocks along grid.y
    unsigned slices = 0, per = 0, blocks = 0;  // blocks along grid.x, each taking `per` samples
    size_t lds_bytes = 0;
    size_t counters = 0;       // 64-bit counters of the pass: P x groups x cells
};

// one pass of the selection over one chunk of n >= 1 samples, with at most `groups` rank groups to a parameter
inline QuantPlan quantile_plan(unsigned n, int P, int groups, int key_bits, int digit_bits, int cus, size_t lds_limit)
{
    QuantPlan p;
    p.n = n;
    p.key_bits = key_bits;
    p.digit_bits = digit_bits;
    p.cells = 1 << digit_bits;
    p.groups = groups;
    p.counters = (size_t)P * groups * p.cells;
    const size_t set_bytes = (size_t)p.cells * 4 + (size_t)key_bits / 8;  // u32 counters and the set's prefix
    const long long fit = (long long)(lds_limit / ((size_t)groups * set_bytes));
    const int widest = P < kQuantPlanThreads ? P : kQuantPlanThreads;
    p.lds = fit >= (P < kQuantMinTile ? P : kQuantMinTile);
    int tile = (p.lds && fit < widest) ? (int)fit : widest;
    p.ptiles = (P + tile - 1) / tile;
    const int even = (P + p.ptiles - 1) / p.ptiles;  // the same number of tiles, evened out
    p.tile = even < kQuantMinTile ? tile : even;
    p.lds_bytes = p.lds ? (size_t)p.tile * groups * set_bytes : 0;
    p.slices = hist_slices_for(n, cus, p.ptiles, p.lds ? (long long)p.tile * groups * p.cells : 1);
    p.per = (n + p.slices - 1) / p.slices;
    p.blocks = (n + p.per - 1) / p.per;
    return p;
}

// the rank-count pass over one chunk: a thread holds kQuantQueryTile queries of its parameter and streams the slice once per
// such tile of queries
struct QuantRankPlan
{
    unsigned n = 0;
    int tile = 0, ptiles = 0, query_tile = kQuantQueryTile;
    unsigned slices = 0, per = 0, blocks = 0;
};

inline QuantRankPlan quantile_rank_plan(unsigned n, int P, int cus)
{
    QuantRankPlan p;
    p.n = n;
    const int widest = P < kQuantPlanThreads ? P : kQuantPlanThreads;
    p.ptiles = (P + widest - 1) / widest;
    p.tile = (P + p.ptiles - 1) / p.ptiles;
    p.slices = hist_slices_for(n, cus, p.ptiles, 1);
    p.per = (n + p.slices - 1) / p.slices;
    p.blocks = (n + p.per - 1) / p.per;
    return p;
}
}  // namespace mcmcpp
