// rank_plan.hpp -- how rank.hip ranks the draws of a parameter: the digits of the radix sort, the items a block takes, the
// blocks of a pass, the workspace of a tile of parameters and the tile that fits MCMCPP_HIP_RANK_WORK_MB, and the steps of an
// upload chunk of host chains -- as pure functions of plain numbers.  No HIP header: this file compiles with the host compiler
// alone, and tests/test_rank_plan.py checks it there over a grid of shapes.  rank.hip turns a plan into launches and buffer
// sizes; it holds no threshold of its own.  No result depends on anything in here: the sort is stable and the ranks are exact.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "rhat_plan.hpp"

namespace mcmcpp
{
constexpr int kRankDigitBits = 8;                                          // an LSD pass sorts by one digit of 8 bits
constexpr int kRankDigits = 1 << kRankDigitBits;                           // 256 digit values: one thread each in the scans
constexpr int kRankThreads = 256;                                          // threads per block of every kernel of the family
constexpr int kRankWave = 64;
constexpr int kRankWaves = kRankThreads / kRankWave;
constexpr int kRankItemsPerThread = 8;                                     // rounds of a block: round i takes items [256 i, 256 i + 256) of its span
constexpr long long kRankMaxDraws = 2147483647LL;                          // S <= 2^31 - 1: a draw index and a rank fit 32 bits
constexpr size_t kRankDefaultWorkMb = 1024;                                // MCMCPP_HIP_RANK_WORK_MB where the environment names none
constexpr size_t kRankAlign = 256;                                         // every array of the workspace starts on such a boundary
constexpr long long kRankGridXMax = 2147483647LL, kRankGridYMax = 65535;

inline int rank_passes(int key_bits) { return key_bits / kRankDigitBits; }                  // 4 or 8: an even number, the result is where the keys began
inline int rank_digit_shift(int pass) { return pass * kRankDigitBits; }                     // pass 0 sorts by the lowest digit
RHAT_HD long long rank_items_per_block() { return (long long)kRankThreads * kRankItemsPerThread; }
RHAT_HD long long rank_blocks(long long S) { return (S + rank_items_per_block() - 1) / rank_items_per_block(); }
// block b of a pass takes draws [first, first + count) of the S in their current order (the histogram and the scatter kernel
// walk this span, round i its draws [256 i, 256 i + 256))
RHAT_HD void rank_block_span(long long S, long long b, long long* first, long long* count)
{
    const long long B = rank_items_per_block();
    *first = b * B;
    *count = S - b * B < B ? (S - b * B < 0 ? 0 : S - b * B) : B;
}

// 32-bit keys where float draws are ranked as they are; 64 bits for double draws and for every folded value (a double)
inline int rank_key_bits(bool f32, bool fold) { return f32 && !fold ? 32 : 64; }

inline size_t rank_align(size_t bytes) { return (bytes + kRankAlign - 1) / kRankAlign * kRankAlign; }

// The workspace of a tile of parameters (byte offsets): keys and draw indices twice (a pass reads one and writes the other),
// the block x digit table of a pass as [parameter][digit][block], and the digit totals [parameter][digit]
struct RankLayout
{
    size_t keys_a = 0, keys_b = 0, idx_a = 0, idx_b = 0, table = 0, totals = 0, bytes = 0;
};
inline RankLayout rank_layout(long long S, int key_bits, int tile)
{
    RankLayout l;
    const size_t keys = rank_align((size_t)S * (size_t)(key_bits / 8) * (size_t)tile), idx = rank_align((size_t)S * 4 * (size_t)tile);
    l.keys_a = 0;
    l.keys_b = l.keys_a + keys;
    l.idx_a = l.keys_b + keys;
    l.idx_b = l.idx_a + idx;
    l.table = l.idx_b + idx;
    l.totals = l.table + rank_align((size_t)rank_blocks(S) * kRankDigits * 4 * (size_t)tile);
    l.bytes = l.totals + rank_align((size_t)kRankDigits * 4 * (size_t)tile);
    return l;
}

// parameters ranked together: as many as fit work_bytes, one at the least (whose workspace is what it is), P at the most
inline int rank_param_tile(long long S, int P, int key_bits, size_t work_bytes)
{
    // the workspace grows with the tile, by less than in proportion where an array is shorter than its alignment: start from
    // the proportion and walk to the largest tile that fits
    const int most = P < kRankGridYMax ? P : (int)kRankGridYMax;
    const size_t one = rank_layout(S, key_bits, 1).bytes;
    long long guess = (long long)(work_bytes / one);
    if (guess > most) guess = most;
    if (guess < 1) guess = 1;
    int tile = (int)guess;
    while (tile > 1 && rank_layout(S, key_bits, tile).bytes > work_bytes) --tile;
    while (tile < most && rank_layout(S, key_bits, tile + 1).bytes <= work_bytes) ++tile;
    return tile;
}
inline int rank_tiles(int P, int tile) { return (P + tile - 1) / tile; }

inline size_t rank_work_bytes_from_env() { return chunk_bytes_from_env("MCMCPP_HIP_RANK_WORK_MB", kRankDefaultWorkMb); }

// host chains: the steps of one copy group (MCMCPP_HIP_RHAT_CHUNK_MB, as for R-hat)
inline long long rank_steps_per_chunk(size_t chunk_bytes, size_t step_bytes) { return rhat_steps_per_chunk(chunk_bytes, step_bytes); }

// grid of the per-draw kernels (gather, score): x over the draws, 256 a block; y over the tile
inline long long rank_draw_blocks(long long S) { return (S + kRankThreads - 1) / kRankThreads; }
// grid of the kernels that take one thread per (draw, parameter) of all P (NaN check, indicators): in 64 bits; the call is
// refused where it exceeds kRankGridXMax (S P > 2^39: more than any device holds as scores, but not for the grid to assume)
inline long long rank_element_blocks(long long S, int P) { return (S * (long long)P + kRankThreads - 1) / kRankThreads; }
inline bool rank_grids_fit(long long S, int P) { return rank_element_blocks(S, P) <= kRankGridXMax && rank_draw_blocks(S) <= kRankGridXMax; }

// The ranks whose order statistics give the quantile q of S draws: h = q (S - 1) in double, lo = floor(h), hi = ceil(h)
struct RankQuantile
{
    double h;
    long long lo, hi;
};
inline RankQuantile rank_quantile(double q, long long S)
{
    RankQuantile r;
    r.h = q * (double)(S - 1);
    r.lo = (long long)r.h;  // (h >= 0: truncation is the floor)
    r.hi = (double)r.lo < r.h ? r.lo + 1 : r.lo;
    return r;
}
inline double rank_quantile_value(double x_lo, double x_hi, const RankQuantile& r) { return x_lo == x_hi ? x_lo : x_lo + (x_hi - x_lo) * (r.h - (double)r.lo); }
}  // namespace mcmcpp
