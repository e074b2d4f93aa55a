// hist_plan.hpp -- how histograms.hip launches its kernels for one chunk of selected samples: the width of a bin index, which
// counters live in LDS, how many pairs share a block, how the samples are cut into slices, and how the pair launch is split at the
// grid.y limit -- as pure functions of plain numbers.  No HIP header: this file compiles with the host compiler alone, and
// tests/test_hist_plan.py checks it there over a grid of shapes, including the ones no GPU test of a few seconds reaches.
// histograms.hip turns a plan into launches and buffer sizes; it holds no threshold of its own.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mcmcpp
{
constexpr int kHistPlanThreads = 256;         // threads per block of every histogram kernel
constexpr int kHistMaxTile = 64;              // most pair histograms one block privatises
constexpr long long kHistGridYMax = 65535;    // blocks along grid.y of one launch
constexpr size_t kHistLdsMost = 65536;        // dynamic LDS asked for at the most

inline int hist_index_bytes(int bins) { return bins <= 256 ? 1 : (bins <= 65536 ? 2 : 4); }
inline long long hist_npairs(int P, bool with_pairs) { return with_pairs ? (long long)P * (P - 1) / 2 : 0; }
inline size_t hist_lds_limit(size_t shared_mem_per_block) { return shared_mem_per_block < kHistLdsMost ? shared_mem_per_block : kHistLdsMost; }

// steps per chunk: bounded by the chunk size (through the index buffer) and by 32-bit sample indexing
inline long long hist_steps_per_chunk(size_t chunk_bytes, size_t step_bytes, int W)
{
    long long k = (long long)(chunk_bytes / step_bytes);
    const long long cap = ((long long)1 << 31) / W - 1;
    if (k > cap) k = cap;
    return k < 1 ? 1 : k;
}

// one launch of the pair kernel: tiles [t0, t0 + now) along grid.y, the first of them starting at pair q0
struct HistPairLaunch
{
    long long t0, now, q0;
};

struct HistPlan
{
    unsigned n = 0;  // samples of the chunk; nothing is launched for 0
    int idx_bytes = 1;
    size_t col = 0;  // elements between two columns of the index array
    // bounds pass: blocks of `per` samples
    unsigned bounds_blocks = 0, bounds_per = 0;
    // bin pass
    unsigned bin_blocks = 0;
    // 1-D histograms: grid (single_blocks, P)
    int single_lds = 0;
    unsigned single_slices = 0, single_per = 0, single_blocks = 0;
    size_t single_lds_bytes = 0;
    // 2-D histograms: grid (pair_blocks, tiles) in launches of at most kHistGridYMax tiles
    long long npairs = 0;  // 0: no pair launch
    int pair_lds = 0, tile = 0, last_count = 0;
    long long tiles = 0;
    unsigned pair_slices = 0, pair_per = 0, pair_blocks = 0;
    size_t pair_lds_bytes = 0;
    long long pair_launches = 0;
    HistPairLaunch pair_launch(long long i) const
    {
        const long long t0 = i * kHistGridYMax;
        return {t0, (tiles - t0 < kHistGridYMax) ? tiles - t0 : kHistGridYMax, t0 * tile};
    }
};

// slices of samples: enough blocks to fill the device, each slice long enough to amortise its flush
inline unsigned hist_slices_for(unsigned n, int cus, long long columns, long long flush_cells)
{
    long long want = ((long long)cus * 4 + columns - 1) / columns;
    const long long most = (long long)n / (flush_cells * 4 > 1024 ? flush_cells * 4 : 1024);
    if (want > most) want = most;
    if (want < 1) want = 1;
    return (unsigned)want;
}

inline HistPlan hist_plan(unsigned n, int P, int bins, bool with_pairs, int cus, size_t lds_limit)
{
    HistPlan p;
    p.n = n;
    p.idx_bytes = hist_index_bytes(bins);
    if (n == 0) return p;
    p.col = ((size_t)n + 15) & ~(size_t)15;
    {
        unsigned blocks = (unsigned)cus * 2;
        if (blocks > (n + 255) / 256) blocks = (n + 255) / 256;
        p.bounds_per = (n + blocks - 1) / blocks;
        p.bounds_blocks = (n + p.bounds_per - 1) / p.bounds_per;
    }
    p.bin_blocks = (n + kHistPlanThreads - 1) / kHistPlanThreads;
    if (p.bin_blocks > (unsigned)cus * 8) p.bin_blocks = (unsigned)cus * 8;
    p.single_lds = (size_t)bins * 4 <= lds_limit;
    p.single_slices = hist_slices_for(n, cus, P, p.single_lds ? bins : 1);
    p.single_per = (n + p.single_slices - 1) / p.single_slices;
    p.single_blocks = (n + p.single_per - 1) / p.single_per;
    p.single_lds_bytes = p.single_lds ? (size_t)bins * 4 : 0;
    p.npairs = hist_npairs(P, with_pairs);
    if (p.npairs > 0)
    {
        const size_t b2 = (size_t)bins * bins;
        p.pair_lds = b2 * 4 <= lds_limit;
        int tile = p.pair_lds ? (int)(lds_limit / (b2 * 4)) : 1;
        if (tile > kHistMaxTile) tile = kHistMaxTile;
        // keep enough tiles to fill the device
        while (tile > 1 && (p.npairs + tile - 1) / tile < (long long)cus * 2) tile /= 2;
        p.tile = tile;
        p.tiles = (p.npairs + tile - 1) / tile;
        p.last_count = (int)(p.npairs - (p.tiles - 1) * tile);
        p.pair_slices = hist_slices_for(n, cus, p.tiles, p.pair_lds ? (long long)(tile * b2) : 1);
        p.pair_per = (n + p.pair_slices - 1) / p.pair_slices;
        p.pair_blocks = (n + p.pair_per - 1) / p.pair_per;
        p.pair_lds_bytes = p.pair_lds ? (size_t)tile * b2 * 4 : 0;
        p.pair_launches = (p.tiles + kHistGridYMax - 1) / kHistGridYMax;
    }
    return p;
}
}  // namespace mcmcpp
