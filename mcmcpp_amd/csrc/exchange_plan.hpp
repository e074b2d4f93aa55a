// exchange_plan.hpp -- the numbers behind the exchange of moved rows (exchange_kernels.hpp): where the pieces of a block lie,
// in how many pieces a row is copied and by how many lanes, and the grids of the three kernels -- as pure functions of plain
// numbers.  No HIP header: this file compiles with the host compiler alone, and tests/test_exchange_kernels.py checks it there
// for every D up to 1024 in both element sizes.  The kernels, SamplerHost::exchange_compact (mcmcpp_hip.hip) and the test shim
// (tests/cpp/exchange_device.hip) all call these functions; none of them holds a copy of the arithmetic.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "canonical.hpp"  // MCMCPP_HD

namespace mcmcpp
{
// ---- a block: [header 16 B][idx: cap x u32][logp: cap x T][rows: cap x D x T], every piece 16-byte aligned ----------------------
constexpr size_t kXBlockHeaderBytes = 16;  // sizeof(XBlockHeader)

MCMCPP_HD size_t xblock_align16(size_t b) { return (b + 15) & ~(size_t)15; }
MCMCPP_HD size_t xblock_idx_offset() { return kXBlockHeaderBytes; }
MCMCPP_HD size_t xblock_logp_offset(uint32_t cap) { return xblock_idx_offset() + xblock_align16((size_t)cap * sizeof(uint32_t)); }
MCMCPP_HD size_t xblock_rows_offset(uint32_t cap, size_t elem_bytes) { return xblock_logp_offset(cap) + xblock_align16((size_t)cap * elem_bytes); }
MCMCPP_HD size_t xblock_bytes(uint32_t cap, int dims, size_t elem_bytes)
{
    return xblock_rows_offset(cap, elem_bytes) + xblock_align16((size_t)cap * (size_t)dims * elem_bytes);
}

// ---- a row: copied in pieces of 16 bytes where its length allows (rows then start 16-byte aligned everywhere), else element by
// element; by `lanes per row` lanes, each taking pieces sub, sub + lpr, ...
struct XRowPieces
{
    bool vec;    // pieces of 16 bytes
    int pieces;  // per row
};
MCMCPP_HD XRowPieces exchange_row_pieces(int dims, size_t elem_bytes)
{
    const bool vec = ((size_t)dims * elem_bytes) % 16 == 0;
    return {vec, vec ? (int)((size_t)dims * elem_bytes / 16) : dims};
}
constexpr int kExchangeMaxLanesPerRow = 64;  // a wavefront
MCMCPP_HD int exchange_lanes_per_row(int pieces)
{
    int lpr = 1;  // a power of two, at most 64
    while (lpr < pieces && lpr < kExchangeMaxLanesPerRow) lpr <<= 1;
    return lpr;
}

// ---- exchange_sync_seen_kernel: one thread per walker of the slice, both colours ------------------------------------------------
constexpr int kSyncSeenThreads = 256;
MCMCPP_HD unsigned exchange_sync_seen_blocks(int shard_count) { return (unsigned)((2 * shard_count + kSyncSeenThreads - 1) / kSyncSeenThreads); }

// ---- exchange_pack_kernel: kPackWalkersPerWave walkers to a wavefront, kPackWavesPerBlock wavefronts to a workgroup -------------
constexpr int kPackWalkersPerWave = 16;
constexpr int kPackWavesPerBlock = 16;
constexpr int kPackThreads = 64 * kPackWavesPerBlock;
// walkers: colors * shard_count
MCMCPP_HD unsigned exchange_pack_blocks(int walkers)
{
    const int pack_waves = (walkers + kPackWalkersPerWave - 1) / kPackWalkersPerWave;
    return (unsigned)((pack_waves + kPackWavesPerBlock - 1) / kPackWavesPerBlock);
}

// ---- exchange_scatter_kernel: grid.x over the slots of a block, 256 / lanes-per-row of them to a workgroup; grid.y over the
// peers (every rank but this one) ---------------------------------------------------------------------------------------------
constexpr int kScatterThreads = 256;
MCMCPP_HD int exchange_scatter_rows_per_block(int lpr) { return kScatterThreads / lpr; }
struct XScatterGrid
{
    unsigned x, y;
};
MCMCPP_HD XScatterGrid exchange_scatter_grid(uint32_t cap, int dims, size_t elem_bytes, int ranks)
{
    const unsigned rows_per_block = (unsigned)exchange_scatter_rows_per_block(exchange_lanes_per_row(exchange_row_pieces(dims, elem_bytes).pieces));
    return {(cap + rows_per_block - 1) / rows_per_block, (unsigned)(ranks - 1)};
}
}  // namespace mcmcpp
