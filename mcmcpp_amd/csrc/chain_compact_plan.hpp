// chain_compact_plan.hpp -- how chain_ops.hip compacts a device-resident chain in place (sliceAndBurnChain on the device): which
// stored steps are kept, where each comes from, and the waves of destination steps that one launch each may move -- as pure
// functions of plain numbers.  No HIP header: this file compiles with the host compiler alone, and tests/test_device_facade.py
// checks it there for every small (n_steps, burn_in, interval).  chain_ops.hip turns a wave into a launch; it holds no
// selection rule of its own.
//
// The selection is the reference's (MCMCpp/Chain/Chain.h:268-305), as the host Chain restates it: nothing to do for
// burn_in = 0 and interval = 1; an empty chain when no step is left behind the burn-in or fewer than `interval` are; otherwise
// destination step j is source step burn_in + j * interval, for every source below n_steps.
//
// Waves.  A source index is never below its destination's, so source and destination ranges overlap and one launch over all
// destinations would let one block overwrite a step another block has yet to read.  Destinations are therefore moved in
// ascending waves [first, first + count), one launch each on one stream, with
//     first + count <= source(first):
// sources ascend with their destinations, so every source of the wave lies at or behind the wave's end -- a wave writes no step
// that it reads -- and every source of a later wave lies at or behind that wave's own first destination, which no earlier wave
// has written.  Launches of one stream run one after the other: no step is written before its last reader is done.  A
// destination that is its own source (step 0 without burn-in) is skipped.  With burn_in = b > 0 the waves hold b, b * interval + b,
// ... steps (they grow geometrically for interval > 1 and stay at b for interval = 1: a pure shift by b takes kept / b launches).
#pragma once

#include <cstdint>

namespace mcmcpp
{
// stored steps after the compaction
inline int64_t chain_compact_kept(int64_t n_steps, int64_t burn_in, int64_t interval)
{
    if (burn_in == 0 && interval == 1) return n_steps;
    if (n_steps <= burn_in || n_steps - burn_in < interval) return 0;
    return (n_steps - burn_in + interval - 1) / interval;
}

// the step that destination step j is copied from
inline int64_t chain_compact_source(int64_t j, int64_t burn_in, int64_t interval) { return burn_in + j * interval; }

// destinations [first, first + count) of one launch
struct ChainCompactWave
{
    int64_t first, count;
};

// The wave behind `done` destinations that are in place already (start with 0, go on with first + count); false when none is left.
inline bool chain_compact_wave(int64_t done, int64_t kept, int64_t burn_in, int64_t interval, ChainCompactWave* wave)
{
    if (burn_in == 0 && interval == 1) return false;  // every step is its own source
    if (done < kept && chain_compact_source(done, burn_in, interval) == done) ++done;  // (step 0 without burn-in; no other)
    if (done >= kept) return false;
    int64_t end = chain_compact_source(done, burn_in, interval);  // > done
    if (end > kept) end = kept;
    wave->first = done;
    wave->count = end - done;
    return true;
}
}  // namespace mcmcpp
