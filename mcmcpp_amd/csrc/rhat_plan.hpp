// rhat_plan.hpp -- how rhat.hip computes the Gelman-Rubin split R-hat: the one summation shape every sum of the family has
// (sum_fixed: include/mcmcpp_hip.h), which steps make a sequence, the steps of an upload chunk, how the elements of a step row
// are tiled over blocks, whether a lane walks all slices of its sequence or one block takes each (element tile, slice), and
// which steps of which slices a block walks in one chunk -- as pure functions of plain numbers.  No HIP header: this file
// compiles with the host compiler alone, and tests/test_rhat_plan.py checks it there over a grid of shapes.  rhat.hip turns a
// plan into launches and buffer sizes, and its kernels walk the slices by rhat_slice_walk; it holds no threshold of its own.
#pragma once

#include <cstddef>
#include <cstdint>

#include "step_chunks.hpp"

#if defined(__HIPCC__)
#define RHAT_HD __host__ __device__ __forceinline__
#else
#define RHAT_HD inline
#endif

namespace mcmcpp
{
constexpr int kRhatPlanThreads = 256;      // threads per block of every kernel of the family
constexpr int kRhatRowsInFlight = 8;       // rows whose loads a lane of the series kernel has in flight
constexpr int kRhatMaxChains = 1024, kRhatMaxParams = 1024;
constexpr long long kRhatMinSlice = 1024;  // a sum of up to 1024 terms is one sequential sum
constexpr int kRhatMaxSlices = 64;
constexpr int kRhatWave = 64;
constexpr int kRhatOwnWavesPerCu = 8;      // lanes own whole sequences where that alone gives every CU this many wavefronts
constexpr int kRhatVectorBytes = 16;
constexpr long long kRhatGridXMax = 2147483647, kRhatGridYMax = 65535, kRhatGridZMax = 65535;

// sum_fixed over v[0..N): consecutive slices of rhat_slice_len(N) terms (the last may be short), each summed in ascending
// order from +0, then the slice sums added in ascending order
RHAT_HD long long rhat_slice_len(long long N)
{
    const long long per = ((N + 63) / 64 + 63) / 64 * 64;
    return per < kRhatMinSlice ? kRhatMinSlice : per;
}
RHAT_HD int rhat_slices(long long N) { return (int)((N + rhat_slice_len(N) - 1) / rhat_slice_len(N)); }

// The sequences of K chains of n used steps of W walkers: H halves of L steps each; sequence m = (k H + h) W + w
struct RhatShape
{
    int H;
    long long L, M;
};
inline RhatShape rhat_shape(int K, long long n, int W, int split)
{
    RhatShape s;
    s.H = split ? 2 : 1;
    s.L = split ? n / 2 : n;
    s.M = (long long)K * s.H * W;
    return s;
}
RHAT_HD long long rhat_half_begin(long long n, long long L, int h) { return h ? n - L : 0; }  // half h: used steps [begin, begin + L)
RHAT_HD long long rhat_sequence(int k, int h, long long w, int H, long long W) { return ((long long)k * H + h) * W + w; }

// steps of an upload chunk (MCMCPP_HIP_RHAT_CHUNK_MB): one at the least; the chunks are walked by for_each_step_chunk
inline long long rhat_steps_per_chunk(size_t chunk_bytes, size_t step_bytes)
{
    const size_t per = chunk_bytes / step_bytes;
    return per < 1 ? 1 : (long long)(per > (size_t)1 << 62 ? (size_t)1 << 62 : per);
}

// elements a lane takes of a row: one 16-byte piece where every row is whole pieces and the base is aligned (every step and
// chain stride is a whole number of rows), else one element
inline int rhat_vector_width(size_t elem_bytes, long long E, uintptr_t base)
{
    return ((size_t)E * elem_bytes) % kRhatVectorBytes == 0 && base % kRhatVectorBytes == 0 ? (int)(kRhatVectorBytes / elem_bytes) : 1;
}

// The series kernel's launch for `zs` (chain, half) pairs of E elements each: grid (etiles, slice_blocks, zs).  own: a lane
// walks every slice of its sequence and keeps the running total (2 slots of state per series: the total, the open slice);
// else block y takes slice y alone (a slot per slice).  cus: the device's CU count, or MCMCPP_HIP_RHAT_PLAN_CUS (rhat_plan_cus):
// it decides between the two and nothing else -- no result depends on it.
struct RhatSeriesPlan
{
    int vec = 1, own = 0, slices = 0, slots = 0;
    long long lanes = 0, waves = 0, slen = 0;  // lanes along a row; wavefronts with a lane at work when every lane owns its sequences
    unsigned etiles = 0, slice_blocks = 0, zs = 0;
};
inline RhatSeriesPlan rhat_series_plan(long long E, int vec, long long L, int zs, int cus)
{
    RhatSeriesPlan p;
    p.vec = vec;
    p.lanes = (E + vec - 1) / vec;
    p.etiles = (unsigned)((p.lanes + kRhatPlanThreads - 1) / kRhatPlanThreads);
    p.zs = (unsigned)zs;
    p.slen = rhat_slice_len(L);
    p.slices = rhat_slices(L);
    p.waves = (p.lanes + kRhatWave - 1) / kRhatWave * zs;
    p.own = p.slices == 1 || p.waves >= (long long)kRhatOwnWavesPerCu * cus;
    p.slots = p.own ? 2 : p.slices;
    p.slice_blocks = p.own ? 1u : (unsigned)p.slices;
    return p;
}

// the CU count the plan is made for: the device's, unless the environment names another (read per call; a value >= 1)
inline int rhat_plan_cus(int device_cus)
{
    if (const char* env = std::getenv("MCMCPP_HIP_RHAT_PLAN_CUS"))
    {
        const long long v = std::atoll(env);
        if (v >= 1 && v <= 1 << 20) return (int)v;
    }
    return device_cus;
}

// The slices block y walks: all of them, or slice y
RHAT_HD void rhat_block_slices(int own, int slices, int y, int* t0, int* t1)
{
    *t0 = own ? 0 : y;
    *t1 = own ? slices : y + 1;
}

// What a lane does with slice t of its half (used steps [a, a + L)) in the chunk that holds used steps [g0, g1): it walks
// steps [s, f) (nothing if s >= f); fresh: the slice starts here, its sums start from +0 (else they come from the state);
// closes: the slice ends here, its sums are final.
struct RhatWalk
{
    long long s, f;
    int fresh, closes;
};
RHAT_HD RhatWalk rhat_slice_walk(long long a, long long L, long long slen, int t, long long g0, long long g1)
{
    const long long b = a + (long long)t * slen;
    const long long e = b + slen < a + L ? b + slen : a + L;
    RhatWalk w;
    w.s = b > g0 ? b : g0;
    w.f = e < g1 ? e : g1;
    w.fresh = w.s == b;
    w.closes = w.f == e;
    return w;
}

// The combine: sum_fixed over the N items of each of G segments of [M][P], one thread per (slice, parameter)
struct RhatSumPlan
{
    long long slen = 0;
    int slices = 0;
    unsigned blocks = 0, segments = 0;
};
inline RhatSumPlan rhat_sum_plan(long long N, int P, int G)
{
    RhatSumPlan p;
    p.slen = rhat_slice_len(N);
    p.slices = rhat_slices(N);
    p.blocks = (unsigned)(((long long)p.slices * P + kRhatPlanThreads - 1) / kRhatPlanThreads);
    p.segments = (unsigned)G;
    return p;
}
}  // namespace mcmcpp
