// step_chunks.hpp -- the arithmetic the analysis entry points share when they take stored steps a chunk at a time (moments.hip,
// autocorr.hip, histograms.hip, quantiles.hip; analysis_host.hpp holds the HIP side): the chunk-size knob, the walk over the
// chunks, and which steps of a chunk follow each other in memory and so go in one copy.  Host-only, no HIP header: tested on
// the CPU (tests/test_step_chunks.py).  How many steps a chunk holds is each family's own rule (hist_plan.hpp,
// quantile_plan.hpp, moments.hip) and is passed in as `per`.
#pragma once

#include <cstddef>
#include <cstdlib>

namespace mcmcpp
{
// A *_CHUNK_MB environment knob in bytes: a value >= 1 (atoll) replaces the default
inline size_t chunk_bytes_from_env(const char* name, size_t default_mb)
{
    size_t mb = default_mb;
    if (const char* env = std::getenv(name))
    {
        const long long v = std::atoll(env);
        if (v >= 1) mb = (size_t)v;
    }
    return mb << 20;
}

// f(k0, now) for every chunk of `used` steps, `per` (>= 1) at a time, in order: chunk i covers steps [k0, k0 + now) with
// k0 = i * per; the last one may be ragged, and none is empty (used == 0: f is never called).  Stops at f's first non-zero
// result and returns it.
template <class F>
int for_each_step_chunk(long long used, long long per, F&& f)
{
    for (long long k0 = 0; k0 < used; k0 += per)
        if (int rc = f(k0, (used - k0 < per) ? used - k0 : per)) return rc;
    return 0;
}

// How many of the steps [k, end) follow each other in memory from step k on (at least one; never past `end`, the end of the
// chunk).  src_of(k) is the address of step k: an entry of a pointer list, or base + k * stride of a flat chain.
template <class SrcOf>
long long contiguous_run(SrcOf&& src_of, long long k, long long end, size_t step_bytes)
{
    const char* src = (const char*)src_of(k);
    long long run = 1;
    while (k + run < end && (const char*)src_of(k + run) == src + step_bytes * (size_t)run) ++run;
    return run;
}
}  // namespace mcmcpp
