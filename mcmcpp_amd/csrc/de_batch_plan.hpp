// de_batch_plan.hpp -- how diffevo.hip sizes the stream planner of Mover::DifferentialEvolution (scheme: diffevo_kernel.hpp):
// the half-steps of a batch, the stream positions a scan looks at, the bad-position lists and the resolver's LDS, the scan's
// grid, the five jump tables, and the numbers of one boundary launch -- as pure functions of plain numbers.  No HIP header:
// this file compiles with the host compiler alone, and tests/test_de_batch_plan.py checks it there over a grid of shapes.
// DePlanner (diffevo_planner.hpp) turns a plan into buffers and launches; diffevo.hip holds no threshold of its own.  The
// planner's constants live here, beside the arithmetic that depends on them; the device code takes them from this file.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mcmcpp
{
constexpr int kDeBatchMax = 64;     // half-steps one plan covers at most
constexpr int kDeShiftMax = 4095;   // thrown-away draws inside one batch that are followed exactly (expected: about one per half-step)
constexpr int kDeWindow = 32;       // raw draws one update's integer part may consume (2 + up to 30 thrown away: even two
                                    // walkers per half, where every second ind2 collides, overrun once in 1e9 updates)
constexpr int kDeOverrun = 255;     // E of a start whose update would not fit that window
constexpr int kDeSegments = 64;     // bad-position lists of a batch (by position)
constexpr int kDeCountStride = 32;  // uint32 between two list counters: one 128-byte line each
constexpr int kDeMaxBad = 8192;     // bad positions of a batch the resolver holds (about (D + 3) per half-step)
constexpr int kDeMaxEvents = 1024;  // events of a batch
constexpr int kDeScanRun = 8;       // consecutive stream positions one scanning lane steps through (default)
constexpr int kDePlanThreads = 256;
constexpr long long kDeRecordUpdates = 8LL << 20;  // updates of a batch: 256 MiB of 32-byte records
constexpr size_t kDeEventBytes = 8;                // sizeof(DePlan)

// what cut the batch of a plan (and, where nothing is left of it, what refused the shape)
enum DeBatchBound
{
    kDeBoundKnob = 0,       // MCMCPP_HIP_DE_BATCH, or kDeBatchMax
    kDeBoundPositions = 1,  // the 32-bit position counters: 2^30 stream positions a batch
    kDeBoundLists = 2,      // the resolver's lists: kDeMaxBad bad positions a batch
    kDeBoundRecords = 3,    // the record memory: kDeRecordUpdates updates a batch
};

struct DeBatchPlan
{
    bool ok = false;             // false: the shape is refused (bound says why); nothing below `by_records` is meaningful
    int bound = kDeBoundKnob;    // the smallest of the four bounds (the first of equals, in the order above)
    int n = 0, dims = 0, per = 0;
    long long by_positions = 0, by_lists = 0, by_records = 0;
    int batch_max = 0;           // half-steps a batch plans
    int scan_run = 0;            // MCMCPP_HIP_DE_SCAN_RUN, at least 1
    uint64_t threshold = 0;      // (2^64 - n) mod n: pcg's bounded_rand throws away what lies below
    long long updates_max = 0;   // n * batch_max
    long long positions_max = 0; // what a scan looks at
    long long expected = 0;      // bad positions among them (one in n), rounded up
    int bad_capacity = 0;        // entries of one of the kDeSegments lists
    int resolve_capacity = 0;    // entries of the resolver's LDS
    long long scan_lanes = 0;
    int scan_blocks = 0;
    // the jump tables, in the order they lie in their one allocation
    size_t small_len = 0, scan_lo_len = 0, lo_len = 0, hi_len = 0, scan_hi_len = 0;
};

// The scan's lanes and workgroups and the lengths of the five jump tables, in the order the tables lie in their one allocation
struct DeTablePlan
{
    long long scan_lanes = 0;
    int scan_blocks = 0;
    size_t small_len = 0, scan_lo_len = 0, lo_len = 0, hi_len = 0, scan_hi_len = 0;
};
inline DeTablePlan plan_de_tables(int dims, long long updates, long long scan_positions, int scan_run)
{
    DeTablePlan t;
    t.scan_lanes = (scan_positions + scan_run - 1) / scan_run;
    t.scan_blocks = (int)((t.scan_lanes + kDePlanThreads - 1) / kDePlanThreads);
    t.small_len = (size_t)kDeShiftMax + (size_t)dims + 2;  // j draws: a shift (<= kDeShiftMax), the D draws to the accept draw
    t.scan_lo_len = 256;                                   // scan_run * j draws
    t.lo_len = 256;                                        // (D + 3) * j draws
    t.hi_len = ((size_t)updates + 255) / 256;              // (D + 3) * 256 * j draws
    t.scan_hi_len = ((size_t)t.scan_lanes + 255) / 256;    // scan_run * 256 * j draws: one entry per scanning workgroup
    return t;
}

// knob_batch, knob_scan_run: the values of MCMCPP_HIP_DE_BATCH and MCMCPP_HIP_DE_SCAN_RUN where the environment names them
// (has_*); both are clamped to 1 from below
inline DeBatchPlan plan_de_batch(int n, int dims, bool has_batch, long knob_batch, bool has_scan_run, long knob_scan_run)
{
    DeBatchPlan p;
    p.n = n, p.dims = dims, p.per = dims + 3;
    p.threshold = (uint64_t)(0 - (uint64_t)n) % (uint64_t)n;
    const int run = has_scan_run ? (int)knob_scan_run : kDeScanRun;
    p.scan_run = run < 1 ? 1 : run;
    // the batch: as many half-steps as the position counters (32 bits), the resolver's lists and a sensible amount of
    // record memory (256 MiB) allow
    const long long per = p.per;
    const int asked = has_batch ? (int)knob_batch : kDeBatchMax;
    long long b = asked < 1 ? 1 : (asked > kDeBatchMax ? kDeBatchMax : asked);
    p.by_positions = ((1LL << 30) - 2 * (kDeShiftMax + 1)) / (per * n);
    p.by_lists = (kDeMaxBad * 5LL / 8 - 2 * (kDeShiftMax + 1) / n) / per;
    p.by_records = kDeRecordUpdates / n;
    p.bound = kDeBoundKnob;
    if (p.by_positions < b) b = p.by_positions, p.bound = kDeBoundPositions;
    if (p.by_lists < b) b = p.by_lists, p.bound = kDeBoundLists;
    if (p.by_records < b) b = p.by_records, p.bound = kDeBoundRecords;
    if (b < 1) return p;
    p.ok = true;
    p.batch_max = (int)b;
    p.updates_max = b * n;
    p.positions_max = per * (p.updates_max - 1) + 2 * (kDeShiftMax + 1);
    // one stream position in n is bad: a batch lists about (D + 3) of them per half-step (and as many again as the
    // kDeShiftMax positions behind its end hold, which matters for tiny ensembles), spread evenly over the lists
    p.expected = p.positions_max / n + 1;
    p.bad_capacity = (int)(4 * ((p.expected + kDeSegments - 1) / kDeSegments) + 64);
    const long long cap = 2 * p.expected + 512;
    p.resolve_capacity = cap > kDeMaxBad ? kDeMaxBad : (int)cap;
    const DeTablePlan t = plan_de_tables(dims, p.updates_max, p.positions_max, p.scan_run);
    p.scan_lanes = t.scan_lanes, p.scan_blocks = t.scan_blocks;
    p.small_len = t.small_len, p.scan_lo_len = t.scan_lo_len, p.lo_len = t.lo_len, p.hi_len = t.hi_len, p.scan_hi_len = t.scan_hi_len;
    return p;
}

// what a refusal says of the bound that fired
inline const char* de_batch_bound_text(int bound)
{
    switch (bound)
    {
    case kDeBoundPositions: return "its 32-bit position counters: 2^30 stream positions";
    case kDeBoundLists: return "the resolver's lists: 8192 bad stream positions, of which 8192 / (walkers per half) lie behind the batch's end";
    case kDeBoundRecords: return "its record memory: 8 Mi updates";
    default: return "the batch knob";
    }
}

// LDS of the resolving workgroup: capacity + 2 * per + 2 + kDeSegments uint32 (de_resolve_block)
inline size_t de_resolve_lds_bytes(int capacity, int per) { return sizeof(uint32_t) * ((size_t)capacity + 2 * (size_t)per + 2 + kDeSegments); }

// The numbers of one boundary launch that planning a batch of `batch_max` half-steps fixes
struct DeLaunchPlan
{
    int updates = 0;         // n * batch_max
    int positions = 0;       // stream positions an update of the batch can start at
    int scan_positions = 0;  // positions the scan looks at, from its provisional start
    int seg_len = 0;         // positions per list
    int record_blocks = 0;   // workgroups that make the batch's records
    size_t resolve_lds = 0, records_lds = 0;  // dynamic LDS bytes of a launch that resolves / makes records (the larger one holds)
};
inline DeLaunchPlan plan_de_launch(int n, int dims, int batch_max, int resolve_capacity)
{
    DeLaunchPlan l;
    const long long per = dims + 3;
    l.updates = n * batch_max;
    l.positions = (int)(per * (long long)(l.updates - 1) + kDeShiftMax + 1);
    l.scan_positions = l.positions + kDeShiftMax + 1;
    l.seg_len = (l.scan_positions + kDeSegments - 1) / kDeSegments;
    l.record_blocks = (l.updates + kDePlanThreads - 1) / kDePlanThreads;
    l.resolve_lds = de_resolve_lds_bytes(resolve_capacity, dims + 3);
    l.records_lds = kDeEventBytes * kDeMaxEvents;
    return l;
}
inline size_t de_launch_lds(const DeLaunchPlan& l, bool resolve, bool records)
{
    const size_t a = resolve ? l.resolve_lds : 0, b = records ? l.records_lds : 0;
    return a > b ? a : b;
}
}  // namespace mcmcpp
