// diffevo_planner.hpp -- the host side of the stream planner of Mover::DifferentialEvolution in one owner: the jump tables,
// the stream head, the two batch records, the two sets of bad-position lists and their counters, and the boundary launch
// that runs the three roles of diffevo_plan.hpp on them.  Every size is a field taken from a DeBatchPlan
// (de_batch_plan.hpp); DeSampler (diffevo.hip) uses the struct as it is, and tests/cpp/de_planner_device.hip constructs it
// alone, with fields of its own choosing, to run the roles on a stream whose every draw it knows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "diffevo_plan.hpp"
#include "sampler_host.hpp"

namespace mcmcpp
{
template <class T>
struct DePlanner
{
    // ---- what a test may override between the plan and create(): these five and no others
    uint64_t threshold = 0;
    int bad_capacity = 0, resolve_capacity = 0, scan_run = kDeScanRun, batch_max = kDeBatchMax;
    // ---- from the plan and the stream, as they are
    int n = 0, dims = 0;
    U128 state0, inc;
    Affine128 batch_jump;  // (D + 3) * n * batch_max draws
    DeLaunchPlan launch;
    int scan_blocks = 0;
    // guard: bytes of kGuardByte in front of and behind the lists, the batch records and the head (the direct harness looks
    // at them after every launch; the library asks for none)
    static constexpr unsigned char kGuardByte = 0xA5;
    size_t guard = 0;

    DeviceBuffer<unsigned char> own_head, own_batch, own_bad;
    DeviceBuffer<Affine128> d_tables;  // jump_small, scan_lo, jump_lo, jump_hi, scan_hi
    DeviceBuffer<uint32_t> d_counts;
    DeHead* d_head = nullptr;
    DeBatch* d_batch = nullptr;  // batch b resolves into record b & 1
    DeBad* d_bad = nullptr;      // two sets of lists (launch_boundary)
    Affine128 *d_jump_small = nullptr, *d_scan_lo = nullptr, *d_jump_lo = nullptr, *d_jump_hi = nullptr, *d_scan_hi = nullptr;

    void take(const DeBatchPlan& p, U128 state0_, U128 inc_)
    {
        threshold = p.threshold;
        bad_capacity = p.bad_capacity;
        resolve_capacity = p.resolve_capacity;
        scan_run = p.scan_run;
        batch_max = p.batch_max;
        n = p.n, dims = p.dims;
        state0 = state0_, inc = inc_;
    }
    size_t bad_bytes() const { return sizeof(DeBad) * 2 * kDeSegments * (size_t)bad_capacity; }
    static constexpr size_t counts_bytes() { return sizeof(uint32_t) * 2 * kDeSegments * kDeCountStride; }

    // Buffers and tables for the five fields as they stand now.  The sizes that follow from them (positions, lanes, table
    // lengths) are the plan's own arithmetic, taken again where a test has changed batch_max or scan_run.
    hipError_t create()
    {
        const unsigned per = (unsigned)dims + 3u;
        launch = plan_de_launch(n, dims, batch_max, resolve_capacity);
        const DeTablePlan tp = plan_de_tables(dims, launch.updates, launch.scan_positions, scan_run);
        scan_blocks = tp.scan_blocks;
        auto guarded = [&](DeviceBuffer<unsigned char>& buf, size_t bytes) -> hipError_t {
            if (const hipError_t e = buf.alloc(bytes + 2 * guard)) return e;
            if (guard)
                if (const hipError_t e = hipMemset(buf, kGuardByte, bytes + 2 * guard)) return e;
            return hipMemset(buf.get() + guard, 0, bytes);
        };
        if (const hipError_t e = d_counts.alloc(counts_bytes())) return e;
        if (const hipError_t e = hipMemset(d_counts, 0, counts_bytes())) return e;
        if (const hipError_t e = guarded(own_bad, bad_bytes())) return e;
        if (const hipError_t e = guarded(own_head, sizeof(DeHead))) return e;
        if (const hipError_t e = guarded(own_batch, sizeof(DeBatch) * 2)) return e;
        d_bad = reinterpret_cast<DeBad*>(own_bad.get() + guard);
        d_head = reinterpret_cast<DeHead*>(own_head.get() + guard);
        d_batch = reinterpret_cast<DeBatch*>(own_batch.get() + guard);
        // the jump tables: D + 3 draws per update
        const std::vector<Affine128> small = jump_powers(pcg_jump(inc, 1), tp.small_len);
        const std::vector<Affine128> lo = jump_powers(pcg_jump(inc, per), tp.lo_len);
        const std::vector<Affine128> hi = jump_powers(pcg_jump(inc, (unsigned __int128)per * 256u), tp.hi_len);
        const std::vector<Affine128> slo = jump_powers(pcg_jump(inc, (unsigned)scan_run), tp.scan_lo_len);
        const std::vector<Affine128> shi = jump_powers(pcg_jump(inc, (unsigned __int128)scan_run * 256u), tp.scan_hi_len);
        std::vector<Affine128> all;  // one allocation
        all.insert(all.end(), small.begin(), small.end());
        all.insert(all.end(), slo.begin(), slo.end());
        all.insert(all.end(), lo.begin(), lo.end());
        all.insert(all.end(), hi.begin(), hi.end());
        all.insert(all.end(), shi.begin(), shi.end());
        if (const hipError_t e = d_tables.alloc(sizeof(Affine128) * all.size())) return e;
        if (const hipError_t e = hipMemcpy(d_tables, all.data(), sizeof(Affine128) * all.size(), hipMemcpyHostToDevice)) return e;
        d_jump_small = d_tables;
        d_scan_lo = d_jump_small + small.size();
        d_jump_lo = d_scan_lo + slo.size();
        d_jump_hi = d_jump_lo + lo.size();
        d_scan_hi = d_jump_hi + hi.size();
        batch_jump = pcg_jump(inc, (unsigned __int128)per * (unsigned)n * (unsigned)batch_max);
        return hipSuccess;
    }

    // The stream at its beginning: nothing resolved, nothing listed (asynchronous, on `stream`)
    hipError_t rewind(hipStream_t stream)
    {
        std::memset(&head0, 0, sizeof head0);
        head0.state = state0;
        head0.provisional[0] = state0;  // (batches 0 and 1 are scanned before anything has been resolved)
        head0.provisional[1] = apply(batch_jump, state0);
        if (const hipError_t e = hipMemcpyAsync(d_head, &head0, sizeof head0, hipMemcpyHostToDevice, stream)) return e;
        return hipMemsetAsync(d_counts, 0, counts_bytes(), stream);
    }

    // The boundary launch in front of a batch: the resolve of batch `resolve_batch` (scanned before), the records of batch
    // `record_batch` (resolved before) into `recs`, and the scan of batch `scan_batch`; any of them < 0: not in this launch
    // (priming).
    void launch_boundary(long long resolve_batch, long long record_batch, long long scan_batch, DeRec<T>* recs, hipStream_t stream)
    {
        DePlanArgs p;
        std::memset(&p, 0, sizeof p);
        p.head = d_head;
        p.scan_hi = d_scan_hi;
        p.scan_lo = d_scan_lo;
        p.jump_hi = d_jump_hi;
        p.jump_lo = d_jump_lo;
        p.jump_small = d_jump_small;
        p.batch_jump = batch_jump;
        p.inc = inc;
        p.threshold = threshold;
        p.n = n;
        p.dims = dims;
        p.updates = launch.updates;
        p.positions = launch.positions;
        p.scan_positions = launch.scan_positions;
        p.scan_run = scan_run;
        p.seg_len = launch.seg_len;
        p.bad_capacity = bad_capacity;
        // two sets of lists: batch b is scanned into set b & 1 (its resolve runs beside the scan of batch b + 1)
        const long long sb = scan_batch >= 0 ? scan_batch : resolve_batch + 1;
        p.scan_parity = (int)(sb & 1);
        p.bad = d_bad + (size_t)(sb & 1) * kDeSegments * (size_t)bad_capacity;
        p.counts = d_counts + (size_t)(sb & 1) * kDeSegments * kDeCountStride;
        p.resolve_bad = d_bad + (size_t)((sb + 1) & 1) * kDeSegments * (size_t)bad_capacity;
        p.resolve_counts = d_counts + (size_t)((sb + 1) & 1) * kDeSegments * kDeCountStride;
        p.batch = d_batch + (resolve_batch >= 0 ? (resolve_batch & 1) : 0);
        const int resolve = resolve_batch >= 0 ? 1 : 0;
        const int record_blocks = record_batch >= 0 ? launch.record_blocks : 0;
        const int scan_now = scan_batch >= 0 ? scan_blocks : 0;
        const size_t lds = de_launch_lds(launch, resolve != 0, record_blocks != 0);
        hipLaunchKernelGGL((de_boundary_kernel<T>), dim3((unsigned)(resolve + record_blocks + scan_now)), dim3(kDePlanThreads), lds, stream, p, resolve, resolve_capacity,
                           record_blocks, d_batch + (record_batch >= 0 ? (record_batch & 1) : 0), recs);
    }

    // Behind a rewind: batch 0 scanned and resolved, batch 1 scanned -- what the boundary in front of a batch finds
    void prime(hipStream_t stream)
    {
        launch_boundary(-1, -1, 0, nullptr, stream);
        launch_boundary(0, -1, 1, nullptr, stream);
    }

private:
    DeHead head0;  // (the source of rewind's copy: it outlives the call)
};
}  // namespace mcmcpp
