// de_planner_device.hip -- the stream planner of Mover::DifferentialEvolution alone, callable from tests/test_de_planner.py:
// no sampler handle, no calculator, no oracle.
//
// The production de_boundary_kernel<T> (diffevo_plan.hpp) runs unchanged, driven by the production DePlanner<T>
// (diffevo_planner.hpp) built from the production plan (de_batch_plan.hpp); a test may override the five fields DePlanner
// names and nothing else.  One launch at a time, a synchronisation after each; then the head, a batch record, the records
// or a set of lists can be read.  The lists, the batch records, the head and the record array lie between guard bytes of a
// known pattern, which are looked at after every launch.  Built by the test with the flags of mcmcpp_amd/csrc/Makefile.
// Every function returns 0, a HIP error code, -1 for arguments with which a kernel would leave its buffers (the kernels
// trust their caller) or -2 for a guard that no longer holds its pattern: nothing aborts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "diffevo_planner.hpp"

using namespace mcmcpp;

namespace
{
const size_t kGuard = 4096;  // bytes on either side (a multiple of every alignment in play)

struct HarnessBase
{
    virtual ~HarnessBase() {}
    virtual int info(long long* out) = 0;
    virtual int prime(int launches) = 0;
    virtual int boundary(long long b) = 0;
    virtual int read(int what, int which, void* out, size_t bytes) = 0;
};

template <class T>
struct Harness final : HarnessBase
{
    DePlanner<T> pl;
    DeviceBuffer<unsigned char> own_recs;
    DeRec<T>* recs = nullptr;
    size_t recs_bytes = 0;

    // what the kernels trust their caller for, with the fields as a test left them
    bool fields_ok() const
    {
        const long long per = pl.dims + 3;
        if (pl.n < 2 || pl.n > (1 << 30) || pl.dims < 1 || pl.dims > 1024 || pl.batch_max < 1 || pl.scan_run < 1 || pl.bad_capacity < 1 || pl.resolve_capacity < 1) return false;
        const long long updates = (long long)pl.n * pl.batch_max;
        if (updates > (1LL << 23)) return false;  // (the walk's keys)
        const long long scan_positions = per * (updates - 1) + 2 * (kDeShiftMax + 1);
        if (scan_positions + pl.scan_run > 2147483647LL) return false;
        if ((((scan_positions - 1) / per) << 8 | 0xFF) > 0xFFFFFFFFLL) return false;
        if (de_resolve_lds_bytes(pl.resolve_capacity, (int)per) > 65536) return false;  // (a plain launch's LDS)
        if ((size_t)pl.bad_capacity > ((size_t)1 << 20)) return false;
        // the scan's fast path for a power-of-two half draws no 64-bit value: it is sound at threshold 0 alone
        if ((pl.n & (pl.n - 1)) == 0 && pl.threshold != 0) return false;
        return true;
    }

    int create()
    {
        if (!fields_ok()) return -1;
        pl.guard = kGuard;
        if (const hipError_t e = pl.create()) return (int)e;
        recs_bytes = sizeof(DeRec<T>) * (size_t)pl.launch.updates;
        if (const hipError_t e = own_recs.alloc(recs_bytes + 2 * kGuard)) return (int)e;
        if (const hipError_t e = hipMemset(own_recs, DePlanner<T>::kGuardByte, recs_bytes + 2 * kGuard)) return (int)e;
        recs = reinterpret_cast<DeRec<T>*>(own_recs.get() + kGuard);
        return 0;
    }

    int info(long long* o) override
    {
        const long long v[] = {pl.batch_max, pl.launch.updates, pl.launch.positions, pl.launch.scan_positions, pl.launch.seg_len, pl.bad_capacity, pl.resolve_capacity,
                               pl.scan_run, pl.scan_blocks, pl.launch.record_blocks, (long long)pl.threshold, (long long)(pl.threshold >> 32), (long long)sizeof(DeBatch),
                               (long long)sizeof(DeRec<T>), (long long)sizeof(DeHead), (long long)de_launch_lds(pl.launch, true, true)};
        memcpy(o, v, sizeof v);
        return 0;
    }

    static int guard_of(const DeviceBuffer<unsigned char>& buf, size_t inner)
    {
        std::vector<unsigned char> g(2 * kGuard);
        if (const hipError_t e = hipMemcpy(g.data(), buf.get(), kGuard, hipMemcpyDeviceToHost)) return (int)e;
        if (const hipError_t e = hipMemcpy(g.data() + kGuard, buf.get() + kGuard + inner, kGuard, hipMemcpyDeviceToHost)) return (int)e;
        for (unsigned char c : g)
            if (c != DePlanner<T>::kGuardByte) return -2;
        return 0;
    }
    int settle()
    {
        if (const hipError_t e = hipGetLastError()) return (int)e;
        if (const hipError_t e = hipDeviceSynchronize()) return (int)e;
        if (int rc = guard_of(pl.own_bad, pl.bad_bytes())) return rc;
        if (int rc = guard_of(pl.own_batch, sizeof(DeBatch) * 2)) return rc;
        if (int rc = guard_of(pl.own_head, sizeof(DeHead))) return rc;
        return guard_of(own_recs, recs_bytes);
    }

    // launches: 0 = rewind only; 1 = the first priming launch (the scan of batch 0); 2 = the second (the resolve of batch 0, the
    // scan of batch 1) -- in this order, one call each, so that the test sees the stream after either
    int prime(int launches) override
    {
        if (launches == 0)
        {
            if (const hipError_t e = pl.rewind(nullptr)) return (int)e;
        }
        else if (launches == 1)
            pl.launch_boundary(-1, -1, 0, nullptr, nullptr);
        else if (launches == 2)
            pl.launch_boundary(0, -1, 1, nullptr, nullptr);
        else
            return -1;
        return settle();
    }
    // the boundary in front of batch b: the resolve of b + 1, the records of b, the scan of b + 2
    int boundary(long long b) override
    {
        if (b < 0) return -1;
        pl.launch_boundary(b + 1, b, b + 2, recs, nullptr);
        return settle();
    }
    // what: 0 head; 1 batch record `which`; 2 the records; 3 the lists of set `which`; 4 the counters of set `which`
    int read(int what, int which, void* out, size_t bytes) override
    {
        const void* src = nullptr;
        size_t have = 0;
        if (which < 0 || which > 1) return -1;
        if (what == 0) src = pl.d_head, have = sizeof(DeHead);
        if (what == 1) src = pl.d_batch + which, have = sizeof(DeBatch);
        if (what == 2) src = recs, have = recs_bytes;
        if (what == 3) src = pl.d_bad + (size_t)which * kDeSegments * (size_t)pl.bad_capacity, have = pl.bad_bytes() / 2;
        if (what == 4) src = pl.d_counts + (size_t)which * kDeSegments * kDeCountStride, have = DePlanner<T>::counts_bytes() / 2;
        if (!src || !out || bytes != have) return -1;
        return (int)hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost);
    }
};

// overrides: {threshold lo32, threshold hi32, bad_capacity, resolve_capacity, scan_run, batch_max}, each -1 for the plan's
// own value (the threshold: both halves -1)
template <class T>
int make(uint64_t seed, int n, int dims, const long long* ov, HarnessBase** out)
{
    if (n < 2 || dims < 1 || !ov || !out) return -1;
    // scan_run and batch_max enter the plan the way the environment's knobs do, so that the capacities follow them
    const DeBatchPlan bp = plan_de_batch(n, dims, ov[5] >= 0 && ov[5] <= kDeBatchMax, (long)ov[5], ov[4] >= 0, (long)ov[4]);
    if (!bp.ok) return -3;
    Harness<T>* h = new (std::nothrow) Harness<T>;
    if (!h) return -1;
    U128 state0, inc;
    pcg_seed(seed, 0, &state0, &inc);
    h->pl.take(bp, state0, inc);
    if (ov[0] >= 0 && ov[1] >= 0) h->pl.threshold = ((uint64_t)ov[1] << 32) | (uint64_t)ov[0];
    if (ov[2] >= 0) h->pl.bad_capacity = (int)ov[2];
    if (ov[3] >= 0) h->pl.resolve_capacity = (int)ov[3];
    if (ov[5] > kDeBatchMax) h->pl.batch_max = (int)ov[5];  // (longer than any plan: a test's way to more events than a plan allows)
    const int rc = h->create();
    if (rc)
    {
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}
}  // namespace

extern "C"
{
int dp_create(int f32, uint64_t seed, int n, int dims, const long long* overrides, void** handle)
{
    HarnessBase* h = nullptr;
    const int rc = f32 ? make<float>(seed, n, dims, overrides, &h) : make<double>(seed, n, dims, overrides, &h);
    if (handle) *handle = h;
    return rc;
}
void dp_destroy(void* h) { delete static_cast<HarnessBase*>(h); }
int dp_info(void* h, long long* out) { return h && out ? static_cast<HarnessBase*>(h)->info(out) : -1; }
int dp_prime(void* h, int launches) { return h ? static_cast<HarnessBase*>(h)->prime(launches) : -1; }
int dp_boundary(void* h, long long b) { return h ? static_cast<HarnessBase*>(h)->boundary(b) : -1; }
int dp_read(void* h, int what, int which, void* out, size_t bytes) { return h ? static_cast<HarnessBase*>(h)->read(what, which, out, bytes) : -1; }
}
