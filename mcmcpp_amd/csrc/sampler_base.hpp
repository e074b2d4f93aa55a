// sampler_base.hpp -- what the C ABI handle is behind include/mcmcpp_hip.h: one abstract interface, implemented by the
// fused stretch-move sampler (mcmcpp_hip.hip), the differential-evolution sampler (diffevo.hip) and the stretch move with a
// batched log-posterior callback (batch.hip).  The host code the three share is in sampler_host.hpp.  Also the owners of
// the library's HIP resources, which every handle (the analysis handles included) uses.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <utility>

#include "../../include/mcmcpp_hip.h"
#include "step_plan.hpp"

namespace mcmcpp
{
// What mcmcpp_hip_evidence_ratios writes (any pointer may be null), and one call as its entry point received it.  The handle
// fills in its own shape (dtype .. D) behind its refusals; evidence.hip does the rest.
struct EvidenceOutputs
{
    double *log_ratio, *mcse, *ess, *kish, *max_u;
    int64_t* nonfinite;
    double *log_ratio_total, *mcse_total;
    int64_t* num_draws;
};
struct EvidenceRequest
{
    const char* what;
    const void* const* steps;
    const void* device_steps;
    bool on_device;
    int64_t chain_stride_steps, n_steps, slice;
    EvidenceOutputs out;
    int32_t dtype = 0, device = -1, K = 0, W = 0, D = 0;
};
// What mcmcpp_hip_evidence_bridge writes (any pointer may be null), and one call: the request of the ratios with these outputs
// (q.out is not used).  bridge.hip does the rest.
struct BridgeOutputs
{
    double *log_ratio, *mcse, *overlap, *ess;
    int64_t *passes, *converged, *nonfinite;
    double *log_ratio_total, *mcse_total;
    int64_t* num_draws;
};
struct BridgeRequest
{
    EvidenceRequest q;
    BridgeOutputs out;
};
// What mcmcpp_hip_evidence_mbar writes (any pointer may be null), and one call: the request of the ratios with these outputs
// (q.out is not used).  mbar.hip does the rest.
struct MbarOutputs
{
    double *log_z, *cov, *log_ratio, *mcse, *ess;
    int64_t* nonfinite;
    double *log_ratio_total, *mcse_total;
    int64_t *passes, *converged, *num_draws;
};
struct MbarRequest
{
    EvidenceRequest q;
    MbarOutputs out;
};
// What mcmcpp_hip_evidence_gaussian writes (any pointer may be null), and one call: the steps of ONE chain in q (q.K is 1 and
// q.chain_stride_steps 0; q.out is not used), the Gaussian and the proposals' stream.  gaussian_bridge.hip does the rest.
struct GaussianBridgeOutputs
{
    double *log_evidence, *mcse, *overlap, *ess;
    int64_t *passes, *converged, *nonfinite, *num_draws;
    void* proposals;
    double* log_q;
};
struct GaussianBridgeRequest
{
    EvidenceRequest q;
    int32_t chain;
    const double *mean, *chol;
    uint64_t seed, stream;
    GaussianBridgeOutputs out;
};
}  // namespace mcmcpp

struct mcmcpp_hip_sampler
{
    std::string error;
    // host-side cost of the last run (mcmcpp_hip_last_run_host_timing)
    double host_enqueue_ms = 0.0, host_wall_ms = 0.0, exchange_us_per_step = 0.0;
    // split ensembles (mcmcpp_hip_last_run_exchange): bytes this rank received per ensemble step of the last run, chunks of
    // steps that had to be repeated with larger exchange blocks, slots of a block at the end of the run
    double xchg_bytes_per_step = 0.0;
    int64_t xchg_rollbacks = 0, xchg_cap_slots = 0;
    // mcmcpp_hip_run_async: the run executes on a worker thread owned by the handle; stored steps are announced as they
    // reach the caller's memory
    std::thread async_worker;
    std::mutex async_mutex;
    std::condition_variable async_cv;
    int64_t async_stored = 0;   // stored steps of the current run that are complete in chain_out
    bool async_active = false;  // a worker has been started and not yet joined
    bool async_done = true;     // the worker's run has returned
    int async_rc = 0;
    void publish_stored(int64_t count)
    {
        {
            std::lock_guard<std::mutex> lock(async_mutex);
            if (count > async_stored) async_stored = count;
        }
        async_cv.notify_all();
    }
    virtual ~mcmcpp_hip_sampler()
    {
        if (async_worker.joinable()) async_worker.join();
    }
    virtual int set_state(const void* pos, const void* logp) = 0;
    virtual int run(int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step) = 0;
    virtual int get_state(void* pos, void* logp, uint32_t* n_accept) = 0;
    virtual int reset_counters() = 0;
    virtual int seek(uint64_t steps_done) = 0;
    virtual int get_counters(uint64_t* accepted, uint64_t* steps, uint64_t* ties, uint64_t* redraws) = 0;
    virtual int calc_logp(const void* pos, int64_t count, void* out) = 0;
    virtual int last_run_timing(double* ms, int64_t* launches) = 0;
    virtual int half_step_async(int32_t color, int64_t save_slot) = 0;
    virtual int bind_device_chain(void* chain, int64_t slots) = 0;
    virtual void* device_positions() = 0;
    virtual int shard_span(int32_t color, int64_t* off, int64_t* cnt) = 0;
    virtual int synchronize() = 0;
    // per-chain calculator parameters (mcmcpp_hip_set_chain_params): the fused stretch-move sampler only
    virtual int set_chain_params(int32_t, const void*, int32_t)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED, "set_chain_params: per-chain parameters are for stretch-move handles only (not differential evolution)");
    }
    virtual int calc_logp_chain(int32_t, const void*, int64_t, void*)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED, "calc_logp_chain: per-chain parameters are for stretch-move handles only (not differential evolution)");
    }
    // one replica-exchange round among the chains of a handle (mcmcpp_hip_exchange_chains): the fused stretch-move sampler only
    virtual int exchange_chains(uint64_t, uint64_t*, uint64_t*, uint64_t*)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED,
                    "exchange_chains: replica exchange is for stretch-move handles with a device calculator only (not the differential-evolution mover, not a batch target)");
    }
    // a run with the rounds inside its launch sequence (mcmcpp_hip_run_tempered, mcmcpp_hip_run_tempered_device): likewise
    virtual int run_tempered(int64_t, int32_t, int64_t, uint64_t, void*, uint32_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, bool)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED,
                    "run_tempered: replica exchange is for stretch-move handles with a device calculator only (not the differential-evolution mover, not a batch target)");
    }
    // the ratios of normalising constants between the rungs of a ladder (mcmcpp_hip_evidence_ratios): likewise
    virtual int evidence_ratios(mcmcpp::EvidenceRequest q)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED,
                    "%s: evidence ratios are for stretch-move handles with a device calculator only (not the differential-evolution mover, not a batch target)", q.what);
    }
    // the bridge estimate of the same ratios (mcmcpp_hip_evidence_bridge): likewise
    virtual int evidence_bridge(mcmcpp::BridgeRequest b)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED,
                    "%s: evidence ratios are for stretch-move handles with a device calculator only (not the differential-evolution mover, not a batch target)", b.q.what);
    }
    // all K log-normalising constants in one joint solve (mcmcpp_hip_evidence_mbar): likewise
    virtual int evidence_mbar(mcmcpp::MbarRequest m)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED,
                    "%s: evidence ratios are for stretch-move handles with a device calculator only (not the differential-evolution mover, not a batch target)", m.q.what);
    }
    // the evidence of one chain's target by a bridge to a fitted Gaussian (mcmcpp_hip_evidence_gaussian): every mover overrides it
    virtual int evidence_gaussian(mcmcpp::GaussianBridgeRequest g) { return fail(MCMCPP_HIP_E_UNSUPPORTED, "%s: not available for this handle", g.q.what); }
    // stored steps and log-posteriors that stay in device memory (mcmcpp_hip_run_device, mcmcpp_hip_calc_logp_device): every
    // mover overrides both
    virtual int run_device(int64_t, int32_t, void*, uint32_t*) { return fail(MCMCPP_HIP_E_UNSUPPORTED, "run_device: not available for this handle"); }
    virtual int calc_logp_device(int32_t, const void*, int64_t, void*)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED, "calc_logp_device: not available for this handle");
    }
    // calc_id MCMCPP_HIP_CALC_BATCH only (batch.hip)
    virtual int set_batch_calculator(mcmcpp_hip_batch_logp_fn, void*, void*, void*)
    {
        return fail(MCMCPP_HIP_E_UNSUPPORTED, "set_batch_calculator: the handle was not created with calc_id MCMCPP_HIP_CALC_BATCH");
    }

    // A call refused because the handle is busy with an asynchronous run: the message is a literal kept beside `error`,
    // which belongs to the worker thread while it runs (only the caller's thread touches `refused`).
    const char* refused = nullptr;
    int refuse(const char* literal)
    {
        refused = literal;
        return MCMCPP_HIP_E_STATE;
    }

    int fail(int code, const char* fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        error = buf;
        return code;
    }
};

#define HIP_TRY(expr)                                                                                       \
    do                                                                                                      \
    {                                                                                                       \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return fail(MCMCPP_HIP_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)


#include "pcg128.hpp"

namespace mcmcpp
{
// ---- Owners of the HIP resources the handles hold ("Who frees what") ----------------------------
// Every device buffer, pinned host buffer, event, instantiated graph and stream of the library belongs to one of these, and
// they are the only code that gives one back to the runtime.  Move-only.  A handle quiesces its stream in its destructor's
// body; its members then free themselves, before the stream goes with the base class.

inline void free_device(void* p)
{
    if (p) (void)hipFree(p);
}
inline void free_pinned(void* p)
{
    if (p) (void)hipHostFree(p);
}

// A block of device memory (Pinned: of pinned host memory) seen as T[], and its capacity in bytes
template <class T, bool Pinned>
class HipBuffer
{
public:
    HipBuffer() = default;
    HipBuffer(const HipBuffer&) = delete;
    HipBuffer& operator=(const HipBuffer&) = delete;
    HipBuffer(HipBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    HipBuffer& operator=(HipBuffer&& o) noexcept
    {
        std::swap(p_, o.p_);  // (o frees what this held)
        std::swap(bytes_, o.bytes_);
        return *this;
    }
    ~HipBuffer() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t bytes() const { return bytes_; }

    void reset()
    {
        (Pinned ? free_pinned : free_device)(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // a new block of `bytes` in place of the old one; on failure the buffer is empty and the runtime's last error cleared
    hipError_t alloc(size_t bytes)
    {
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess)
        {
            (void)hipGetLastError();
            return e;
        }
        p_ = static_cast<T*>(p);
        bytes_ = bytes;
        return hipSuccess;
    }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
template <class T = void>
using DeviceBuffer = HipBuffer<T, false>;
template <class T = void>
using PinnedBuffer = HipBuffer<T, true>;

// The one grow rule for buffers kept from call to call: nothing if `buf` holds `bytes` already; else, once `stream` is
// idle (work on it may still use the old block), the old block goes and one of `bytes` takes its place.  Returns the
// synchronisation's error or the allocation's (the buffer is then empty and the runtime's last error cleared).
template <class T, bool Pinned>
hipError_t grow(HipBuffer<T, Pinned>& buf, size_t bytes, hipStream_t stream)
{
    if (bytes <= buf.bytes()) return hipSuccess;
    if (const hipError_t e = hipStreamSynchronize(stream)) return e;
    buf.reset();
    return buf.alloc(bytes);
}

// A hipEvent_t or hipGraphExec_t, destroyed with its owner
template <class H, hipError_t (*Destroy)(H)>
class HipHandle
{
public:
    HipHandle() = default;
    HipHandle(const HipHandle&) = delete;
    HipHandle& operator=(const HipHandle&) = delete;
    HipHandle(HipHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    HipHandle& operator=(HipHandle&& o) noexcept
    {
        std::swap(h_, o.h_);
        return *this;
    }
    ~HipHandle() { reset(); }

    operator H() const { return h_; }
    void reset()
    {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    // where a create call writes the new handle (the old one destroyed first)
    H* replace()
    {
        reset();
        return &h_;
    }

private:
    H h_ = nullptr;
};
using Event = HipHandle<hipEvent_t, hipEventDestroy>;
using GraphExec = HipHandle<hipGraphExec_t, hipGraphExecDestroy>;

// A stream of the library's own making (hipStreamCreateWithFlags(s.replace(), ...)): synchronised, then destroyed, with its
// owner.  Whatever the stream's work used must outlive it: a function declares its Stream behind its buffers, a handle
// struct as its last member.
inline hipError_t destroy_idle_stream(hipStream_t s)
{
    (void)hipStreamSynchronize(s);
    return hipStreamDestroy(s);
}
using Stream = HipHandle<hipStream_t, destroy_idle_stream>;

// What the runtime knows about a pointer that a caller says is device memory: one probe for every entry point that takes
// such a pointer.  Each caller words its own refusal.
struct DeviceRange
{
    enum Kind
    {
        NotDevice,     // a host pointer (pageable, pinned or managed) or one the runtime has never seen: never dereferenced
        OtherDevice,   // device memory of `device`, which is not the one asked about
        NoAllocation,  // the runtime does not know the allocation around it
        Found          // `room` bytes lie between the pointer and the end of its allocation
    } kind;
    int device;
    size_t room;
};
inline DeviceRange probe_device_range(const void* p, int device)
{
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();  // (some runtimes report pageable memory as an error)
    if (e != hipSuccess || at.type != hipMemoryTypeDevice) return {DeviceRange::NotDevice, -1, 0};
    if (at.device != device) return {DeviceRange::OtherDevice, at.device, 0};
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess)
    {
        (void)hipGetLastError();
        return {DeviceRange::NoAllocation, at.device, 0};
    }
    // (a pointer below the base the runtime reports has no room at all)
    return {DeviceRange::Found, at.device, (const char*)p < (const char*)base ? 0 : (size_t)((const char*)base + size - (const char*)p)};
}

inline Affine128 compose(const Affine128& g, const Affine128& f)  // g after f
{
    Affine128 r;
    r.mult = mul128(g.mult, f.mult);
    r.plus = add128(mul128(g.mult, f.plus), g.plus);
    return r;
}

// Selects device `requested` (< 0: the calling thread's current one) and reads its properties.  Every handle and entry
// point of the library opens its device here: anything but gfx950 is refused.  On failure *why holds the message.
inline int open_gfx950_device(int requested, int* device, hipDeviceProp_t* prop, std::string* why)
{
    char buf[256];
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    {
        *why = "no HIP device visible to this process";
        return MCMCPP_HIP_E_NO_DEVICE;
    }
    if (requested >= ndev)
    {
        snprintf(buf, sizeof buf, "device %d out of range (%d visible)", requested, ndev);
        *why = buf;
        return MCMCPP_HIP_E_NO_DEVICE;
    }
    int d = requested;
    hipError_t e = d >= 0 ? hipSuccess : hipGetDevice(&d);
    if (e == hipSuccess) e = hipSetDevice(d);
    if (e == hipSuccess) e = hipGetDeviceProperties(prop, d);
    if (e != hipSuccess)
    {
        snprintf(buf, sizeof buf, "cannot select device %d: %s", d, hipGetErrorString(e));
        *why = buf;
        return MCMCPP_HIP_E_HIP;
    }
    if (std::strncmp(prop->gcnArchName, "gfx950", 6) != 0)
    {
        snprintf(buf, sizeof buf, "device %d is %s; this library is built for gfx950 (MI355X) only", d, prop->gcnArchName);
        *why = buf;
        return MCMCPP_HIP_E_NO_DEVICE;
    }
    *device = d;
    return MCMCPP_HIP_OK;
}

// launch table (LaunchTable<double> / LaunchTable<float>) of a built-in or registered calculator, or nullptr
const void* launch_table_lookup(int dtype, int calc_id);
// Mover::DifferentialEvolution (diffevo.hip) and StretchMove with a batched log-posterior callback (batch.hip): see make_handle
mcmcpp_hip_sampler* make_de_sampler(const mcmcpp_hip_config& cfg, int* rc);
mcmcpp_hip_sampler* make_batch_sampler(const mcmcpp_hip_config& cfg, int* rc);
// the body of mcmcpp_hip_evidence_ratios behind the handle's refusals (evidence.hip): q's shape is the handle's, whose
// calc_logp_device evaluates the draws and whose message slot takes a failure's words
int evidence_compute(mcmcpp_hip_sampler& h, const EvidenceRequest& q);
// its checks that need no device, shared with the bridge: the used steps of a rung, or the refusal
int evidence_check(mcmcpp_hip_sampler& h, const EvidenceRequest& q, long long* used_steps);
// the body of mcmcpp_hip_evidence_bridge, likewise (bridge.hip)
int bridge_compute(mcmcpp_hip_sampler& h, const BridgeRequest& b);
// the body of mcmcpp_hip_evidence_mbar, likewise (mbar.hip)
int mbar_compute(mcmcpp_hip_sampler& h, const MbarRequest& m);
// the body of mcmcpp_hip_evidence_gaussian behind the handle's refusals (gaussian_bridge.hip): g.q's shape is the handle's, whose
// calc_logp_device evaluates the draws and the proposals with chain g.chain's parameters
int gaussian_bridge_compute(mcmcpp_hip_sampler& h, const GaussianBridgeRequest& g);
}  // namespace mcmcpp
