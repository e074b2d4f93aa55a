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
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <utility>

#include "../../include/mcmcpp_hip.h"

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
// Every device buffer, pinned host buffer, event and instantiated graph of the library belongs to one of these, and they
// are the only code that gives one back to the runtime.  Move-only.  A handle quiesces its stream in its destructor's
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

inline int pow2_at_least(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int ilog2(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
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

inline std::optional<long> env_long(const char* name)
{
    const char* v = std::getenv(name);
    if (v && *v) return std::strtol(v, nullptr, 10);
    return std::nullopt;
}
inline long env_long(const char* name, long fallback) { return env_long(name).value_or(fallback); }

// The library's tuning knobs (environment variables, DESIGN.md section 9 lists them).  Read ONCE, when a handle is
// created; nothing on the launch path touches the environment.  Negative "unset" values mean "library default"; a knob
// whose default differs between the movers is left empty when unset (-1 is one of its values).
struct Knobs
{
    long passes;                  // MCMCPP_HIP_PASSES                   walkers-per-wavefront rounds of the half-step kernels (0: chosen from the size)
    long waves_per_simd;          // MCMCPP_HIP_WAVES_PER_SIMD           wavefronts per SIMD to reach before a wavefront takes more walkers (2)
    long matrix_core_min_walkers; // MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS  smallest shard stepped by the matrix-core kernels (0; -1: never)
    std::optional<long> matrix_core_4pass;  // MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS from this many updates per launch on: 16 walkers per wavefront
                                            //                                      (stretch 18432, differential evolution 32768)
    long matrix_core_late;        // MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS    from this many updates per launch on: the 16-walker wavefronts make their next draws behind the accept, four to a SIMD (49152; -1: never)
    long full_step;               // MCMCPP_HIP_FULL_STEP                1: one launch per ensemble step for small ensembles (1)
    long full_step_max_walkers;   // MCMCPP_HIP_FULL_STEP_MAX_WALKERS    largest ensemble stepped that way (-1: 32768; 32767 where the matrix-core
                                  //                                     half-step kernel is the alternative)
    long task_table_mb;           // MCMCPP_HIP_TASK_TABLE_MB            size limit of the one-entry-per-draw jump table (16)
    long chain_subchunk_mb;       // MCMCPP_HIP_CHAIN_SUBCHUNK_MB        device chain staging per sub-chunk / ring budget (32)
    long graph_steps;             // MCMCPP_HIP_GRAPH_STEPS              ensemble steps per hipGraph replay (-1 here: 300 up to 32768 walkers, else 128)
    long trickle;                 // MCMCPP_HIP_TRICKLE                  1: stored steps forwarded to pinned memory by the launches (1)
    long no_draw_wave;            // MCMCPP_HIP_NO_DRAW_WAVE             1: no extra draw wavefronts (0)
    long batch_draws;             // MCMCPP_HIP_BATCH_DRAWS              ensemble steps whose draw records one launch makes ahead of the matrix-core full-step launches; 0: the launches make them themselves; -1: as many as a graph replays (-1)
    long pinned_direct;           // MCMCPP_HIP_PINNED_DIRECT            1: stored steps forwarded straight into a pinned chain_out (1)
    long comm_full_step;          // MCMCPP_HIP_COMM_FULL_STEP           split ensembles: 1 = one exchange per ensemble step (1), 0 = one per half-step
    long comm_compact;            // MCMCPP_HIP_COMM_COMPACT             split ensembles of more than one rank: 1 = exchange only the rows that moved (1), 0 = all-gather the slices
    long comm_compact_cap;        // MCMCPP_HIP_COMM_COMPACT_CAP         slots of an exchange block (0: learned from the run; a bound that is too small costs
                                  //                                     a repeated chunk, never a wrong chain)
    long comm_compact_chunk;      // MCMCPP_HIP_COMM_COMPACT_CHUNK       ensemble steps between two looks at the overflow flag (256)
    std::optional<long> de_scan_run;  // MCMCPP_HIP_DE_SCAN_RUN          differential evolution: stream positions one scanning lane steps through (kDeScanRun)
    std::optional<long> de_batch;     // MCMCPP_HIP_DE_BATCH             differential evolution: half-steps planned together (kDeBatchMax)
    static Knobs from_environment()
    {
        Knobs k;
        k.passes = env_long("MCMCPP_HIP_PASSES", 0);
        k.waves_per_simd = env_long("MCMCPP_HIP_WAVES_PER_SIMD", 2);
        k.matrix_core_min_walkers = env_long("MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS", 0);
        k.matrix_core_4pass = env_long("MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS");
        k.matrix_core_late = env_long("MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS", 49152);
        k.full_step = env_long("MCMCPP_HIP_FULL_STEP", 1);
        k.full_step_max_walkers = env_long("MCMCPP_HIP_FULL_STEP_MAX_WALKERS", -1);
        k.task_table_mb = env_long("MCMCPP_HIP_TASK_TABLE_MB", 16);
        k.chain_subchunk_mb = env_long("MCMCPP_HIP_CHAIN_SUBCHUNK_MB", 32);
        k.graph_steps = env_long("MCMCPP_HIP_GRAPH_STEPS", -1);
        k.trickle = env_long("MCMCPP_HIP_TRICKLE", 1);
        k.no_draw_wave = env_long("MCMCPP_HIP_NO_DRAW_WAVE", 0);
        k.batch_draws = env_long("MCMCPP_HIP_BATCH_DRAWS", -1);
        k.pinned_direct = env_long("MCMCPP_HIP_PINNED_DIRECT", 1);
        k.comm_full_step = env_long("MCMCPP_HIP_COMM_FULL_STEP", 1);
        k.comm_compact = env_long("MCMCPP_HIP_COMM_COMPACT", 1);
        k.comm_compact_cap = env_long("MCMCPP_HIP_COMM_COMPACT_CAP", 0);
        k.comm_compact_chunk = env_long("MCMCPP_HIP_COMM_COMPACT_CHUNK", 256);
        if (k.comm_compact_chunk < 1) k.comm_compact_chunk = 1;
        k.de_scan_run = env_long("MCMCPP_HIP_DE_SCAN_RUN");
        k.de_batch = env_long("MCMCPP_HIP_DE_BATCH");
        return k;
    }
};

// launch table (LaunchTable<double> / LaunchTable<float>) of a built-in or registered calculator, or nullptr
const void* launch_table_lookup(int dtype, int calc_id);
// Mover::DifferentialEvolution (diffevo.hip) and StretchMove with a batched log-posterior callback (batch.hip): see make_handle
mcmcpp_hip_sampler* make_de_sampler(const mcmcpp_hip_config& cfg, int* rc);
mcmcpp_hip_sampler* make_batch_sampler(const mcmcpp_hip_config& cfg, int* rc);
}  // namespace mcmcpp
