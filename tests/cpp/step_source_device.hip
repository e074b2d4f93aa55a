// step_source_device.hip -- mcmcpp::StepSource<T> and the device range check of mcmcpp_amd/csrc/analysis_host.hpp on a device,
// alone: no kernel, no analysis family.  A program of its own (tests/test_step_source.py builds it with the flags of
// mcmcpp_amd/csrc/Makefile and runs it as a child process): every span for_each_chunk yields is copied back and compared with the
// steps it must hold.  Prints a line per case; exit code 0 if all of them hold, 1 if one does not, 2 if a HIP call failed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "analysis_host.hpp"

using namespace mcmcpp;

namespace
{
constexpr int W = 3, P = 2, kSteps = 7, kElems = W * P;
constexpr long long kPers[] = {1, 2, 3, 7, 9};
int g_failed = 0;

#define MUST(expr)                                                                            \
    do                                                                                        \
    {                                                                                         \
        const hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                                 \
        {                                                                                     \
            std::printf("HIP %s: %s\n", #expr, hipGetErrorString(e_));                        \
            std::exit(2);                                                                     \
        }                                                                                     \
    } while (0)

void report(bool ok, const std::string& what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what.c_str());
    if (!ok) ++g_failed;
}

// element e of step k in generation g of the data: exact in float, different for every (g, k, e)
template <class T>
T value(int g, long long k, int e)
{
    return (T)(1000 * g + 10 * k + e + 1);
}

// where step k lies, in steps from the start of the arena (the four layouts of tests/test_step_chunks.py)
const int kSlot[4][kSteps] = {
    {0, 1, 2, 3, 4, 5, 6},     // contiguous
    {0, 2, 4, 6, 8, 10, 12},   // scattered
    {0, 1, 3, 5, 6, 7, 9},     // runs of 2, 1, 3, 1
    {6, 5, 4, 3, 2, 1, 0},     // descending
};
const char* const kLayout[4] = {"contiguous", "scattered", "runs_2_1_3_1", "descending"};

template <class T>
void fill(std::vector<T>& arena, const int* slot, int g)
{
    for (int k = 0; k < kSteps; ++k)
        for (int e = 0; e < kElems; ++e) arena[(size_t)slot[k] * kElems + e] = value<T>(g, k, e);
}

// One pass over the source: every span copied back and compared with generation `g` of steps first + k * every; also the
// chunks' sizes and their number.  Returns whether everything held.
template <class T>
bool pass_holds(StepSource<T>& src, long long per, int g, long long every, const T* lo, const T* hi)
{
    bool ok = true;
    long long seen = 0, chunks = 0;
    const int rc = src.for_each_chunk(per, [&](const StepSpan<T>& sp) -> int {
        const long long want = src.used - seen < per ? src.used - seen : per;
        ++chunks;
        if (sp.n_steps != want || sp.base < lo || sp.base + (sp.n_steps - 1) * sp.step_stride + kElems > hi) return ok = false, 7;  // (nothing is read outside [lo, hi))
        std::vector<T> got((size_t)sp.n_steps * kElems);
        for (long long j = 0; j < sp.n_steps; ++j)
            MUST(hipMemcpyAsync(&got[(size_t)j * kElems], sp.base + j * sp.step_stride, sizeof(T) * kElems, hipMemcpyDeviceToHost, src.stream));
        MUST(hipStreamSynchronize(src.stream));
        for (long long j = 0; j < sp.n_steps; ++j)
            for (int e = 0; e < kElems; ++e) ok = ok && got[(size_t)j * kElems + e] == value<T>(g, (seen + j) * every, e);
        seen += sp.n_steps;
        return 0;
    });
    return ok && rc == 0 && seen == src.used && chunks == (src.used + per - 1) / per;
}

template <class T>
void host_sources(hipStream_t stream, const char* type)
{
    std::string error;
    for (int l = 0; l < 4; ++l)
        for (const long long per : kPers)
        {
            std::vector<T> arena((size_t)13 * kElems, (T)-1);
            fill(arena, kSlot[l], 1);
            const void* ptrs[kSteps];
            for (int k = 0; k < kSteps; ++k) ptrs[k] = &arena[(size_t)kSlot[l][k] * kElems];
            DeviceBuffer<> chunk;
            StepSource<T> src{ptrs, nullptr, kSteps, 1, W, P, stream, &chunk, &error};
            const size_t bytes = src.upload_bytes(per);
            bool ok = bytes == sizeof(T) * kElems * (size_t)(per < kSteps ? per : kSteps);
            MUST(grow(chunk, bytes, stream));
            const T* lo = (const T*)chunk.get();
            ok = ok && pass_holds(src, per, 1, 1, lo, lo + bytes / sizeof(T));
            // the resident rule by its effect: new values in host memory reach a second pass only if it uploads again
            fill(arena, kSlot[l], 2);
            ok = ok && pass_holds(src, per, per >= kSteps ? 1 : 2, 1, lo, lo + bytes / sizeof(T));
            MUST(hipStreamSynchronize(stream));
            report(ok, std::string(type) + " host " + kLayout[l] + " per=" + std::to_string(per));
        }
}

template <class T>
void device_sources(hipStream_t stream, const char* type)
{
    std::string error;
    // the chain starts one step into its allocation
    std::vector<T> host((size_t)(kSteps + 1) * kElems, (T)-1);
    for (int k = 0; k < kSteps; ++k)
        for (int e = 0; e < kElems; ++e) host[(size_t)(k + 1) * kElems + e] = value<T>(1, k, e);
    DeviceBuffer<T> chain;
    MUST(chain.alloc(sizeof(T) * host.size()));
    MUST(hipMemcpy(chain, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice));
    const T* first = chain.get() + kElems;
    for (long long slice = 1; slice <= 3; ++slice)
        for (const long long per : kPers)
        {
            const long long used = (kSteps + slice - 1) / slice;
            DeviceBuffer<> chunk;  // (stays empty: a device chain is read where it lies)
            StepSource<T> src{nullptr, first, used, slice, W, P, stream, &chunk, &error};
            bool ok = src.upload_bytes(per) == 0;
            long long k0 = 0;
            ok = ok && 0 == src.for_each_chunk(per, [&](const StepSpan<T>& sp) -> int {  // the spans are the chain itself
                ok = ok && sp.base == first + k0 * slice * kElems && sp.step_stride == slice * kElems;
                k0 += sp.n_steps;
                return 0;
            });
            ok = ok && pass_holds(src, per, 1, slice, first, first + (size_t)kSteps * kElems) && pass_holds(src, per, 1, slice, first, first + (size_t)kSteps * kElems);
            report(ok && !chunk, std::string(type) + " device slice=" + std::to_string(slice) + " (" + std::to_string(used) + " steps) per=" + std::to_string(per));
        }
}

template <class T>
void empty_and_failing_sources(hipStream_t stream, const char* type)
{
    std::string error;
    DeviceBuffer<> chunk;
    int calls = 0;
    const auto count = [&](const StepSpan<T>&) { return ++calls, 0; };
    StepSource<T> none{nullptr, nullptr, 0, 1, W, P, stream, &chunk, &error};
    bool ok = none.upload_bytes(3) == 0 && none.for_each_chunk(3, count) == 0 && none.for_each_chunk(3, count) == 0;
    DeviceBuffer<T> chain;
    MUST(chain.alloc(sizeof(T) * kElems));
    StepSource<T> none_device{nullptr, chain.get(), 0, 2, W, P, stream, &chunk, &error};
    ok = ok && none_device.for_each_chunk(3, count) == 0 && calls == 0 && error.empty();
    report(ok, std::string(type) + " used == 0: f is never called, the result is OK");
    // f's failure ends the walk and is what for_each_chunk returns
    std::vector<T> arena((size_t)kSteps * kElems, (T)0);
    const void* ptrs[kSteps];
    for (int k = 0; k < kSteps; ++k) ptrs[k] = &arena[(size_t)k * kElems];
    StepSource<T> src{ptrs, nullptr, kSteps, 1, W, P, stream, &chunk, &error};
    MUST(grow(chunk, src.upload_bytes(2), stream));
    calls = 0;
    ok = src.for_each_chunk(2, [&](const StepSpan<T>&) { return ++calls == 2 ? 5 : 0; }) == 5 && calls == 2;
    MUST(hipStreamSynchronize(stream));
    report(ok, std::string(type) + " the first failure of f ends the walk");
}

void range_probe(int device)
{
    const size_t size = 65536, offset = 1024;
    DeviceBuffer<char> block;
    MUST(block.alloc(size));
    // what the runtime says about the allocation, asked here and not through the code under test
    hipDeviceptr_t base = nullptr;
    size_t reported = 0;
    MUST(hipMemGetAddressRange(&base, &reported, block.get()));
    report(base == (hipDeviceptr_t)block.get() && reported >= size, "the runtime knows the allocation: " + std::to_string(reported) + " bytes for " + std::to_string(size) + " asked for");
    const char* p = block.get() + offset;
    const size_t room = (size_t)((const char*)base + reported - p);
    std::string slot = "untouched";
    const DeviceRange r = probe_device_range(p, device);
    report(r.kind == DeviceRange::Found && r.device == device && r.room == room, "probe: the room behind a pointer into the middle of an allocation");
    report(check_device_steps(slot, "probe", p, room, device) == MCMCPP_HIP_OK && slot == "untouched", "exactly enough room is enough");
    report(check_device_steps(slot, "probe", p, room + 1, device) == MCMCPP_HIP_E_ARG && slot == "probe: n_steps steps do not end inside the allocation around device_steps",
           "one byte more is refused: " + slot);
    report(probe_device_range(p, device + 1).kind == DeviceRange::OtherDevice && check_device_steps(slot, "probe", p, 1, device + 1) == MCMCPP_HIP_E_ARG &&
               slot == "probe: device_steps is memory of device " + std::to_string(device) + ", not of device " + std::to_string(device + 1),
           "memory of another device than the one asked about: " + slot);
    PinnedBuffer<char> pinned;
    MUST(pinned.alloc(4096));
    slot.clear();
    report(probe_device_range(pinned.get(), device).kind == DeviceRange::NotDevice && check_device_steps(slot, "probe", pinned.get(), 1, device) == MCMCPP_HIP_E_ARG &&
               slot == "probe: device_steps is not device memory",
           "pinned host memory: " + slot);
    std::vector<char> pageable(4096);
    slot.clear();
    report(probe_device_range(pageable.data(), device).kind == DeviceRange::NotDevice && check_device_steps(slot, "probe", pageable.data(), 1, device) == MCMCPP_HIP_E_ARG &&
               slot == "probe: device_steps is not device memory",
           "pageable host memory: " + slot);
    report(hipGetLastError() == hipSuccess, "a refused pointer leaves no error behind in the runtime");
}
}  // namespace

int main()
{
    int device = 0;
    MUST(hipSetDevice(device));
    {
        Stream stream;
        MUST(hipStreamCreateWithFlags(stream.replace(), hipStreamNonBlocking));
        host_sources<double>(stream, "f64");
        host_sources<float>(stream, "f32");
        device_sources<double>(stream, "f64");
        device_sources<float>(stream, "f32");
        empty_and_failing_sources<double>(stream, "f64");
        empty_and_failing_sources<float>(stream, "f32");
    }
    range_probe(device);
    std::printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
