// Cases for mcmcpp_amd/csrc/step_chunks.hpp, built with the host compiler alone (tests/test_step_chunks.py): prints what the
// header computes, the test judges it.
//   walk used per              -> a line "k0 now" per chunk
//   runs step_bytes end a0 a1 ... -> the chunk [0, end) of a pointer list with these addresses: a line "k run" per copy
//   strided stride end step_bytes -> the same for the flat form base + k * stride * step_bytes
//   knob NAME default_mb       -> chunk_bytes_from_env(NAME, default_mb)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "step_chunks.hpp"

template <class SrcOf>
static void print_runs(SrcOf&& src_of, long long n, size_t step_bytes)
{
    for (long long k = 0; k < n;)
    {
        const long long run = mcmcpp::contiguous_run(src_of, k, n, step_bytes);
        std::printf("%lld %lld\n", k, run);
        if (run < 1) return;
        k += run;
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const auto num = [&](int i) { return i < argc ? std::atoll(argv[i]) : 0; };
    if (!std::strcmp(argv[1], "walk"))
        return mcmcpp::for_each_step_chunk(num(2), num(3), [](long long k0, long long now) {
            std::printf("%lld %lld\n", k0, now);
            return 0;
        });
    if (!std::strcmp(argv[1], "runs"))
    {
        std::vector<const void*> steps;
        for (int i = 4; i < argc; ++i) steps.push_back(reinterpret_cast<const void*>(static_cast<size_t>(num(i))));
        if (num(3) > (long long)steps.size()) return 2;
        print_runs([&](long long k) { return steps[(size_t)k]; }, num(3), (size_t)num(2));
        return 0;
    }
    if (!std::strcmp(argv[1], "strided"))
    {
        const long long stride = num(2);
        const size_t step_bytes = (size_t)num(4);
        const char* base = reinterpret_cast<const char*>(static_cast<size_t>(4096));
        print_runs([&](long long k) { return base + step_bytes * (size_t)(k * stride); }, num(3), step_bytes);
        return 0;
    }
    if (!std::strcmp(argv[1], "knob") && argc == 4)
    {
        std::printf("%zu\n", mcmcpp::chunk_bytes_from_env(argv[2], (size_t)num(3)));
        return 0;
    }
    return 2;
}
