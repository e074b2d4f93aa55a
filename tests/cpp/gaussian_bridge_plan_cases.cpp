// gaussian_bridge_plan_cases.cpp -- prints what mcmcpp_amd/csrc/gaussian_bridge_plan.hpp plans and computes for
// mcmcpp_hip_evidence_gaussian (tests/test_gaussian_bridge_plan.py).  Built with the host compiler against the header (and the
// headers it includes) alone: that it compiles without HIP is part of the test.  Doubles are printed as the 16 hex digits of
// their bits, floats as 8.
//   gaussian_bridge_plan_cases limits
//   gaussian_bridge_plan_cases shape D=.. N=..        rows of a block, bytes of LDS, blocks, jump entries, doubles of parameters
//   gaussian_bridge_plan_cases position j=.. D=.. d=..
//   gaussian_bridge_plan_cases p r=..                 p and 1 - p of the raw draw r
//   gaussian_bridge_plan_cases check file=.. D=..     the file holds mean [D], chol [D][D]: the fault and its entry
//   gaussian_bridge_plan_cases rows file=.. D=.. N=.. f32=0|1
//        the file holds mean [D], chol [D][D], then N D raw draws of 8 bytes: k; then per proposal its row and the log q of
//        the rounded row
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "gaussian_bridge_plan.hpp"

using namespace mcmcpp;

static std::vector<double> read_doubles(const std::string& path)
{
    std::vector<double> v;
    if (std::FILE* f = std::fopen(path.c_str(), "rb"))
    {
        double buf[1024];
        size_t got;
        while ((got = std::fread(buf, 8, 1024, f)) > 0) v.insert(v.end(), buf, buf + got);
        std::fclose(f);
    }
    return v;
}
static unsigned long long bits(double x)
{
    unsigned long long b;
    std::memcpy(&b, &x, 8);
    return b;
}
static unsigned bits(float x)
{
    unsigned b;
    std::memcpy(&b, &x, 4);
    return b;
}

template <class T>
static void print_rows(int D, long long N, const double* prm, const double* raw)
{
    const double k = gaussian_log_norm(D, prm);
    std::printf("%016llx\n", bits(k));
    std::vector<uint64_t> r((size_t)D);
    std::vector<T> x((size_t)D);
    for (long long j = 0; j < N; ++j)
    {
        std::memcpy(r.data(), raw + (size_t)j * D, 8 * (size_t)D);
        gaussian_row(D, prm, r.data(), x.data());
        for (int d = 0; d < D; ++d)
        {
            if constexpr (sizeof(T) == 8)
                std::printf("%016llx ", bits(x[(size_t)d]));
            else
                std::printf("%08x ", bits(x[(size_t)d]));
        }
        std::printf("%016llx\n", bits(gaussian_log_q(D, prm, k, x.data())));
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    std::map<std::string, std::string> a;
    for (int i = 2; i < argc; ++i)
    {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        a[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    auto get = [&](const char* key, long long fallback) { return a.count(key) ? std::atoll(a[key].c_str()) : fallback; };
    const int D = (int)get("D", 1);

    if (what == "limits")
    {
        std::printf("max_d=%d stage_bytes=%d diff_threads=%d half_log_2pi=%016llx\n", kGaussianMaxD, kGaussianStageBytes, kGaussianDiffThreads, bits(kGaussianHalfLog2Pi));
        return 0;
    }
    if (what == "shape")
    {
        const long long N = get("N", 1);
        const int rows = gaussian_rows_per_block(D);
        std::printf("rows=%d lds=%zu blocks=%lld fits=%d entries=%d params=%zu diff_blocks=%lld\n", rows, gaussian_lds_bytes(D, rows), gaussian_blocks(N, rows),
                    (int)gaussian_grid_fits(N, D), gaussian_jump_entries(N), gaussian_param_doubles(D), gaussian_diff_blocks(N));
        return 0;
    }
    if (what == "position")
    {
        std::printf("%llu\n", (unsigned long long)gaussian_position(get("j", 0), D, (int)get("d", 0)));
        return 0;
    }
    if (what == "p")
    {
        const double p = gaussian_p(std::strtoull(a["r"].c_str(), nullptr, 10));
        std::printf("%016llx %016llx\n", bits(p), bits(1.0 - p));
        return 0;
    }
    const std::vector<double> v = read_doubles(a["file"]);
    if (what == "check")
    {
        int i = 0, d = 0;
        const int fault = (int)gaussian_check(D, v.data(), v.data() + D, &i, &d);
        std::printf("%d %d %d\n", fault, i, d);
        return 0;
    }
    if (what == "rows")
    {
        std::vector<double> prm(gaussian_param_doubles(D));
        gaussian_pack(D, v.data(), v.data() + D, prm.data());
        const double* raw = v.data() + D + (size_t)D * D;
        if (get("f32", 0))
            print_rows<float>(D, get("N", 0), prm.data(), raw);
        else
            print_rows<double>(D, get("N", 0), prm.data(), raw);
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
