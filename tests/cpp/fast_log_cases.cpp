// fast_log_cases.cpp -- mcmcpp::fast_log (mcmcpp_amd/csrc/fast_log.hpp) against an exact logarithm, on the CPU.
//
// Built by tests/test_accept_logs.py with the host compiler alone against fast_log.hpp and canonical.hpp (no HIP header:
// that it compiles is an assertion), -ffp-contract=off like the library, linked with libquadmath.  The judge is logq on the
// exact double argument: 113 bits, so its own error is below 2^-60 ulp of a double.  glibc's log (the oracle's logarithm)
// is measured beside it, never used as the judge.
//
//   fast_log_cases check            one line per input family and a total:
//       family=NAME n=N worst_ulp=E worst_arg=HEX glibc_worst_ulp=E differ=N max_dist=N sign_bad=N
//     worst_ulp        max |fast_log(x) - log x| in ulp of the exact value
//     glibc_worst_ulp  the same for glibc's log
//     differ           inputs on which fast_log(x) != log(x) of glibc;  max_dist: their largest distance in ulp
//     sign_bad         inputs on which the sign of fast_log(x) is not the sign of x - 1 (0 only at x == 1)
//   fast_log_cases dump IN OUT      the same inputs as raw doubles to IN and the host build's fast_log of each to OUT
//
// Input families (the header's domain: z in [1/2, 2] and 1-u in [2^-53, 1]; the binades run on to 4, which alpha up to 4
// would reach):
//   sampler_a2_z, sampler_a2_1mu, sampler_a32_z, sampler_a32_1mu   z = (t1 u + t0)^2 and 1 - u with u = canonical(r, double())
//                      of kSampler seeded 64-bit values each, t1/t0 as stretch_args computes them for alpha = 2 and 3/2
//   below_one, above_one   1 - j 2^-53 and 1 + j 2^-52, j = 1 .. 10^6
//   sqrt2, sqrt_half   kBranch doubles each side of the branch constant of fast_log and of half of it, by nextafter
//   binades            2^e .. 2^(e+1), e = -53 .. 1: both ends and kMantissas random mantissas each
//   edges              2^-53, 1 - 2^-53, 1/2, 1, 2
#include <math.h>
#include <quadmath.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "canonical.hpp"
#include "fast_log.hpp"

namespace
{

const int kSampler = 3000000, kNearOne = 1000000, kBranch = 300000, kMantissas = 4096;

struct Family
{
    std::string name;
    std::vector<double> x;
};

uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

void sampler_families(std::vector<Family>& out, const char* tag, int num, int den, uint64_t seed)
{
    // GwDistribution constants as stretch_args (sampler_host.hpp) computes them, z as draw_store (stretch_kernel.hpp)
    const double alpha = (double)num / (double)den;
    const double sqrt_a = sqrt(alpha);
    const double inv_sqrt_a = 1.0 / sqrt_a;
    const double t1 = sqrt_a - inv_sqrt_a, t0 = inv_sqrt_a;
    Family fz, fu;
    fz.name = std::string("sampler_") + tag + "_z";
    fu.name = std::string("sampler_") + tag + "_1mu";
    uint64_t s = seed;
    for (int i = 0; i < kSampler; ++i)
    {
        const double u1 = mcmcpp::canonical(splitmix64(s), double());
        const double tmp = t1 * u1 + t0;
        fz.x.push_back(tmp * tmp);
        const double u2 = mcmcpp::canonical(splitmix64(s), double());
        fu.x.push_back(1.0 - u2);
    }
    out.push_back(fz);
    out.push_back(fu);
}

void around(Family& f, double centre, int each_side)
{
    f.x.push_back(centre);
    double lo = centre, hi = centre;
    for (int i = 0; i < each_side; ++i)
    {
        lo = nextafter(lo, 0.0);
        hi = nextafter(hi, 4.0);
        f.x.push_back(lo);
        f.x.push_back(hi);
    }
}

std::vector<Family> make_families()
{
    std::vector<Family> fams;
    sampler_families(fams, "a2", 2, 1, 0x1234567ULL);
    sampler_families(fams, "a32", 3, 2, 0x89ABCDEFULL);
    Family below, above, s2, sh, bin, edges;
    below.name = "below_one";
    above.name = "above_one";
    for (int j = 1; j <= kNearOne; ++j)
    {
        below.x.push_back(1.0 - (double)j * 0x1p-53);
        above.x.push_back(1.0 + (double)j * 0x1p-52);
    }
    s2.name = "sqrt2";
    around(s2, 1.41421356237309504880, kBranch);
    sh.name = "sqrt_half";
    around(sh, 0.5 * 1.41421356237309504880, kBranch);
    bin.name = "binades";
    uint64_t s = 0xB1AADE5ULL;
    for (int e = -53; e <= 1; ++e)
    {
        const double lo = ldexp(1.0, e);
        bin.x.push_back(lo);
        bin.x.push_back(nextafter(2.0 * lo, 0.0));
        for (int i = 0; i < kMantissas; ++i)
        {
            const uint64_t bits = ((uint64_t)(e + 1023) << 52) | (splitmix64(s) >> 12);
            double x;
            memcpy(&x, &bits, 8);
            bin.x.push_back(x);
        }
    }
    edges.name = "edges";
    const double e[] = {0x1p-53, 1.0 - 0x1p-53, 0.5, 1.0, 2.0};
    edges.x.assign(e, e + 5);
    fams.push_back(below);
    fams.push_back(above);
    fams.push_back(s2);
    fams.push_back(sh);
    fams.push_back(bin);
    fams.push_back(edges);
    return fams;
}

// |got - exact| in ulp of the exact value (a double's ulp at |exact|); exact == 0 asks for got == 0
double ulp_error(double got, __float128 exact)
{
    if (exact == 0) return got == 0.0 ? 0.0 : INFINITY;
    int e;
    frexpq(fabsq(exact), &e);  // |exact| = m 2^e, m in [1/2, 1): a double there has ulp 2^(e-53)
    return (double)(fabsq((__float128)got - exact) / ldexpq(1, e - 53));
}

// doubles as integers in their numerical order
int64_t ordered(double v)
{
    int64_t b;
    memcpy(&b, &v, 8);
    return b < 0 ? INT64_MIN - b : b;
}

struct Stats
{
    long long n = 0, differ = 0, sign_bad = 0, max_dist = 0;
    double worst = 0, worst_arg = 1, glibc_worst = 0;
    void merge(const Stats& o)
    {
        n += o.n;
        differ += o.differ;
        sign_bad += o.sign_bad;
        if (o.max_dist > max_dist) max_dist = o.max_dist;
        if (o.worst > worst) worst = o.worst, worst_arg = o.worst_arg;
        if (o.glibc_worst > glibc_worst) glibc_worst = o.glibc_worst;
    }
    void print(const char* name) const
    {
        printf("family=%s n=%lld worst_ulp=%.4f worst_arg=%a glibc_worst_ulp=%.4f differ=%lld max_dist=%lld sign_bad=%lld\n", name, n, worst,
               worst_arg, glibc_worst, differ, max_dist, sign_bad);
    }
};

Stats check(const std::vector<double>& xs)
{
    Stats total;
#pragma omp parallel
    {
        Stats st;
#pragma omp for schedule(static)
        for (long long i = 0; i < (long long)xs.size(); ++i)
        {
            const double x = xs[i];
            const double got = mcmcpp::fast_log(x), libm = log(x);
            const __float128 exact = logq((__float128)x);
            const double err = ulp_error(got, exact), gerr = ulp_error(libm, exact);
            st.n += 1;
            if (!(err <= st.worst)) st.worst = err, st.worst_arg = x;  // (a NaN error is the worst too)
            if (gerr > st.glibc_worst) st.glibc_worst = gerr;
            if (got != libm || signbit(got) != signbit(libm))
            {
                st.differ += 1;
                int64_t d = ordered(got) - ordered(libm);
                if (d < 0) d = -d;
                if (d > st.max_dist) st.max_dist = d;
            }
            const bool sign_ok = x > 1.0 ? got > 0.0 : (x < 1.0 ? got < 0.0 : (got == 0.0 && !signbit(got)));
            if (!sign_ok) st.sign_bad += 1;
        }
#pragma omp critical
        total.merge(st);
    }
    return total;
}

}  // namespace

int main(int argc, char** argv)
{
    const std::vector<Family> fams = make_families();
    if (argc == 2 && !strcmp(argv[1], "check"))
    {
        Stats total;
        for (const Family& f : fams)
        {
            const Stats st = check(f.x);
            st.print(f.name.c_str());
            total.merge(st);
        }
        total.print("total");
        const double one = mcmcpp::fast_log(1.0);
        uint64_t bits;
        memcpy(&bits, &one, 8);
        printf("fast_log_of_one_bits=0x%016llx\n", (unsigned long long)bits);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "dump"))
    {
        FILE* fi = fopen(argv[2], "wb");
        FILE* fo = fopen(argv[3], "wb");
        if (!fi || !fo) return 2;
        for (const Family& f : fams)
        {
            std::vector<double> y(f.x.size());
            for (size_t i = 0; i < f.x.size(); ++i) y[i] = mcmcpp::fast_log(f.x[i]);
            if (fwrite(f.x.data(), 8, f.x.size(), fi) != f.x.size() || fwrite(y.data(), 8, y.size(), fo) != y.size()) return 2;
        }
        return fclose(fi) | fclose(fo) ? 2 : 0;
    }
    fprintf(stderr, "usage: fast_log_cases check | dump IN OUT\n");
    return 1;
}
