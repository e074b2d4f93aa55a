// accept_log_device.hip -- the device builds of the accept test's arithmetic, callable from tests/test_accept_logs.py.
//
// Every kernel here calls the PRODUCTION function unchanged: dev_log and draw_store<T> from stretch_kernel.hpp, canonical
// from canonical.hpp (through pcg128.hpp), on a HalfStepArgs<T> filled by stretch_args<T> (sampler_host.hpp).  Built by
// the test with the flags of mcmcpp_amd/csrc/Makefile.  Host functions return 0 or the HIP error code; nothing aborts.
// The host side also offers glibc's log / logf over an array (the oracle's logarithms: NumPy's own are a different
// implementation) and the comparison of one binade of device logf results with glibc's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "sampler_host.hpp"

using namespace mcmcpp;

namespace
{

template <class T>
__global__ void log_kernel(const T* x, T* y, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = dev_log(x[i]);
}

// y[i] = dev_log(the float whose bits are first_bits + i)
__global__ void log_range_f32_kernel(uint32_t first_bits, unsigned n, float* y)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = dev_log(__uint_as_float(first_bits + i));
}

template <class T>
__global__ void canonical_kernel(const uint64_t* r, T* u, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[i] = canonical(r[i], T());
}

template <class T>
__global__ void draw_kernel(HalfStepArgs<T> a, int k, const uint64_t* r, DrawRec<T>* rec, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) draw_store<T>(a, k, r[i], rec + i);
}

struct DevBuf
{
    void* p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
};

#define TRY(x)                          \
    do                                  \
    {                                   \
        const hipError_t e_ = (x);      \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

const unsigned kBlock = 256;
const unsigned kMaxN = 1u << 26;  // elements per call: bounds every buffer and keeps the index arithmetic in 32 bits

inline unsigned blocks(unsigned n) { return (n + kBlock - 1) / kBlock; }

template <class T>
HalfStepArgs<T> args_of(int alpha_num, int alpha_den, int dims)
{
    mcmcpp_hip_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.num_walkers = 2 * dims + 2;
    cfg.num_params = dims;
    cfg.gw_alpha_num = alpha_num;
    cfg.gw_alpha_den = alpha_den;
    return stretch_args<T>(cfg, 0, make_u128(0, 1), Affine128());
}

template <class T>
int dev_log_array(const T* x, T* y, unsigned n)
{
    if (n == 0) return 0;
    if (!x || !y || n > kMaxN) return -1;
    DevBuf dx, dy;
    TRY(dx.alloc(sizeof(T) * n));
    TRY(dy.alloc(sizeof(T) * n));
    TRY(hipMemcpy(dx.p, x, sizeof(T) * n, hipMemcpyHostToDevice));
    log_kernel<T><<<blocks(n), kBlock>>>((const T*)dx.p, (T*)dy.p, n);
    TRY(hipGetLastError());
    TRY(hipMemcpy(y, dy.p, sizeof(T) * n, hipMemcpyDeviceToHost));
    return 0;
}

template <class T>
int dev_canonical_array(const uint64_t* r, T* u, unsigned n)
{
    if (n == 0) return 0;
    if (!r || !u || n > kMaxN) return -1;
    DevBuf dr, du;
    TRY(dr.alloc(8 * (size_t)n));
    TRY(du.alloc(sizeof(T) * n));
    TRY(hipMemcpy(dr.p, r, 8 * (size_t)n, hipMemcpyHostToDevice));
    canonical_kernel<T><<<blocks(n), kBlock>>>((const uint64_t*)dr.p, (T*)du.p, n);
    TRY(hipGetLastError());
    TRY(hipMemcpy(u, du.p, sizeof(T) * n, hipMemcpyDeviceToHost));
    return 0;
}

// draw_store<T> of task k (1: z and zs; 2: ln_u) on every r; fields the task does not write come back as 0
template <class T>
int dev_draw_array(int alpha_num, int alpha_den, int dims, int k, const uint64_t* r, unsigned n, T* z, T* zs, T* ln_u)
{
    if (n == 0) return 0;
    if (!r || !z || !zs || !ln_u || n > kMaxN || (k != 1 && k != 2) || dims < 1) return -1;
    const HalfStepArgs<T> a = args_of<T>(alpha_num, alpha_den, dims);
    DevBuf dr, drec;
    TRY(dr.alloc(8 * (size_t)n));
    TRY(drec.alloc(sizeof(DrawRec<T>) * n));
    TRY(hipMemcpy(dr.p, r, 8 * (size_t)n, hipMemcpyHostToDevice));
    TRY(hipMemset(drec.p, 0, sizeof(DrawRec<T>) * n));
    draw_kernel<T><<<blocks(n), kBlock>>>(a, k, (const uint64_t*)dr.p, (DrawRec<T>*)drec.p, n);
    TRY(hipGetLastError());
    std::vector<DrawRec<T>> rec(n);
    TRY(hipMemcpy(rec.data(), drec.p, sizeof(DrawRec<T>) * n, hipMemcpyDeviceToHost));
    for (unsigned i = 0; i < n; ++i)
    {
        z[i] = rec[i].z;
        zs[i] = rec[i].zs;
        ln_u[i] = rec[i].ln_u;
    }
    return 0;
}

// floats as integers in their numerical order
inline int64_t ordered(float v)
{
    int32_t b;
    memcpy(&b, &v, 4);
    return b < 0 ? (int64_t)INT32_MIN - b : b;
}

}  // namespace

extern "C"
{
// dtype 0: double, 1: float (as everywhere in the C API)
int ald_log_f64(const double* x, double* y, unsigned n) { return dev_log_array<double>(x, y, n); }
int ald_log_f32(const float* x, float* y, unsigned n) { return dev_log_array<float>(x, y, n); }
int ald_canonical_f64(const uint64_t* r, double* u, unsigned n) { return dev_canonical_array<double>(r, u, n); }
int ald_canonical_f32(const uint64_t* r, float* u, unsigned n) { return dev_canonical_array<float>(r, u, n); }
int ald_draw_f64(int an, int ad, int dims, int k, const uint64_t* r, unsigned n, double* z, double* zs, double* ln_u)
{
    return dev_draw_array<double>(an, ad, dims, k, r, n, z, zs, ln_u);
}
int ald_draw_f32(int an, int ad, int dims, int k, const uint64_t* r, unsigned n, float* z, float* zs, float* ln_u)
{
    return dev_draw_array<float>(an, ad, dims, k, r, n, z, zs, ln_u);
}

// dev_log(float) on the n floats whose bits are first_bits .. first_bits + n - 1
int ald_log_f32_range(uint32_t first_bits, unsigned n, float* y)
{
    if (n == 0) return 0;
    if (!y || n > kMaxN || (uint64_t)first_bits + n > 0x7F800000ull) return -1;  // positive finite floats only
    DevBuf dy;
    TRY(dy.alloc(4 * (size_t)n));
    log_range_f32_kernel<<<blocks(n), kBlock>>>(first_bits, n, (float*)dy.p);
    TRY(hipGetLastError());
    TRY(hipMemcpy(y, dy.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// Host only.  y[i] (a device result for the float with bits first_bits + i) against glibc's logf of the same float:
// the number of arguments on which they differ, their largest distance in ulp and the argument bits of the first such case.
void ald_compare_logf_range(uint32_t first_bits, unsigned n, const float* y, uint64_t* differ, uint32_t* max_dist, uint32_t* worst_bits)
{
    uint64_t nd = 0;
    int64_t md = 0;
    uint32_t wb = 0;
    for (unsigned i = 0; i < n; ++i)
    {
        float x;
        const uint32_t b = first_bits + i;
        memcpy(&x, &b, 4);
        const float want = logf(x);
        if (memcmp(&want, &y[i], 4) != 0)
        {
            nd += 1;
            int64_t d = ordered(want) - ordered(y[i]);
            if (d < 0) d = -d;
            if (!(y[i] == y[i])) d = INT32_MAX;  // NaN
            if (d > md) md = d, wb = b;
        }
    }
    *differ = nd;
    *max_dist = (uint32_t)(md > (int64_t)UINT32_MAX ? UINT32_MAX : md);
    *worst_bits = wb;
}

// Host only: glibc's log / logf, the oracle's logarithms
void ald_host_log_f64(const double* x, double* y, size_t n)
{
    for (size_t i = 0; i < n; ++i) y[i] = log(x[i]);
}
void ald_host_log_f32(const float* x, float* y, size_t n)
{
    for (size_t i = 0; i < n; ++i) y[i] = logf(x[i]);
}

// Host only: tie_eps as the library sets it.  mover 0: stretch_args<T> (stretch and batch samplers); 1: accept_tie_eps<T>(), the
// expression the differential-evolution sampler assigns (diffevo.hip)
double ald_tie_eps(int dtype, int mover)
{
    if (mover == 0) return dtype == 0 ? (double)args_of<double>(2, 1, 4).tie_eps : (double)args_of<float>(2, 1, 4).tie_eps;
    return dtype == 0 ? (double)accept_tie_eps<double>() : (double)accept_tie_eps<float>();
}

// Host only: the GwDistribution constants and (T)(D-1) of stretch_args<T>, for the test's restatement to be checked against
void ald_stretch_constants(int dtype, int an, int ad, int dims, double* gw_term1, double* gw_inv_sqrt, double* dims_minus_one)
{
    if (dtype == 0)
    {
        const HalfStepArgs<double> a = args_of<double>(an, ad, dims);
        *gw_term1 = a.gw_term1, *gw_inv_sqrt = a.gw_inv_sqrt, *dims_minus_one = a.dims_minus_one;
    }
    else
    {
        const HalfStepArgs<float> a = args_of<float>(an, ad, dims);
        *gw_term1 = a.gw_term1, *gw_inv_sqrt = a.gw_inv_sqrt, *dims_minus_one = a.dims_minus_one;
    }
}
}
