// batch_calc.hip -- batch log-posterior callbacks for tests/test_batch_calc.py (mcmcpp_hip_set_batch_calculator).
//
// Kind 4 is a target with a bounded support (params = {half_width, outside}): IsoGaussian's value where every
// |x_j| <= half_width, `outside` verbatim elsewhere; it counts the rows it found outside (batch_calc_outside).
//
// The four built-in Calculators restated one thread per walker, in the operation order of their host twins
// (include/MCMCpp/Device/Calculators.h): element terms combined by the canonical pairwise tree sum over +0 padding to a
// power of two, every product and sum rounded on its own (built with -ffp-contract=off), fma exactly where the twin
// writes std::fma (DenseGaussian's row dot product).  A batch target that computes these bits must reproduce the
// fused path's chains -- and the reference's fixtures -- bit for bit.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cmath>
#include <cstring>
#include <new>

namespace
{
enum Kind { kIso = 0, kDense = 1, kRosenbrock = 2, kSkewed = 3, kBoxedIso = 4 };

struct Ctx
{
    int kind, dtype, dims;
    void* d_params;         // device copy of the parameters (dense: P row-major as the twin reads it)
    int64_t calls;          // callbacks so far
    int64_t fail_at;        // >= 0: the call with this index returns fail_code
    int fail_code;
    unsigned long long* d_outside;  // device counter: rows the boxed target found outside its box
};

// Pairwise tree sum of term(0) .. term(P2-1) (term(j) = +0 for j >= dims) without an array: a binary counter of partial
// sums, left operand always the older (lower-index) half -- the recursion of Detail::treeSum, bottom-up.
template <class T, class Term>
__device__ T tree_sum(int dims, Term term)
{
    int p2 = 1;
    while (p2 < dims) p2 <<= 1;
    T stack[12];
    for (int i = 0; i < p2; ++i)
    {
        T v = i < dims ? term(i) : (T)0;
        int lvl = 0;
        while ((i >> lvl) & 1)
        {
            v = stack[lvl] + v;
            ++lvl;
        }
        stack[lvl] = v;
    }
    int top = 0;
    while ((1 << top) < p2) ++top;
    return stack[top];
}

template <class T>
__global__ void batch_logp_kernel(int kind, const T* __restrict__ x, T* __restrict__ out, long long count, int dims, const T* __restrict__ prm,
                                  unsigned long long* outside)
{
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= count) return;
    const T* r = x + (size_t)w * dims;
    T lp;
    if (kind == kIso)
    {
        const T s = tree_sum<T>(dims, [&](int j) { return r[j] * r[j]; });
        lp = (T)(-0.5) * s;
    }
    else if (kind == kDense)
    {
        const T s = tree_sum<T>(dims, [&](int i) {
            T acc = (T)0;
            const T* row = prm + (size_t)i * dims;
            for (int j = 0; j < dims; ++j) acc = fma(row[j], r[j], acc);
            return r[i] * acc;
        });
        lp = (T)(-0.5) * s;
    }
    else if (kind == kRosenbrock)
    {
        const T s = tree_sum<T>(dims, [&](int i) {
            if (i + 1 >= dims) return (T)0;
            const T sq = r[i] * r[i];
            const T u = r[i + 1] - sq;
            const T v = prm[0] - r[i];
            const T uu = u * u;
            const T buu = prm[1] * uu;
            const T vv = v * v;
            return buu + vv;
        });
        const T scaled = s * prm[2];
        lp = -scaled;
    }
    else if (kind == kBoxedIso)
    {
        bool inside = true;
        for (int j = 0; j < dims; ++j)
            if (!(r[j] <= prm[0] && r[j] >= -prm[0])) inside = false;  // (a NaN coordinate is outside)
        if (inside)
        {
            const T s = tree_sum<T>(dims, [&](int j) { return r[j] * r[j]; });
            lp = (T)(-0.5) * s;
        }
        else
        {
            lp = prm[1];
            atomicAdd(outside, 1ULL);
        }
    }
    else
    {
        const T half = r[0] / (T)2;
        const T lo = half - r[1];
        const T hi = half + r[1];
        const T a = (lo * lo) / prm[0];
        const T b = hi * hi;
        lp = (a + b) / (T)(-2);
    }
    out[w] = lp;
}
}  // namespace

extern "C"
{
// kind: 0 IsoGaussian, 1 DenseGaussian (P[D*D] row-major), 2 Rosenbrock (a, b, c), 3 SkewedGaussian2D (eps),
//       4 boxed IsoGaussian (half_width, outside)
void* batch_calc_create(int kind, int dtype, int dims, const void* params, int n_params)
{
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return nullptr;
    c->kind = kind;
    c->dtype = dtype;
    c->dims = dims;
    c->d_params = nullptr;
    c->calls = 0;
    c->fail_at = -1;
    c->fail_code = 0;
    const size_t bytes = (size_t)(n_params > 0 ? n_params : 1) * (dtype == 0 ? 8 : 4);
    if (hipMalloc(&c->d_params, bytes) != hipSuccess)
    {
        delete c;
        return nullptr;
    }
    if (n_params > 0 && hipMemcpy(c->d_params, params, bytes, hipMemcpyHostToDevice) != hipSuccess)
    {
        (void)hipFree(c->d_params);
        delete c;
        return nullptr;
    }
    c->d_outside = nullptr;
    if (hipMalloc(&c->d_outside, sizeof(unsigned long long)) != hipSuccess || hipMemset(c->d_outside, 0, sizeof(unsigned long long)) != hipSuccess)
    {
        (void)hipFree(c->d_outside);
        (void)hipFree(c->d_params);
        delete c;
        return nullptr;
    }
    return c;
}

void batch_calc_destroy(void* user)
{
    Ctx* c = static_cast<Ctx*>(user);
    if (!c) return;
    (void)hipFree(c->d_params);
    (void)hipFree(c->d_outside);
    delete c;
}

// rows the boxed target found outside its box so far (synchronises the device); -1 on error
int64_t batch_calc_outside(void* user)
{
    Ctx* c = static_cast<Ctx*>(user);
    unsigned long long v = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, c->d_outside, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

// the call with index `call` (counted from now) returns `code` instead of evaluating anything
void batch_calc_fail_at(void* user, int64_t call, int code)
{
    Ctx* c = static_cast<Ctx*>(user);
    c->calls = 0;
    c->fail_at = call;
    c->fail_code = code;
}

int64_t batch_calc_calls(void* user) { return static_cast<Ctx*>(user)->calls; }

// mcmcpp_hip_batch_logp_fn
int batch_calc_logp(void* user, const void* proposals, void* logp_out, int64_t count, int32_t num_params, void* hip_stream)
{
    Ctx* c = static_cast<Ctx*>(user);
    const int64_t call = c->calls++;
    if (call == c->fail_at) return c->fail_code;
    if (num_params != c->dims) return -1;
    const unsigned block = 256, grid = (unsigned)((count + block - 1) / block);
    if (c->dtype == 0)
        hipLaunchKernelGGL(batch_logp_kernel<double>, dim3(grid), dim3(block), 0, (hipStream_t)hip_stream, c->kind, (const double*)proposals,
                           (double*)logp_out, (long long)count, (int)num_params, (const double*)c->d_params, c->d_outside);
    else
        hipLaunchKernelGGL(batch_logp_kernel<float>, dim3(grid), dim3(block), 0, (hipStream_t)hip_stream, c->kind, (const float*)proposals,
                           (float*)logp_out, (long long)count, (int)num_params, (const float*)c->d_params, c->d_outside);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
}
