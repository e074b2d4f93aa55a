// Example, device side: a batch log-posterior (see examples/batch_calculator.cpp for the host side).
//
// A batch target is evaluated by the caller for a whole half-step of proposals at once (MCMCPP_HIP_CALC_BATCH,
// include/mcmcpp_hip.h): the library forms the W/2 proposals in device memory, calls the Calculator's
// hipBatchLogPostProb, and accepts.  This file is that evaluation for the isotropic Gaussian, one thread per walker, in
// the operation order of the library's host twin (Device/Calculators.h, IsoGaussian): squares, the canonical pairwise
// tree sum over +0 padding to a power of two, times -1/2 -- so the chains equal the built-in target's bit for bit.
// Nothing here depends on the library's kernel headers: any HIP code (or a BLAS call, or a network) would do.
//
//   hipcc -std=c++17 -O3 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fPIC -shared \
//         examples/batch_calculator_device.hip -o libbatch_calculator.so
#include <hip/hip_runtime.h>

__global__ void iso_gaussian_batch_kernel(const double* __restrict__ x, double* __restrict__ out, long long count, int dims)
{
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= count) return;
    const double* r = x + (size_t)w * dims;
    int p2 = 1, top = 0;
    while (p2 < dims)
    {
        p2 <<= 1;
        ++top;
    }
    // the pairwise tree sum as a binary counter of partial sums: the left operand is always the lower-index half
    double partial[12];
    for (int i = 0; i < p2; ++i)
    {
        double v = i < dims ? r[i] * r[i] : 0.0;
        int lvl = 0;
        while ((i >> lvl) & 1)
        {
            v = partial[lvl] + v;
            ++lvl;
        }
        partial[lvl] = v;
    }
    out[w] = -0.5 * partial[top];
}

// the hipBatchLogPostProb of examples/batch_calculator.cpp: enqueue on the library's stream and return
extern "C" int iso_gaussian_batch_logp(const double* dProposals, long long count, int numParams, double* dLogp, void* hipStream)
{
    const unsigned block = 256, grid = (unsigned)((count + block - 1) / block);
    hipLaunchKernelGGL(iso_gaussian_batch_kernel, dim3(grid), dim3(block), 0, (hipStream_t)hipStream, dProposals, dLogp, count, numParams);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
