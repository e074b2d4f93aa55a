// gaussian_bridge_plan.hpp -- the host's decisions of gaussian_bridge.hip (mcmcpp_hip_evidence_gaussian, include/mcmcpp_hip.h),
// and the arithmetic of a proposal's row and of log q as the kernels do it: the cap on D, the checks of the Gaussian, its
// parameters as the kernels read them, the stream position of a proposal's coordinate, p from a raw draw, the constant k, the
// launch shapes and the buffer sizes -- as pure functions of plain numbers.  No HIP header: this file compiles with the host
// compiler alone, and tests/test_gaussian_bridge_plan.py checks it there against the numpy restatement.  gaussian_bridge.hip
// turns a plan into launches and buffer sizes; it holds no threshold of its own.
//
// gaussian_row_core and gaussian_log_q_core are what a thread that owns a row runs, and what the host runs: one text, one order
// of operations.  They reach the row through an accessor z(d), which is a plain array on the host and a column of LDS on the
// device (element d of the block's thread t at [d][t]: the lanes of a wavefront read consecutive words).
#pragma once

#include <cfloat>
#include <cstddef>
#include <cstdint>

#include "normal_score.hpp"
#include "rhat_plan.hpp"

namespace mcmcpp
{
constexpr int kGaussianMaxD = 64;                  // the widest Gaussian: L takes D (D + 1) / 2 doubles of LDS beside the rows
constexpr int kGaussianStageBytes = 34 * 1024;     // LDS the rows of a block may take: (rows + 1) * D doubles
constexpr double kGaussianHalfLog2Pi = 0.91893853320467274178;

// The Gaussian as the kernels read it: mean [D], then the lower triangle of L row by row, L[i][d] at D + i (i + 1) / 2 + d
MCMCPP_NS_HD int gaussian_tri(int i, int d) { return i * (i + 1) / 2 + d; }
inline size_t gaussian_param_doubles(int D) { return (size_t)D + (size_t)D * (size_t)(D + 1) / 2; }
inline void gaussian_pack(int D, const double* mean, const double* chol, double* prm)
{
    for (int i = 0; i < D; ++i) prm[i] = mean[i];
    for (int i = 0; i < D; ++i)
        for (int d = 0; d <= i; ++d) prm[D + gaussian_tri(i, d)] = chol[(size_t)i * D + d];
}

// What is refused of a Gaussian, in the order it is looked for; *at_i, *at_d: the entry (the coordinate of the mean in *at_i)
enum GaussianFault
{
    kGaussianOk = 0,
    kGaussianTooWide,         // D > kGaussianMaxD
    kGaussianMeanNotFinite,   // mean[i]
    kGaussianFactorNotFinite, // chol[i][d], d <= i
    kGaussianDiagonal         // chol[i][i] is not a positive normal number
};
inline bool gaussian_finite(double x) { return x - x == 0.0; }
inline GaussianFault gaussian_check(int D, const double* mean, const double* chol, int* at_i, int* at_d)
{
    *at_i = 0, *at_d = 0;
    if (D > kGaussianMaxD) return kGaussianTooWide;
    for (int i = 0; i < D; ++i)
        if (!gaussian_finite(mean[i])) return *at_i = i, kGaussianMeanNotFinite;
    for (int i = 0; i < D; ++i)
        for (int d = 0; d <= i; ++d)
            if (!gaussian_finite(chol[(size_t)i * D + d])) return *at_i = i, *at_d = d, kGaussianFactorNotFinite;
    for (int i = 0; i < D; ++i)
        if (!(chol[(size_t)i * D + i] >= DBL_MIN)) return *at_i = i, *at_d = i, kGaussianDiagonal;
    return kGaussianOk;
}

// Coordinate d of proposal j takes the raw output at this position of the stream: a row's D outputs follow each other.  (The
// host makes the jump table's entry b from the position of row 2^b; a thread steps through d.)
MCMCPP_NS_HD uint64_t gaussian_position(long long j, int D, int d) { return (uint64_t)j * (uint64_t)D + (uint64_t)d; }
// p = ((r >> 12) + 0.5) 2^-52: 52 bits and a half, so both operations are exact, 0 < p < 1, and so is 1 - p
MCMCPP_NS_HD double gaussian_p(uint64_t r)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return ((double)(r >> 12) + 0.5) * 0x1p-52;
}

// z(d) holds the scores z_d on entry and x_i = mean_i + acc_i, still a double, on return: acc_i from +0, + L[i][d] z[d] for
// d = 0 .. i in ascending order.  (From the last row up: x_i takes the place of z_i, which no earlier row reads.)
template <class Z>
MCMCPP_NS_HD void gaussian_row_core(int D, const double* prm, Z&& z)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int i = D - 1; i >= 0; --i)
    {
        const double* row = prm + D + gaussian_tri(i, 0);
        double acc = 0.0;
        for (int d = 0; d <= i; ++d) acc = acc + row[d] * z(d);
        z(i) = prm[i] + acc;
    }
}
// z(i) holds x_i widened to double on entry and z_i = ((x_i - mean_i) - t_i) / L[i][i] on return; t_i from +0, + L[i][d] z[d] for
// d < i in ascending order; s from +0, + z_i z_i in ascending i; returns (-0.5 s) + k
template <class Z>
MCMCPP_NS_HD double gaussian_log_q_core(int D, const double* prm, double k, Z&& z)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int i = 0; i < D; ++i)
    {
        const double* row = prm + D + gaussian_tri(i, 0);
        double t = 0.0;
        for (int d = 0; d < i; ++d) t = t + row[d] * z(d);
        const double zi = ((z(i) - prm[i]) - t) / row[i];
        z(i) = zi;
        s = s + zi * zi;
    }
    return (-0.5 * s) + k;
}
// k = -(the sum from +0, in ascending i, of normal_score_log(L[i][i])) - D 0.91893853320467274178: formed once, on the host
inline double gaussian_log_norm(int D, const double* prm)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double sum = 0.0;
    for (int i = 0; i < D; ++i) sum = sum + normal_score_log(prm[D + gaussian_tri(i, i)]);
    return -sum - (double)D * kGaussianHalfLog2Pi;
}

// The host's row and log q, in the kernels' order: r [D] the raw outputs at gaussian_position(j, D, 0 .. D - 1)
struct GaussianHostColumn
{
    double* v;
    double& operator()(int d) const { return v[d]; }
};
template <class T>
void gaussian_row(int D, const double* prm, const uint64_t* r, T* x)
{
    double z[kGaussianMaxD];
    for (int d = 0; d < D; ++d) z[d] = normal_score(gaussian_p(r[d]));
    gaussian_row_core(D, prm, GaussianHostColumn{z});
    for (int d = 0; d < D; ++d) x[d] = (T)z[d];
}
template <class T>
double gaussian_log_q(int D, const double* prm, double k, const T* x)
{
    double z[kGaussianMaxD];
    for (int d = 0; d < D; ++d) z[d] = (double)x[d];
    return gaussian_log_q_core(D, prm, k, GaussianHostColumn{z});
}

// Both kernels: a thread owns a row, a block `rows` of them, staged through LDS as columns [D][rows + 1] of doubles (the odd
// stride keeps the transposed accesses of the coalesced loads and stores off one bank) behind the Gaussian's parameters.
inline int gaussian_rows_per_block(int D)
{
    for (int rows = 256; rows > 64; rows /= 2)
        if ((size_t)(rows + 1) * (size_t)D * 8 <= (size_t)kGaussianStageBytes) return rows;
    return 64;
}
inline size_t gaussian_lds_bytes(int D, int rows) { return 8 * (gaussian_param_doubles(D) + (size_t)(rows + 1) * (size_t)D); }
inline long long gaussian_blocks(long long count, int rows) { return (count + rows - 1) / rows; }
inline bool gaussian_grid_fits(long long count, int D) { return gaussian_blocks(count, gaussian_rows_per_block(D)) <= kRhatGridXMax; }
// The jump table of the generating kernel: entry b is the map of D 2^b steps of the stream; a thread reaches row j's position
// through the entries of j's set bits.  As many entries as N - 1 has bits, one at the least.
inline int gaussian_jump_entries(long long N)
{
    int bits = 1;
    while (bits < 63 && ((N - 1) >> bits) != 0) ++bits;
    return bits;
}
// The differences kernel: one thread a draw
constexpr int kGaussianDiffThreads = 256;
inline long long gaussian_diff_blocks(long long count) { return (count + kGaussianDiffThreads - 1) / kGaussianDiffThreads; }
}  // namespace mcmcpp
