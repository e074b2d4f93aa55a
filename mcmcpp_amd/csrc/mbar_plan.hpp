// mbar_plan.hpp -- the host's decisions of mbar.hip (mcmcpp_hip_evidence_mbar, include/mcmcpp_hip.h): how the sums of a pass are
// numbered and grouped, the shapes of sum_tree over all K N draws and over the N draws of a rung, the buffers and launch shapes,
// the Cholesky solve of the reduced system, the solver that turns passes into zeta, and the covariance -- as pure functions of
// plain numbers and of a callable that evaluates one pass.  No HIP header: this file compiles with the host compiler alone,
// and tests/test_mbar_plan.py checks it there, with a host pass in place of the kernels.  mbar.hip turns a plan into launches and
// buffer sizes; it holds no threshold of its own.
//
// The sums of a pass, Q = K + K (K + 1) / 2 of them: S_k at k; P_kl (k <= l) at K + k K - k (k - 1) / 2 + (l - k), row by row.
// Group k (the pass kernel's grid.y) forms S_k and row k of P: 1 + K - k sums, in batches of kMbarBatch through LDS.
// sum_tree is bridge_plan.hpp's, over K N terms (the joint tree) and, behind the final pass, over the N terms of each rung (a
// tree of its own that begins at the rung's first draw).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "bridge_plan.hpp"

namespace mcmcpp
{
constexpr int kMbarMaxChains = 16;                          // the rungs of a handle (step_layout.hpp's kMaxChains)
constexpr int kMbarBatch = 4;                               // sums a block reduces at a time
constexpr int kMbarSolverPasses = 200;                      // the solver's bound; the final pass comes on top
constexpr double kMbarStepCap = 4.0;                        // no component of a step exceeds it
constexpr double kMbarTolerance = 9.094947017729282e-13;    // 2^-40

inline int mbar_quantities(int K) { return K + K * (K + 1) / 2; }
MCMCPP_EE_HD int mbar_index_p(int K, int k, int l) { return K + k * K - k * (k - 1) / 2 + (l - k); }  // k <= l
MCMCPP_EE_HD int mbar_group_quantities(int K, int k) { return 1 + K - k; }

// The shape of sum_tree over `terms` terms
struct MbarTree
{
    long long terms = 0, tiles = 0;
    int slices = 0;
};
inline MbarTree mbar_tree(long long terms)
{
    const BridgePlan b = bridge_plan(terms);
    MbarTree t;
    t.terms = terms, t.tiles = b.tiles, t.slices = b.slices;
    return t;
}

// One call: the joint tree and a rung's; the pass kernel's grid is (tiles, K groups, sets) with sets = 1 over the joint tree
// and K over the rungs'; tile sums [set][Q][tiles], slice sums [set][Q][slices].  These two buffers serve both launches of the
// final pass in turn: K tiles of a rung's tree are no fewer than the joint tree's.  Totals: [Q] of the joint tree, then [K][Q] of
// the rungs'.
struct MbarPlan
{
    int K = 0, Q = 0;
    MbarTree joint, rung;
    size_t l_doubles = 0, series_doubles = 0, tile_sum_doubles = 0, slice_sum_doubles = 0, total_doubles = 0;
};
inline MbarPlan mbar_plan(int K, long long N)
{
    MbarPlan p;
    p.K = K, p.Q = mbar_quantities(K);
    p.joint = mbar_tree((long long)K * N), p.rung = mbar_tree(N);
    p.l_doubles = (size_t)K * (size_t)K * (size_t)N;
    p.series_doubles = (size_t)K * (size_t)N;
    p.tile_sum_doubles = (size_t)K * (size_t)p.Q * (size_t)p.rung.tiles;
    p.slice_sum_doubles = (size_t)K * (size_t)p.Q * (size_t)p.rung.slices;
    p.total_doubles = (size_t)(K + 1) * (size_t)p.Q;
    return p;
}
inline bool mbar_grid_fits(int K, long long N) { return bridge_grid_fits((long long)K * N); }
// the closing kernels: one thread per (set, sum, slice), then one per (set, sum)
inline unsigned mbar_close_blocks(long long items) { return (unsigned)((items + kBridgeThreads - 1) / kBridgeThreads); }

// The weights of one draw: l[k * stride] is the draw's log-posterior under chain k
inline void mbar_weights(int K, const double* l, size_t stride, const double* zeta, double* w)
{
    double a[kMbarMaxChains];
    for (int k = 0; k < K; ++k) a[k] = l[(size_t)k * stride] - zeta[k];
    double m = a[0];
    for (int k = 1; k < K; ++k)
        if (a[k] > m) m = a[k];
    if (m == -std::numeric_limits<double>::infinity())
    {
        for (int k = 0; k < K; ++k) w[k] = 0.0;
        return;
    }
    double dn = 0.0;
    for (int k = 0; k < K; ++k)
    {
        w[k] = evidence_exp(a[k] - m);
        dn = dn + w[k];
    }
    for (int k = 0; k < K; ++k) w[k] = w[k] / dn;
}

// The Q sums over terms [first, first + count) of l [K][total], on the host in the kernel's order; `series`, where it is not
// null, takes w_own of every term
inline void mbar_host_sums(int K, const double* l, size_t total, long long first, long long count, const double* zeta, double* q, double* series, int own)
{
    std::vector<double> w((size_t)K * (size_t)count), v((size_t)count);
    for (long long i = 0; i < count; ++i)
    {
        double one[kMbarMaxChains];
        mbar_weights(K, l + first + i, total, zeta, one);
        for (int k = 0; k < K; ++k) w[(size_t)k * (size_t)count + (size_t)i] = one[k];
        if (series) series[i] = one[own];
    }
    for (int k = 0; k < K; ++k)
    {
        q[k] = bridge_sum_tree(w.data() + (size_t)k * (size_t)count, count);
        for (int l2 = k; l2 < K; ++l2)
        {
            for (long long i = 0; i < count; ++i) v[(size_t)i] = w[(size_t)k * (size_t)count + (size_t)i] * w[(size_t)l2 * (size_t)count + (size_t)i];
            q[mbar_index_p(K, k, l2)] = bridge_sum_tree(v.data(), count);
        }
    }
}

// The reduced system of order M = K - 1 from the sums of a pass: A_kk = S_k - P_kk, A_kl = -P_kl; G_k = S_k - N
inline void mbar_system(int K, long long N, const double* q, double* A, double* G)
{
    const int M = K - 1;
    const double Nd = (double)N;
    for (int k = 0; k < M; ++k)
    {
        for (int l = 0; l < M; ++l) A[k * M + l] = k == l ? q[k] - q[mbar_index_p(K, k, k)] : -q[mbar_index_p(K, k < l ? k : l, k < l ? l : k)];
        G[k] = q[k] - Nd;
    }
}
// A = L L^T in the header's order; false where a pivot is not positive
inline bool mbar_factor(int M, const double* A, double* L)
{
    for (int i = 0; i < M; ++i)
    {
        for (int j = 0; j < i; ++j)
        {
            double t = A[i * M + j];
            for (int k = 0; k < j; ++k) t = t - L[i * M + k] * L[j * M + k];
            L[i * M + j] = t / L[j * M + j];
        }
        double d = A[i * M + i];
        for (int k = 0; k < i; ++k) d = d - L[i * M + k] * L[i * M + k];
        if (!(d > 0.0)) return false;
        L[i * M + i] = std::sqrt(d);
    }
    return true;
}
// x = A^-1 b through the factor: forward, then backward (b and x may be the same array)
inline void mbar_substitute(int M, const double* L, const double* b, double* x)
{
    double y[kMbarMaxChains];
    for (int i = 0; i < M; ++i)
    {
        double t = b[i];
        for (int k = 0; k < i; ++k) t = t - L[i * M + k] * y[k];
        y[i] = t / L[i * M + i];
    }
    for (int i = M - 1; i >= 0; --i)
    {
        double t = y[i];
        for (int k = i + 1; k < M; ++k) t = t - L[k * M + i] * x[k];
        x[i] = t / L[i * M + i];
    }
}

// The sums of a pass: joint [Q]; behind the final pass rung [K][Q] too
struct MbarSums
{
    std::vector<double> joint, rung;
};
struct MbarRoot
{
    std::vector<double> zeta;  // [K]
    long long passes = 0;
    int converged = 0;
    bool failed = false;  // a factor failed: no mass is shared
    MbarSums at;          // the final pass's sums, at zeta
    std::vector<double> L;  // the factor behind the final pass, [K - 1][K - 1]
};

// The solver of the header.  eval(zeta, final, &sums) is one pass and returns 0, or a code that ends the solve.
template <class Eval>
int mbar_solve(int K, long long N, Eval&& eval, MbarRoot* out)
{
    const int M = K - 1;
    MbarRoot r;
    r.zeta.assign((size_t)K, 0.0);
    r.L.assign((size_t)M * (size_t)M, 0.0);
    std::vector<double> A((size_t)M * (size_t)M), G((size_t)M), delta((size_t)M);
    MbarSums s;
    for (int it = 0; it < kMbarSolverPasses && !r.converged; ++it)
    {
        if (int rc = eval(r.zeta.data(), false, &s)) return rc;
        ++r.passes;
        mbar_system(K, N, s.joint.data(), A.data(), G.data());
        if (!mbar_factor(M, A.data(), r.L.data()))
        {
            r.failed = true, r.converged = 1;
            *out = r;
            return 0;
        }
        mbar_substitute(M, r.L.data(), G.data(), delta.data());
        const auto largest = [&](const std::vector<double>& v, int count) {
            double mx = 0.0;
            for (int k = 0; k < count; ++k)
            {
                const double size = v[(size_t)k] < 0.0 ? -v[(size_t)k] : v[(size_t)k];
                if (size > mx) mx = size;
            }
            return mx;
        };
        double mx = largest(delta, M);
        if (mx > kMbarStepCap)
        {
            const double scale = kMbarStepCap / mx;
            for (int k = 0; k < M; ++k) delta[(size_t)k] = delta[(size_t)k] * scale;
            mx = largest(delta, M);
        }
        for (int k = 0; k < M; ++k) r.zeta[(size_t)k] = r.zeta[(size_t)k] + delta[(size_t)k];
        const double size = largest(r.zeta, M);
        if (mx <= kMbarTolerance * (size > 1.0 ? size : 1.0)) r.converged = 1;
    }
    if (int rc = eval(r.zeta.data(), true, &r.at)) return rc;
    ++r.passes;
    mbar_system(K, N, r.at.joint.data(), A.data(), G.data());
    if (!mbar_factor(M, A.data(), r.L.data())) r.failed = true, r.converged = 1;
    *out = r;
    return 0;
}

// cov [K][K] behind the final pass: V from the rungs' sums [K][Q] and ess [K], then the sandwich through the factor
inline void mbar_covariance(int K, long long N, const double* L, const double* rung, const double* ess, double* cov)
{
    const int M = K - 1, Q = mbar_quantities(K);
    const double Nd = (double)N;
    std::vector<double> V((size_t)M * (size_t)M, 0.0), Y((size_t)M * (size_t)M), col((size_t)M), x((size_t)M);
    for (int r = 0; r < K; ++r)
    {
        const double* q = rung + (size_t)r * (size_t)Q;
        const double f = (Nd * Nd) / ess[r];
        for (int k = 0; k < M; ++k)
            for (int l = k; l < M; ++l)
            {
                const double c = q[mbar_index_p(K, k, l)] / Nd - (q[k] / Nd) * (q[l] / Nd);
                const double term = c == 0.0 ? 0.0 : f * c;
                V[(size_t)(k * M + l)] = V[(size_t)(k * M + l)] + term;
            }
    }
    for (int k = 0; k < M; ++k)
        for (int l = 0; l < k; ++l) V[(size_t)(k * M + l)] = V[(size_t)(l * M + k)];
    for (int c = 0; c < M; ++c)
    {
        for (int k = 0; k < M; ++k) col[(size_t)k] = V[(size_t)(k * M + c)];
        mbar_substitute(M, L, col.data(), x.data());
        for (int k = 0; k < M; ++k) Y[(size_t)(k * M + c)] = x[(size_t)k];
    }
    for (int i = 0; i < K * K; ++i) cov[i] = 0.0;
    for (int c = 0; c < M; ++c)
    {
        mbar_substitute(M, L, Y.data() + (size_t)c * (size_t)M, x.data());
        for (int k = 0; k < M; ++k) cov[c * K + k] = x[(size_t)k];
    }
}

// log_ratio, mcse [K - 1] and the totals from zeta and cov
inline double mbar_root_of_variance(double v) { return v < 0.0 ? 0.0 : std::sqrt(v); }
inline void mbar_figures(int K, const double* zeta, const double* cov, double* log_ratio, double* mcse, double* log_ratio_total, double* mcse_total)
{
    for (int p = 0; p + 1 < K; ++p)
    {
        const int q = p + 1;
        log_ratio[p] = zeta[p] - zeta[q];
        mcse[p] = mbar_root_of_variance((cov[p * K + p] + cov[q * K + q]) - 2.0 * cov[p * K + q]);
    }
    *log_ratio_total = zeta[0];
    *mcse_total = mbar_root_of_variance(cov[0]);
}
}  // namespace mcmcpp
