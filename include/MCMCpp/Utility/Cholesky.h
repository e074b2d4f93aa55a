/*
 * Utility/Cholesky.h -- the lower Cholesky factor of a small symmetric matrix, on the host, in double: what the samplers'
 * gaussianBridgeEvidence needs between Analysis::CovarianceMatrix and mcmcpp_hip_evidence_gaussian.  Not part of the reference's
 * API.
 */
#ifndef MCMCPP_UTILITY_CHOLESKY_H
#define MCMCPP_UTILITY_CHOLESKY_H

#include <cmath>
#include <cstddef>
#include <vector>

namespace MCMC
{
namespace Utility
{
/// factor [n][n], row-major: L with L L^T = a (the lower triangle of `a` is read), zeros above the diagonal.  False, with
/// `factor` unspecified, when a pivot is not a positive finite number: the matrix is not positive definite to rounding.
inline bool choleskyLower(const std::vector<double>& a, int n, std::vector<double>& factor)
{
    const std::size_t N = static_cast<std::size_t>(n);
    factor.assign(N * N, 0.0);
    for (std::size_t i = 0; i < N; ++i)
        for (std::size_t j = 0; j <= i; ++j)
        {
            double sum = a[i * N + j];
            for (std::size_t k = 0; k < j; ++k) sum -= factor[i * N + k] * factor[j * N + k];
            if (i == j)
            {
                if (!(sum > 0.0) || !std::isfinite(sum)) return false;
                factor[i * N + i] = std::sqrt(sum);
            }
            else
                factor[i * N + j] = sum / factor[j * N + j];
        }
    return true;
}
}  // namespace Utility
}  // namespace MCMC
#endif  // MCMCPP_UTILITY_CHOLESKY_H
