/*
 * Device/GaussianBridge.h -- the log-evidence of a sampled target from the chain of an ordinary run: a Gaussian fitted to the first
 * half of the stored steps behind the burn-in (Analysis::CovarianceMatrix, Utility/Cholesky.h), bridged with the second half
 * (mcmcpp_hip_evidence_gaussian, include/mcmcpp_hip.h).  A device chain (MCMCPP_CHAIN_MEMORY=device) is read where it lies.  What
 * EnsembleSampler, ParallelEnsembleSampler and, per rung, ReplicaExchangeSampler call.  Not part of the reference's API.
 */
#ifndef MCMCPP_DEVICE_GAUSSIANBRIDGE_H
#define MCMCPP_DEVICE_GAUSSIANBRIDGE_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../Analysis/CovarianceMatrix.h"
#include "../Analysis/Detail/DeviceSpan.h"
#include "../Chain/Chain.h"
#include "../Utility/Cholesky.h"
#include "HipBackend.h"

namespace MCMC
{
/// What gaussianBridgeEvidence returns: the estimate of log Z with its standard error, the bridge's diagnostics
/// (mcmcpp_hip_evidence_gaussian: index 0 of ess and nonfinite is the Gaussian's proposals, 1 the chain's draws), and the Gaussian.
struct GaussianBridgeEvidence
{
    double logEvidence, mcse, overlap, ess[2];
    std::int64_t passes, converged, nonfinite[2], numDraws;
    std::vector<double> mean;  ///< [numParams]
    std::vector<double> chol;  ///< [numParams][numParams], lower
};

namespace Device
{
/// Every sliceInterval'th stored step of `chain` behind the first burnIn: the first half of them fits the Gaussian, the second
/// half is bridged against as many proposals from pcg64(seed, 0), with the parameters of the handle's chain `chainIndex`.
/// std::invalid_argument for bad arguments or fewer than four used steps in either half; std::runtime_error where the fitted
/// covariance has no Cholesky factor.
template <class ParamType>
GaussianBridgeEvidence gaussianBridgeEvidence(const HipHandle& handle, int chainIndex, Chain::Chain<ParamType>& chain, int numWalkers, int numParams, int burnIn,
                                              int sliceInterval, std::uint64_t seed)
{
    typedef Chain::ChainStepIterator<ParamType> StepItt;
    if (burnIn < 0 || sliceInterval < 1) throw std::invalid_argument("gaussianBridgeEvidence: burnIn >= 0 and sliceInterval >= 1");
    const std::int64_t stored = chain.getStoredStepCount(), behind = stored - burnIn;
    const std::int64_t used = behind < 1 ? 0 : (behind + sliceInterval - 1) / sliceInterval, fitUsed = used / 2;
    if (fitUsed < 4) throw std::invalid_argument("gaussianBridgeEvidence: " + std::to_string(used) + " used steps; each half needs four");
    const StepItt start(&chain, burnIn), middle(&chain, burnIn + fitUsed * sliceInterval), end(&chain, stored);

    GaussianBridgeEvidence r = GaussianBridgeEvidence();
    const std::size_t D = static_cast<std::size_t>(numParams);
    {
        Analysis::CovarianceMatrix<ParamType> fit(numParams, numWalkers);
        fit.calculateCovar(start, middle, sliceInterval);
        std::vector<double> cov(D * D);
        r.mean.resize(D);
        for (std::size_t i = 0; i < D; ++i)
        {
            r.mean[i] = static_cast<double>(fit.getMean(static_cast<int>(i)));
            for (std::size_t j = 0; j < D; ++j) cov[i * D + j] = static_cast<double>(fit.getCovarianceMatrixElement(static_cast<int>(i), static_cast<int>(j)));
        }
        if (!Utility::choleskyLower(cov, numParams, r.chol))
            throw std::runtime_error("gaussianBridgeEvidence: the covariance of the fitted half is not positive definite");
    }

    Analysis::Detail::DeviceSpan<ParamType> span;
    if (Analysis::Detail::deviceSpan(middle, end, &span))  // a device chain: the second half is read in place
    {
        handle.check("mcmcpp_hip_evidence_gaussian_device",
                     mcmcpp_hip_evidence_gaussian_device(handle.get(), chainIndex, span.first, span.steps, sliceInterval, r.mean.data(), r.chol.data(), seed, 0,
                                                         &r.logEvidence, &r.mcse, &r.overlap, r.ess, &r.passes, &r.converged, r.nonfinite, &r.numDraws, nullptr, nullptr));
        return r;
    }
    std::vector<ParamType> staging;  // (a device chain with the device path switched off: the selected steps, downloaded)
    std::vector<const void*> steps;
    if (!Analysis::Detail::pointersStay(middle))
    {
        const std::int64_t n = Analysis::Detail::downloadSteps(middle, end, sliceInterval, staging);
        const std::size_t cells = static_cast<std::size_t>(numWalkers) * D;
        for (std::int64_t s = 0; s < n; ++s) steps.push_back(staging.data() + static_cast<std::size_t>(s) * cells);
    }
    else
        for (StepItt itt(middle); itt != end; itt += sliceInterval) steps.push_back(*itt);
    handle.check("mcmcpp_hip_evidence_gaussian",
                 mcmcpp_hip_evidence_gaussian(handle.get(), chainIndex, steps.data(), static_cast<std::int64_t>(steps.size()), 1, r.mean.data(), r.chol.data(), seed, 0,
                                              &r.logEvidence, &r.mcse, &r.overlap, r.ess, &r.passes, &r.converged, r.nonfinite, &r.numDraws, nullptr, nullptr));
    return r;
}
}  // namespace Device
}  // namespace MCMC
#endif  // MCMCPP_DEVICE_GAUSSIANBRIDGE_H
