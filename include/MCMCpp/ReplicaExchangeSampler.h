/*
 * ReplicaExchangeSampler.h -- parallel tempering on one MI355X (an extension of this repository; the reference has none).
 *
 * K ensembles ("rungs") run on a ladder of targets, one Calculator per rung: rung 0 has the target of interest, the others
 * flattened versions of it (Device::DenseGaussian with beta_k P, Device::Rosenbrock with beta_k c, a plug-in with beta in its
 * parameter blob).  All rungs are the chains of ONE handle, stepped by the same launches with the stretch move
 * (GwDistribution<ParamType, 2, 1>); after every `exchangeEvery` ensemble steps a replica-exchange round proposes to swap
 * walker w of rung k with walker w of rung k + 1 (mcmcpp_hip_exchange_chains, include/mcmcpp_hip.h: the rule, the random
 * stream and the numbering of rounds; mcmcpp_hip_run_tempered puts the rounds into the run).  Rung k steps with seed randSeed + k, as a sampler of its own would.
 *
 * One host Chain per rung: the existing Analysis classes accept rung 0's chain (getStepIttBegin(0) / getStepIttEnd(0)) like
 * any other.  Device-memory chains are not offered here.
 *
 * evidenceRatios() estimates the ratios of normalising constants between neighbouring rungs from the stored steps
 * (mcmcpp_hip_evidence_ratios): their chain is the evidence of rung 0 when the top rung is a normalised density.
 * evidenceBridge() gives the bridge estimate of the same ratios, one per pair from the draws of both rungs
 * (mcmcpp_hip_evidence_bridge).  evidenceMbar() solves for all rungs' log-normalising constants at once from every draw of
 * every rung, with their covariance (mcmcpp_hip_evidence_mbar).
 */
#ifndef MCMCPP_REPLICAEXCHANGESAMPLER_H
#define MCMCPP_REPLICAEXCHANGESAMPLER_H

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Chain/Chain.h"
#include "Device/Calculators.h"
#include "Device/GaussianBridge.h"
#include "Device/HipBackend.h"
#include "Utility/UserOjbectsTest.h"

namespace MCMC
{

/// What ReplicaExchangeSampler::evidenceRatios returns (mcmcpp_hip_evidence_ratios, include/mcmcpp_hip.h): every vector is
/// [2][numRungs - 1], direction-major -- at(d, p): d = 0 the stepping-stone direction (draws of the flatter rung p + 1), d = 1 the
/// reverse; both estimate log(Z_p / Z_{p+1}).
struct EvidenceRatios
{
    int numPairs;
    std::int64_t numDraws;  ///< draws per rung: used steps times walkers
    std::vector<double> logRatio, mcse, ess, kish, maxU;
    std::vector<std::int64_t> nonfinite;
    double logRatioTotal[2], mcseTotal[2];  ///< log(Z_0 / Z_{numRungs-1}) by each direction, and its standard error
    std::size_t at(int direction, int pair) const { return static_cast<std::size_t>(direction) * static_cast<std::size_t>(numPairs) + static_cast<std::size_t>(pair); }
};

/// What ReplicaExchangeSampler::evidenceBridge returns (mcmcpp_hip_evidence_bridge, include/mcmcpp_hip.h): the bridge estimate
/// (Bennett's acceptance ratio) of log(Z_p / Z_{p+1}) per pair p, from the draws of both rungs.  ess and nonfinite are
/// [2][numRungs - 1], direction-major -- at(d, p): d = 0 the draws of rung p + 1, d = 1 those of rung p.
struct EvidenceBridge
{
    int numPairs;
    std::int64_t numDraws;  ///< draws per rung: used steps times walkers
    std::vector<double> logRatio, mcse, overlap;  ///< [numRungs - 1]; overlap: 1 for identical rungs, towards 0 for disjoint ones
    std::vector<std::int64_t> passes, converged;  ///< [numRungs - 1]: the solver's passes, and whether it stopped on its rule
    std::vector<double> ess;
    std::vector<std::int64_t> nonfinite;
    double logRatioTotal, mcseTotal;  ///< log(Z_0 / Z_{numRungs-1}) and its standard error
    std::size_t at(int direction, int pair) const { return static_cast<std::size_t>(direction) * static_cast<std::size_t>(numPairs) + static_cast<std::size_t>(pair); }
};

/// What ReplicaExchangeSampler::evidenceMbar returns (mcmcpp_hip_evidence_mbar, include/mcmcpp_hip.h): the multistate Bennett
/// acceptance ratio, one joint solve from every draw of every rung.  logZ [numRungs]: log(Z_k / Z_{numRungs-1}); cov
/// [numRungs][numRungs], row-major: the covariance of logZ, from which the error of any difference follows.
struct EvidenceMbar
{
    int numRungs;
    std::int64_t numDraws;  ///< draws per rung: used steps times walkers
    std::vector<double> logZ, cov;
    std::vector<double> logRatio, mcse;  ///< [numRungs - 1]: log(Z_p / Z_{p+1}) and its standard error from cov
    std::vector<double> ess;             ///< [numRungs]
    std::vector<std::int64_t> nonfinite;  ///< [numRungs][numRungs]: at(r, k) counts the draws of rung r that are not finite under rung k
    double logRatioTotal, mcseTotal;      ///< log(Z_0 / Z_{numRungs-1}) and its standard error
    std::int64_t passes, converged;       ///< the solver's passes, and whether it stopped on its rule
    std::size_t at(int row, int column) const { return static_cast<std::size_t>(row) * static_cast<std::size_t>(numRungs) + static_cast<std::size_t>(column); }
};

template <class ParamType, class Calculator>
class ReplicaExchangeSampler
{
public:
    typedef Chain::Chain<ParamType> ChainType;
    typedef Chain::ChainStepIterator<ParamType> StepItt;

    static_assert(Utility::CheckDeviceCalculator<Calculator>::value && !Utility::CheckBatchCalculator<Calculator, ParamType>::value,
                  "ReplicaExchangeSampler: the Calculator names a device functor: 'static const int hipCalcId', 'const ParamType* hipParams() const' "
                  "and 'int hipParamCount() const' (Device/Calculators.h); batch targets cannot be exchanged");

    /// One Calculator per rung, rung 0 first (2 to 16 rungs, all naming the same device functor with the same number of
    /// parameters: std::invalid_argument otherwise).  numWalker must be even and exceed 2*numParameter; maxChainSizeBytes
    /// bounds the host memory of each rung's stored steps.
    ReplicaExchangeSampler(int randSeed, int numWalker, int numParameter, const std::vector<Calculator>& rungCalculators,
                           unsigned long long maxChainSizeBytes = 2147483648ULL)
        : calcs(rungCalculators), numWalkers(numWalker), numParams(numParameter), numRungs(static_cast<int>(rungCalculators.size())), nextRound(0),
          placed(rungCalculators.size(), false), uploaded(false)
    {
        checkRungs(calcs);
        const std::size_t K = static_cast<std::size_t>(numRungs);
        for (std::size_t k = 0; k < K; ++k) chains.push_back(std::unique_ptr<ChainType>(new ChainType(numWalkers, numParams, maxChainSizeBytes)));
        initPos.resize(K * static_cast<std::size_t>(numWalkers) * numParams);
        initAux.resize(K * static_cast<std::size_t>(numWalkers));
        swapProposed.assign(K - 1, 0);
        swapAccepted.assign(K - 1, 0);
        mcmcpp_hip_config cfg = mcmcpp_hip_config();
        cfg.struct_size = sizeof(cfg);
        cfg.dtype = Device::HipDtype<ParamType>::value;
        cfg.num_walkers = numWalkers;
        cfg.num_params = numParams;
        cfg.calc_id = Calculator::hipCalcId;
        cfg.calc_params = calcs[0].hipParams();
        cfg.calc_params_len = calcs[0].hipParamCount();
        cfg.seed = static_cast<std::uint64_t>(static_cast<long long>(randSeed));
        cfg.stream = 0;
        cfg.gw_alpha_num = 2;
        cfg.gw_alpha_den = 1;
        cfg.mover = MCMCPP_HIP_MOVER_STRETCH;
        cfg.device = Device::Placement::fromEnvironment().device(0);
        cfg.num_chains = numRungs;
        handle.create(cfg);
        if (cfg.calc_params_len > 0)
            for (int k = 1; k < numRungs; ++k)
                handle.check("mcmcpp_hip_set_chain_params",
                             mcmcpp_hip_set_chain_params(handle.get(), k, calcs[static_cast<std::size_t>(k)].hipParams(), cfg.calc_params_len));
    }
    ReplicaExchangeSampler(const ReplicaExchangeSampler&) = delete;
    ReplicaExchangeSampler& operator=(const ReplicaExchangeSampler&) = delete;

    /// What the constructor checks before it touches the device.
    static void checkRungs(const std::vector<Calculator>& rungs)
    {
        if (rungs.size() < 2 || rungs.size() > 16)
            throw std::invalid_argument("ReplicaExchangeSampler: a ladder has 2 to 16 rungs, got " + std::to_string(rungs.size()));
        for (std::size_t k = 1; k < rungs.size(); ++k)
            if (static_cast<int>(rungs[k].hipCalcId) != static_cast<int>(rungs[0].hipCalcId) || rungs[k].hipParamCount() != rungs[0].hipParamCount())
                throw std::invalid_argument("ReplicaExchangeSampler: the calculators of all rungs must name the same device functor with the same number of parameters: rung " +
                                            std::to_string(k) + " has id " + std::to_string(static_cast<int>(rungs[k].hipCalcId)) + " with " +
                                            std::to_string(rungs[k].hipParamCount()) + " parameters, rung 0 id " + std::to_string(static_cast<int>(rungs[0].hipCalcId)) +
                                            " with " + std::to_string(rungs[0].hipParamCount()));
    }

    int getNumRungs() const { return numRungs; }

    /// positions: numWalker*numParameter values, walker-major; auxValues: the log-posterior of each walker under THIS rung's
    /// calculator.  The initial placement becomes step 0 of the rung's chain.  Every rung is placed before the first runMCMC.
    void setInitialWalkerPos(int rung, ParamType* positions, ParamType* auxValues)
    {
        const std::size_t k = checkedRung(rung), cells = static_cast<std::size_t>(numWalkers) * numParams;
        std::memcpy(&initPos[k * cells], positions, sizeof(ParamType) * cells);
        std::memcpy(&initAux[k * static_cast<std::size_t>(numWalkers)], auxValues, sizeof(ParamType) * static_cast<std::size_t>(numWalkers));
        for (int w = 0; w < numWalkers; ++w) chains[k]->storeWalker(w, positions + static_cast<std::size_t>(w) * numParams);
        chains[k]->incrementChainStep();
        placed[k] = true;
        uploaded = false;
    }

    /// numSteps more stored steps of every rung, with a replica-exchange round after every exchangeEvery of them (a tail shorter
    /// than exchangeEvery runs without a trailing exchange).  One mcmcpp_hip_run_tempered call: the rounds lie inside the run's
    /// launch sequence.  False when a chain's byte budget ran out first (the steps that fit are run and stored).  The call's
    /// stored steps of all rungs pass through one host staging vector on their way into the Chains.
    bool runMCMC(int numSteps, int exchangeEvery)
    {
        if (exchangeEvery < 1) throw std::invalid_argument("ReplicaExchangeSampler::runMCMC: exchangeEvery must be positive");
        upload();
        if (numSteps < 1) return true;
        const std::size_t K = static_cast<std::size_t>(numRungs), cells = static_cast<std::size_t>(numWalkers) * numParams;
        std::int64_t steps = numSteps;
        for (std::size_t k = 0; k < K; ++k)
            if (chains[k]->remainingSteps() < steps) steps = chains[k]->remainingSteps();
        if (steps < 1) return false;
        segment.resize(K * static_cast<std::size_t>(steps) * cells);
        std::uint64_t proposed[16] = {0}, accepted[16] = {0}, rounds = 0;
        handle.check("mcmcpp_hip_run_tempered",
                     mcmcpp_hip_run_tempered(handle.get(), steps, 1, exchangeEvery, nextRound, segment.data(), nullptr, proposed, accepted, nullptr, &rounds));
        for (std::size_t k = 0; k < K; ++k)
            for (std::int64_t s = 0; s < steps; ++s)
            {
                const ParamType* step = &segment[(k * static_cast<std::size_t>(steps) + static_cast<std::size_t>(s)) * cells];
                for (int w = 0; w < numWalkers; ++w) chains[k]->storeWalker(w, step + static_cast<std::size_t>(w) * numParams);
                chains[k]->incrementChainStep();
            }
        for (std::size_t p = 0; p + 1 < K; ++p)
        {
            swapProposed[p] += proposed[p];
            swapAccepted[p] += accepted[p];
        }
        nextRound += rounds;
        return steps == numSteps;
    }

    int getStoredSteps() { return static_cast<int>(chains[0]->getStoredStepCount()); }
    StepItt getStepIttBegin(int rung) { return chains[checkedRung(rung)]->getStepIteratorBegin(); }
    StepItt getStepIttEnd(int rung) { return chains[checkedRung(rung)]->getStepIteratorEnd(); }
    ChainType& chain(int rung) { return *chains[checkedRung(rung)]; }

    /// Accepted stretch proposals of the rung's walkers over its walkers times steps, the initial placement counted as one
    /// accepted step per walker (as EnsembleSampler::getAcceptanceFraction does).  Swaps are not counted here.
    ParamType getAcceptanceFraction(int rung)
    {
        const std::size_t k = checkedRung(rung);
        upload();
        std::vector<std::uint32_t> nacc(static_cast<std::size_t>(numRungs) * numWalkers);
        std::uint64_t steps = 0;
        handle.check("mcmcpp_hip_get_state", mcmcpp_hip_get_state(handle.get(), nullptr, nullptr, nacc.data()));
        handle.check("mcmcpp_hip_get_counters", mcmcpp_hip_get_counters(handle.get(), nullptr, &steps, nullptr, nullptr));
        unsigned long long acc = static_cast<unsigned long long>(numWalkers);
        for (int w = 0; w < numWalkers; ++w) acc += nacc[k * static_cast<std::size_t>(numWalkers) + static_cast<std::size_t>(w)];
        return static_cast<ParamType>(acc) / static_cast<ParamType>(static_cast<unsigned long long>(numWalkers) * (steps + 1ULL));
    }

    /// Accepted over proposed swaps between rung `pair` and rung `pair + 1` so far (0 before the first round that pairs them).
    ParamType getSwapFraction(int pair) const
    {
        if (pair < 0 || pair + 1 >= numRungs) throw std::out_of_range("ReplicaExchangeSampler::getSwapFraction: pair " + std::to_string(pair) + " out of range");
        const std::size_t p = static_cast<std::size_t>(pair);
        return swapProposed[p] ? static_cast<ParamType>(swapAccepted[p]) / static_cast<ParamType>(swapProposed[p]) : static_cast<ParamType>(0);
    }
    /// Rounds done so far; the next round has this number.
    std::uint64_t getExchangeRounds() const { return nextRound; }

    /// The ratios of normalising constants between neighbouring rungs, from every sliceInterval'th stored step of every rung
    /// behind the first burnIn (the initial placement is stored step 0), through the host-pointer entry.  At least four used
    /// steps; the walker state is not touched.
    EvidenceRatios evidenceRatios(int burnIn = 0, int sliceInterval = 1)
    {
        std::int64_t used = 0;
        const std::vector<const void*> steps = usedSteps("evidenceRatios", burnIn, sliceInterval, used);
        const std::size_t K = static_cast<std::size_t>(numRungs);
        EvidenceRatios r;
        r.numPairs = numRungs - 1;
        r.numDraws = 0;
        const std::size_t outs = 2 * (K - 1);
        r.logRatio.resize(outs), r.mcse.resize(outs), r.ess.resize(outs), r.kish.resize(outs), r.maxU.resize(outs), r.nonfinite.resize(outs);
        handle.check("mcmcpp_hip_evidence_ratios",
                     mcmcpp_hip_evidence_ratios(handle.get(), steps.empty() ? nullptr : steps.data(), used, 1, r.logRatio.data(), r.mcse.data(), r.ess.data(),
                                                r.kish.data(), r.maxU.data(), r.nonfinite.data(), r.logRatioTotal, r.mcseTotal, &r.numDraws));
        return r;
    }

    /// The bridge estimate of the same ratios (mcmcpp_hip_evidence_bridge): one per pair, from the draws of both rungs; the
    /// steps are chosen as for evidenceRatios.
    EvidenceBridge evidenceBridge(int burnIn = 0, int sliceInterval = 1)
    {
        std::int64_t used = 0;
        const std::vector<const void*> steps = usedSteps("evidenceBridge", burnIn, sliceInterval, used);
        const std::size_t pairs = static_cast<std::size_t>(numRungs - 1);
        EvidenceBridge r;
        r.numPairs = numRungs - 1;
        r.numDraws = 0;
        r.logRatioTotal = r.mcseTotal = 0.0;
        r.logRatio.resize(pairs), r.mcse.resize(pairs), r.overlap.resize(pairs), r.passes.resize(pairs), r.converged.resize(pairs);
        r.ess.resize(2 * pairs), r.nonfinite.resize(2 * pairs);
        handle.check("mcmcpp_hip_evidence_bridge",
                     mcmcpp_hip_evidence_bridge(handle.get(), steps.empty() ? nullptr : steps.data(), used, 1, r.logRatio.data(), r.mcse.data(), r.overlap.data(),
                                                r.ess.data(), r.passes.data(), r.converged.data(), r.nonfinite.data(), &r.logRatioTotal, &r.mcseTotal, &r.numDraws));
        return r;
    }

    /// All rungs' log-normalising constants in one joint solve from every draw of every rung, with their covariance
    /// (mcmcpp_hip_evidence_mbar); the steps are chosen as for evidenceRatios.
    EvidenceMbar evidenceMbar(int burnIn = 0, int sliceInterval = 1)
    {
        std::int64_t used = 0;
        const std::vector<const void*> steps = usedSteps("evidenceMbar", burnIn, sliceInterval, used);
        const std::size_t K = static_cast<std::size_t>(numRungs);
        EvidenceMbar r;
        r.numRungs = numRungs;
        r.numDraws = r.passes = r.converged = 0;
        r.logRatioTotal = r.mcseTotal = 0.0;
        r.logZ.resize(K), r.cov.resize(K * K), r.logRatio.resize(K - 1), r.mcse.resize(K - 1), r.ess.resize(K), r.nonfinite.resize(K * K);
        handle.check("mcmcpp_hip_evidence_mbar",
                     mcmcpp_hip_evidence_mbar(handle.get(), steps.empty() ? nullptr : steps.data(), used, 1, r.logZ.data(), r.cov.data(), r.logRatio.data(), r.mcse.data(),
                                              r.ess.data(), r.nonfinite.data(), &r.logRatioTotal, &r.mcseTotal, &r.passes, &r.converged, &r.numDraws));
        return r;
    }

    /// The log-evidence of ONE rung's target from that rung's chain alone (Device/GaussianBridge.h, mcmcpp_hip_evidence_gaussian):
    /// a Gaussian fitted to the first half of the rung's used steps, bridged with the second half.  Where the top rung is not a
    /// normalised density, this closes the chain of evidenceBridge's ratios.
    GaussianBridgeEvidence gaussianBridgeEvidence(int rung, int burnIn = 0, int sliceInterval = 1, std::uint64_t seed = 0)
    {
        const std::size_t k = checkedRung(rung);
        return Device::gaussianBridgeEvidence(handle, rung, *chains[k], numWalkers, numParams, burnIn, sliceInterval, seed);
    }

    /// Walker positions [K][W][D], log-posteriors [K][W] and per-walker accepted counts [K][W] as they stand on the device.
    void currentState(ParamType* positions, ParamType* logp, std::uint32_t* nAccept)
    {
        upload();
        handle.check("mcmcpp_hip_get_state", mcmcpp_hip_get_state(handle.get(), positions, logp, nAccept));
    }

private:
    /// every sliceInterval'th stored step of every rung behind the first burnIn, rung-major; used: their number per rung
    std::vector<const void*> usedSteps(const char* caller, int burnIn, int sliceInterval, std::int64_t& used)
    {
        const std::string who = std::string("ReplicaExchangeSampler::") + caller;
        if (burnIn < 0 || sliceInterval < 1) throw std::invalid_argument(who + ": burnIn >= 0 and sliceInterval >= 1");
        std::vector<const void*> steps;
        used = 0;
        for (std::size_t k = 0; k < static_cast<std::size_t>(numRungs); ++k)
        {
            StepItt itt = chains[k]->getStepIteratorBegin(), end = chains[k]->getStepIteratorEnd();
            std::int64_t index = 0, mine = 0;
            for (; itt != end; ++itt, ++index)
                if (index >= burnIn && (index - burnIn) % sliceInterval == 0)
                {
                    steps.push_back(*itt);
                    ++mine;
                }
            if (k > 0 && mine != used) throw std::logic_error(who + ": the rungs hold different numbers of steps");
            used = mine;
        }
        return steps;
    }

    std::size_t checkedRung(int rung) const
    {
        if (rung < 0 || rung >= numRungs) throw std::out_of_range("ReplicaExchangeSampler: rung " + std::to_string(rung) + " out of range");
        return static_cast<std::size_t>(rung);
    }
    void upload()
    {
        if (uploaded) return;
        for (std::size_t k = 0; k < placed.size(); ++k)
            if (!placed[k]) throw std::logic_error("ReplicaExchangeSampler: setInitialWalkerPos has not been called for rung " + std::to_string(k));
        handle.check("mcmcpp_hip_set_state", mcmcpp_hip_set_state(handle.get(), initPos.data(), initAux.data()));
        uploaded = true;
    }

    std::vector<Calculator> calcs;  // (the handle's create-time parameters point into calcs[0])
    int numWalkers, numParams, numRungs;
    std::uint64_t nextRound;
    std::vector<bool> placed;
    bool uploaded;
    std::vector<std::unique_ptr<ChainType> > chains;
    std::vector<ParamType> initPos, initAux, segment;
    std::vector<std::uint64_t> swapProposed, swapAccepted;
    Device::HipHandle handle;
};

}  // namespace MCMC
#endif  // MCMCPP_REPLICAEXCHANGESAMPLER_H
