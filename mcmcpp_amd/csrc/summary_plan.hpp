// summary_plan.hpp -- what summary.hip decides on the host, as pure functions of plain numbers: the checks of probs and
// hdi_prob, the window of the highest-density interval and the blocks of its reduction, the ranks of a quantile's Monte Carlo
// standard error from the Beta quantile, and the host arithmetic of sd and the standard errors.  No HIP header: this file
// compiles with the host compiler alone, and tests/test_summary_plan.py checks it there.  summary.hip turns a plan into launches;
// it holds no threshold of its own.  No result depends on the spans: the order the reduction uses is total.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "beta_quantile.hpp"
#include "rank_plan.hpp"

namespace mcmcpp
{
constexpr int kSummaryMaxProbs = 16;
constexpr int kSummaryThreads = kRankThreads;                // threads of a block of every summary kernel
constexpr long long kSummaryHdiSpan = 8 * kSummaryThreads;   // window starts a block of the HDI reduction takes: 8 a thread
constexpr double kSummaryLowerTail = 0.15865525393145707;    // Phi(-1) and Phi(1): a standard error is half the width between them
constexpr double kSummaryUpperTail = 0.8413447460685429;

// "" or why the probabilities are refused
inline std::string summary_check_probs(const double* probs, int32_t n_probs)
{
    if (n_probs < 0 || n_probs > kSummaryMaxProbs) return "0 <= n_probs <= 16";
    if (n_probs > 0 && !probs) return "probs must not be NULL where n_probs > 0";
    for (int i = 0; i < n_probs; ++i)
        if (!(probs[i] > 0.0 && probs[i] < 1.0)) return "0 < prob < 1 for every prob (probs[" + std::to_string(i) + "] is not)";
    return "";
}

// the draws an interval of hdi_prob spans: m = floor(hdi_prob S), in double
inline long long summary_hdi_m(double hdi_prob, long long S) { return (long long)std::floor(hdi_prob * (double)S); }

// "" or why hdi_prob is refused for S draws (0: no interval is asked for)
inline std::string summary_check_hdi(double hdi_prob, long long S)
{
    if (hdi_prob == 0.0) return "";
    if (!(hdi_prob > 0.0 && hdi_prob < 1.0)) return "hdi_prob = 0 (no interval) or 0 < hdi_prob < 1";
    const long long m = summary_hdi_m(hdi_prob, S);
    if (m < 1 || m > S - 1) return "1 <= floor(hdi_prob S) <= S - 1 (it is " + std::to_string(m) + " of S = " + std::to_string(S) + " draws)";
    return "";
}

// the sorted keys of all parameters, kept where they do not fit one tile; MCMCPP_HIP_SUMMARY_KEEP_MB bounds them (read per
// call; default: no bound but the device's memory)
constexpr size_t kSummaryDefaultKeepMb = (size_t)1 << 24;  // 16 TiB
inline size_t summary_keep_bytes(long long S, int P, int key_bits) { return (size_t)S * (size_t)P * (size_t)(key_bits / 8); }
inline size_t summary_keep_limit_from_env() { return chunk_bytes_from_env("MCMCPP_HIP_SUMMARY_KEEP_MB", kSummaryDefaultKeepMb); }

// windows i = 0 .. S - m - 1: [x_(i), x_(i+m)]
inline long long summary_hdi_windows(long long S, long long m) { return S - m; }
RHAT_HD long long summary_hdi_blocks(long long windows) { return (windows + kSummaryHdiSpan - 1) / kSummaryHdiSpan; }
// block b of the reduction takes window starts [first, first + count)
RHAT_HD void summary_hdi_block_span(long long windows, long long b, long long* first, long long* count)
{
    *first = b * kSummaryHdiSpan;
    const long long left = windows - *first;
    *count = left < kSummaryHdiSpan ? (left < 0 ? 0 : left) : kSummaryHdiSpan;
}
inline bool summary_grids_fit(long long windows, int tile) { return summary_hdi_blocks(windows) <= kRankGridXMax && tile <= kRankGridYMax; }

// the pooled sample variance of S = M L draws from the sequences' within and between (times `over`: 1 / (S - 1) or 1 / S)
inline double summary_pooled(long long L, long long M, double within, double between, long long over)
{
    return ((double)((L - 1) * M) * within + (double)(L * (M - 1)) * between) / (double)over;
}

// The ranks between which a quantile's standard error is read: the order statistics at the 15.87 % and 84.13 % points of
// Beta(ess prob + 1, ess (1 - prob) + 1).  A NaN ess gives -1, -1.
struct SummaryMcseRanks
{
    long long lower, upper;
};
inline SummaryMcseRanks summary_mcse_ranks(double ess, double prob, long long S)
{
    if (ess != ess) return SummaryMcseRanks{-1, -1};
    const double a = ess * prob + 1.0, b = ess * (1.0 - prob) + 1.0;
    const double lo = std::floor(beta_quantile(kSummaryLowerTail, a, b) * (double)S), hi = std::ceil(beta_quantile(kSummaryUpperTail, a, b) * (double)S);
    SummaryMcseRanks r;
    r.lower = (long long)(lo > 1.0 ? lo : 1.0) - 1;
    r.upper = (long long)(hi < (double)S ? hi : (double)S) - 1;
    return r;
}
}  // namespace mcmcpp
