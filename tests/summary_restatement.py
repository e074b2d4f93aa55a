"""The definition of mcmcpp_hip_posterior_summary (include/mcmcpp_hip.h) restated in numpy, for tests/test_summary.py: the draws
and the order statistics of tests/rank_restatement.py, the effective sample sizes of tests/ess_restatement.py on the draws, on
their squared deviations and on the indicator chains of the quantiles, and the host arithmetic of sd, the standard errors and
the highest-density interval, every operation a float64 operation rounded on its own.  The Beta quantile is the library's
(capi.beta_quantile), which tests/test_beta_quantile.py checks by itself; `beta` replaces it."""
import math

import numpy as np

from mcmcpp_amd import capi
from tests import ess_restatement as er
from tests import rank_restatement as rk

LOWER_TAIL, UPPER_TAIL = 0.15865525393145707, 0.8413447460685429


def pooled(L, M, within, between, over):
    return (np.float64((L - 1) * M) * within + np.float64(L * (M - 1)) * between) / np.float64(over)


def sorted_draws(x):
    """the draws x [(S,)] of one parameter as float64, in the total order of the keys (-0 below +0)"""
    return x[np.argsort(rk.to_key(x), kind="stable")].astype(np.float64)


def quantile_of(xs, prob):
    h, lo, hi = capi.quantile_ranks([prob], xs.size)
    with np.errstate(invalid="ignore"):
        return capi.quantile_rule(xs[lo][None], xs[hi][None], h, "linear", np.float64)[0, 0]


def mcse_ranks(ess, prob, S, beta=None):
    """(rank_lower, rank_upper) of the header; -1, -1 for a NaN ess"""
    if np.isnan(ess):
        return -1, -1
    beta = beta or capi.beta_quantile
    a, b = np.float64(ess) * np.float64(prob) + 1.0, np.float64(ess) * (1.0 - np.float64(prob)) + 1.0
    lo, hi = math.floor(np.float64(beta(LOWER_TAIL, a, b)) * np.float64(S)), math.ceil(np.float64(beta(UPPER_TAIL, a, b)) * np.float64(S))
    return max(lo, 1) - 1, min(hi, S) - 1


def hdi_of(xs, hdi_prob):
    """(lower, upper, i) of the narrowest window of m = floor(hdi_prob S) steps in the sorted draws; NaN, NaN, -1 where every
    width is NaN"""
    S = xs.size
    m = int(math.floor(np.float64(hdi_prob) * np.float64(S)))
    assert 1 <= m <= S - 1
    with np.errstate(invalid="ignore"):
        w = xs[m:] - xs[:S - m]
    if np.isnan(w).all():
        return np.nan, np.nan, -1
    i = int(np.flatnonzero(w == np.nanmin(w))[0])  # the first of equal minima (a NaN equals nothing; nanargmin would take one for +inf)
    return xs[i], xs[i + m], i


def posterior_summary(steps, probs=(0.05, 0.5, 0.95), hdi_prob=0.94, split=True, max_lag=0, slice_interval=1, beta=None):
    d = rk.draws(steps, split, slice_interval)
    K, HL, W, P = d.shape
    if np.isnan(d).any():
        raise ValueError("a NaN draw has no place in the order")
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    Q = probs.size
    ess = lambda chain: er.effective_sample_size(chain, split, max_lag)
    with np.errstate(all="ignore"):
        first = ess(d)
        L, M = first["sequence_length"], first["num_sequences"]
        S = L * M
        sd = np.sqrt(pooled(L, M, first["within"], first["between"], S - 1))
        out = dict(mean=first["mean"], ess_mean=first["ess"], sd=sd, mcse_mean=sd / np.sqrt(first["ess"]))
        e = d.astype(np.float64) - first["mean"]
        second = ess(e * e)
        out.update(ess_sd=second["ess"], mcse_sd=np.sqrt(((pooled(L, M, second["within"], second["between"], S) / second["ess"]) / second["mean"]) / 4.0))
        flat = d.reshape(S, P)
        xs = [sorted_draws(np.ascontiguousarray(flat[:, p])) for p in range(P)]
        out["quantile"] = np.array([[quantile_of(xs[p], q) for q in probs] for p in range(P)], dtype=np.float64).reshape(P, Q)
        out["ess_quantile"] = np.zeros((P, Q))
        for j in range(Q):
            out["ess_quantile"][:, j] = ess((d.astype(np.float64) <= out["quantile"][:, j]).astype(np.float64))["ess"]
        out["rank_lower"], out["rank_upper"] = np.zeros((P, Q), np.int64), np.zeros((P, Q), np.int64)
        out["mcse_quantile"] = np.full((P, Q), np.nan)
        for p in range(P):
            for j in range(Q):
                lo, hi = mcse_ranks(out["ess_quantile"][p, j], probs[j], S, beta)
                out["rank_lower"][p, j], out["rank_upper"][p, j] = lo, hi
                if lo >= 0:
                    out["mcse_quantile"][p, j] = (xs[p][hi] - xs[p][lo]) / 2.0
        out["hdi_lower"], out["hdi_upper"], out["hdi_start"] = np.full(P, np.nan), np.full(P, np.nan), np.full(P, -1, np.int64)
        if hdi_prob != 0:
            for p in range(P):
                out["hdi_lower"][p], out["hdi_upper"][p], out["hdi_start"][p] = hdi_of(xs[p], hdi_prob)
    out.update(sequence_length=L, num_sequences=M)
    return out
