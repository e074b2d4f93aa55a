"""The evidence ratios of mcmcpp_amd/csrc/evidence.hip, restated in numpy from the definition in include/mcmcpp_hip.h
(mcmcpp_hip_evidence_ratios) alone, taking the log-posteriors as input: importance weights between neighbouring rungs in both
directions, the fixed summation shape (sum_fixed of tests/rhat_restatement.py), evidence_exp and normal_score_log as their
headers spell them out, the effective sample size of tests/ess_restatement.py on the weights; every operation a float64
operation rounded on its own.  What the GPU returns equals this bit for bit; tests/test_evidence.py checks the restatement
itself against a long-double log-sum-exp."""
import numpy as np

from tests import ess_restatement as er
from tests import rank_restatement as rk
from tests import rhat_restatement as rr

FLUSH = -708.3964185322
LN2_HI, LN2_LO, INV_LN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.4426950408889634
COEFFS = (1.6059043836821613e-10, 2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05,
          0.0001984126984126984, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664, 0.16666666666666666, 0.5)  # c13 .. c2
KEYS = ("log_ratio", "mcse", "ess", "kish", "max_u")


def evidence_exp(x):
    """mcmcpp_amd/csrc/evidence_exp.hpp, line by line, on an array of float64"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(x.shape)
    nan = np.isnan(x)
    out[nan] = x[nan]
    live = ~nan & ~(x < FLUSH)
    v = x[live]
    with np.errstate(all="ignore"):
        kd = np.trunc(v * INV_LN2 - 0.5)
        r = (v - kd * LN2_HI) - kd * LN2_LO
        q = np.full(v.shape, COEFFS[0])
        for c in COEFFS[1:]:
            q = q * r + c
        p = 1.0 + (r + (r * r) * q)
        scale = ((1023 + kd.astype(np.int64)) << 52).view(np.float64)
        out[live] = p * scale
    return out


def max_u(u):
    """the largest u, +0 above -0 (none is NaN)"""
    m = u.max()
    if m == 0.0:
        m = np.float64(0.0) if (~np.signbit(u[u == 0.0])).any() else np.float64(-0.0)
    return np.float64(m)


def direction(u, n, W):
    """the figures of one (d, p) from its u [N], N = n W in the order i = s W + w: a dict of log_ratio (lme: the caller negates the
    reverse direction's), mcse, ess, kish, max_u, nonfinite"""
    u = np.asarray(u, dtype=np.float64)
    N = n * W
    assert u.shape == (N,) and n >= 4
    nan = np.float64(np.nan)
    out = dict(log_ratio=nan, mcse=nan, ess=nan, kish=nan, max_u=nan, nonfinite=int((~np.isfinite(u)).sum()))
    if np.isnan(u).any() or (u == np.inf).any():
        return out
    m = max_u(u)
    out["max_u"] = m
    if m == -np.inf:
        out["log_ratio"] = np.float64(-np.inf)
        return out
    with np.errstate(all="ignore"):
        e = evidence_exp(u - m)
        S1, S2 = rr.sum_fixed(e), rr.sum_fixed(e * e)
        Nd = np.float64(N)
        wbar = S1 / Nd
        lme = m + rk.normal_score_log(np.array([wbar]))[0]
        var = S2 / Nd - wbar * wbar
        rel2 = (var if var > 0.0 else np.float64(0.0)) / (wbar * wbar)
        ess = er.effective_sample_size(e.reshape(1, n, W, 1), split=True, max_lag=0)["ess"][0]
        out.update(log_ratio=np.float64(lme), kish=np.float64((S1 * S1) / S2), ess=np.float64(ess),
                   mcse=np.float64(0.0) if rel2 == 0.0 else np.float64(np.sqrt(rel2 / ess)), weights=e)
    return out


def evidence_ratios(logp_own, logp_lower, logp_upper):
    """logp_own [K][n][W]: rung k's log-posterior of its own draws; logp_lower [K][n][W]: rung k - 1's of rung k's draws (row 0
    unused); logp_upper [K][n][W]: rung k + 1's of rung k's draws (row K - 1 unused); float32 or float64, as calc_logp returned
    them.  A dict of float64 arrays [2][K - 1] (nonfinite: int64), the totals [2], and num_draws."""
    own, lower, upper = (np.asarray(a) for a in (logp_own, logp_lower, logp_upper))
    K, n, W = own.shape
    N = n * W
    out = {key: np.full((2, K - 1), np.nan) for key in KEYS}
    out["nonfinite"] = np.zeros((2, K - 1), np.int64)
    with np.errstate(all="ignore"):
        for p in range(K - 1):
            a, b = p, p + 1
            us = ((lower[b].astype(np.float64) - own[b].astype(np.float64)).reshape(N),  # d = 0: the draws of b
                  (upper[a].astype(np.float64) - own[a].astype(np.float64)).reshape(N))  # d = 1: the draws of a
            for d, u in enumerate(us):
                got = direction(u, n, W)
                for key in KEYS + ("nonfinite",):
                    out[key][d, p] = got[key]
            out["log_ratio"][1, p] = -out["log_ratio"][1, p]
        total, squares = np.zeros(2), np.zeros(2)
        for p in range(K - 1):
            total = total + out["log_ratio"][:, p]
            squares = squares + out["mcse"][:, p] * out["mcse"][:, p]
        out["log_ratio_total"], out["mcse_total"] = total, np.sqrt(squares)
    out["num_draws"] = N
    return out


def log_mean_exp_long_double(u):
    """log of the mean of exp(u) in long double: what the restatement is measured against"""
    u = np.asarray(u, dtype=np.longdouble)
    m = u.max()
    return m + np.log(np.exp(u - m).mean())
