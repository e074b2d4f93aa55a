"""The multi-sequence effective sample size of mcmcpp_amd/csrc/ess.hip, restated in numpy from the definition in
include/mcmcpp_hip.h (mcmcpp_hip_effective_sample_size) alone: the R-hat state of tests/rhat_restatement.py, plain ascending
lagged products per sequence, sum_fixed over the sequences, Geyer's initial monotone sequence; every operation a float64
operation rounded on its own.  What the GPU returns equals this bit for bit; tests/test_ess.py checks the restatement itself
against a long-double direct computation."""
import math

import numpy as np

from tests import rhat_restatement as rr


def sequences(steps, split=True, slice_interval=1):
    """the samples as sequences [L][M][P] in the chain's type, m = (k H + h) W + w"""
    x = np.asarray(steps)
    if x.ndim == 3:
        x = x[None]
    x = x[:, ::slice_interval]
    K, n, W, P = x.shape
    parts = rr.halves(n, split)
    L = parts[0][1]
    seqs = np.stack([x[:, a:a + L] for a, _ in parts], axis=1)  # [K][H][L][W][P]
    return np.ascontiguousarray(seqs.transpose(2, 0, 1, 3, 4)).reshape(L, K * len(parts) * W, P)


def window_shape(L, max_lag):
    cap = L - 1 if max_lag == 0 else min(max_lag, L - 1)
    return cap, (cap - 1) // 2


def lagged_products(e, t0, t1):
    """A[t - t0][m][p] for t in [t0, t1): e_0 e_t + e_1 e_(t+1) + ..., added in ascending s from +0"""
    L = e.shape[0]
    acc = np.zeros((t1 - t0,) + e.shape[1:])
    for s in range(L):
        hi = min(t1, L - s)
        if hi > t0:
            acc[:hi - t0] = acc[:hi - t0] + e[s] * e[s + t0:s + hi]
    return acc


def walk_window(rho, kmax):
    """(total, pairs summed, closed) by the window rule, over rho[0 .. 2 kmax + 1]; None where rho is too short to decide"""
    total, q, pairs = np.float64(0.0), None, 0
    for k in range(kmax + 1):
        if 2 * k + 1 >= len(rho):
            return None
        p = rho[2 * k] + rho[2 * k + 1]
        if k >= 1 and not p >= 0:
            return total, pairs, 1
        q = p if k == 0 else (p if p < q else q)
        total = q if k == 0 else total + q
        pairs = k + 1
    return total, pairs, 0


def effective_sample_size(steps, split=True, max_lag=0, n_functions=0, slice_interval=1, first_lags=64):
    """A dict: ess, tau [(P,)] float64, lags_used, closed [(P,)] int64, rho, autocov [(P, n_functions)], the R-hat outputs rhat,
    mean, within, between, and sequence_length, num_sequences.  first_lags: how many lags are evaluated before the windows are
    first walked (no value depends on it)."""
    g = rr.gelman_rubin(steps, split, slice_interval)
    L, M = g["sequence_length"], g["num_sequences"]
    P = g["mean"].shape[0]
    cap, kmax = window_shape(L, max_lag)
    F = min(n_functions, cap + 1)
    needed = max(2 * kmax + 2, F)
    with np.errstate(all="ignore"):
        e = sequences(steps, split, slice_interval).astype(np.float64) - g["sequence_mean"]
        within, varplus = g["within"], (g["within"] * np.float64(L - 1)) / np.float64(L) + g["between"]
        gamma = np.zeros((0, P))
        size = max(first_lags, F, 1)
        while True:
            t0, t1 = gamma.shape[0], min(gamma.shape[0] + size, needed)
            A = lagged_products(e, t0, t1)  # [lags][M][P]
            S = rr.sum_fixed(np.ascontiguousarray(A.transpose(1, 0, 2)))  # over m
            gamma = np.concatenate([gamma, (S / np.float64(M)) / np.float64(L)])
            rho = 1.0 - (within - gamma) / varplus
            rho[0] = 1.0
            walks = [walk_window(rho[:, p], kmax) for p in range(P)]
            if gamma.shape[0] >= needed or (gamma.shape[0] >= F and all(w is not None for w in walks)):
                break
            size *= 2
        N = np.float64(M * L)
        floor = np.float64(1.0 / math.log10(float(N)))
        tau = np.array([-1.0 + 2.0 * w[0] for w in walks])
        tau = np.where(tau < floor, floor, tau)
        out = dict(ess=N / tau, tau=tau, lags_used=np.array([2 * w[1] for w in walks], np.int64), closed=np.array([w[2] for w in walks], np.int64))
    out["rho"], out["autocov"] = np.full((P, n_functions), np.nan), np.full((P, n_functions), np.nan)
    out["rho"][:, :F], out["autocov"][:, :F] = rho[:F].T, gamma[:F].T
    for key in ("rhat", "mean", "within", "between", "sequence_length", "num_sequences"):
        out[key] = g[key]
    return out


def direct_long_double(steps, split=True, max_lag=0, n_functions=0, slice_interval=1):
    """the same quantities by the textbook formulas in long double (two-pass means, direct lagged products, plain sums), the
    same window rule: what the restatement is measured against.  Also `closing`: the P_k that closed each window (NaN: none)."""
    x = sequences(steps, split, slice_interval).astype(np.longdouble)
    L, M, P = x.shape
    cap, kmax = window_shape(L, max_lag)
    F = min(n_functions, cap + 1)
    needed = max(2 * kmax + 2, F)
    mean_m = x.mean(axis=0)
    e = x - mean_m
    within = ((e ** 2).sum(axis=0) / (L - 1)).mean(axis=0)
    between = ((mean_m - mean_m.mean(axis=0)) ** 2).sum(axis=0) / (M - 1)
    varplus = within * (L - 1) / L + between
    gamma = np.stack([(e[:L - t] * e[t:]).sum(axis=0).mean(axis=0) / L for t in range(needed)])
    rho = 1 - (within - gamma) / varplus
    rho[0] = 1
    N = np.longdouble(M * L)
    tau, closing, lags_used, closed = np.zeros(P, np.longdouble), np.full(P, np.nan), np.zeros(P, np.int64), np.zeros(P, np.int64)
    for p in range(P):
        total, pairs, closed[p] = walk_window(rho[:, p], kmax)
        lags_used[p] = 2 * pairs
        if closed[p]:
            closing[p] = float(rho[2 * pairs, p] + rho[2 * pairs + 1, p])
        tau[p] = max(-1 + 2 * total, 1 / np.log10(N))
    return dict(ess=N / tau, tau=tau, lags_used=lags_used, closed=closed, rho=rho[:F].T, autocov=gamma[:F].T, closing=closing)
