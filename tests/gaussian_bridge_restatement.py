"""The evidence by a bridge to a fitted Gaussian (mcmcpp_amd/csrc/gaussian_bridge.hip), restated in numpy from the definition in
include/mcmcpp_hip.h (mcmcpp_hip_evidence_gaussian) alone, taking the log-posteriors as input: the proposals from the raw pcg64
stream of tests/de_stream_restatement.py through the normal score of tests/rank_restatement.py, log q by forward substitution,
the two u arrays, and from there tests/bridge_restatement.py's pair; every operation a float64 operation rounded on its own.  What
the GPU returns equals this bit for bit."""
import numpy as np

from tests import bridge_restatement as br
from tests import de_stream_restatement as ds
from tests import rank_restatement as rk

MAX_D = 64
HALF_LOG_2PI = 0.91893853320467274178
FIGURES = ("log_evidence", "mcse", "overlap", "ess", "passes", "converged", "nonfinite")


def state_at(seed, stream, position):
    """(state, inc) of pcg64(seed, stream) after `position` steps: the LCG's map composed with itself by squaring"""
    state, inc = ds.seed_engine(seed, stream)
    mult, plus, acc_mult, acc_plus = ds.MULT, inc, 1, 0
    while position > 0:
        if position & 1:
            acc_mult, acc_plus = (acc_mult * mult) & ds.M128, (acc_plus * mult + plus) & ds.M128
        plus = ((mult + 1) * plus) & ds.M128
        mult = (mult * mult) & ds.M128
        position >>= 1
    return (acc_mult * state + acc_plus) & ds.M128, inc


def raws(seed, stream, first, count):
    """the raw outputs at positions first .. first + count - 1: draw k is the output of the state after k + 1 steps"""
    state, inc = state_at(seed, stream, first)
    out = np.empty(count, np.uint64)
    for k in range(count):
        state = ds.step(state, inc)
        out[k] = ds.output(state)
    return out


def p_of(r):
    """p = ((r >> 12) + 0.5) 2^-52: both operations exact"""
    return ((np.asarray(r, np.uint64) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def lower(chol):
    L = np.asarray(chol, np.float64)
    return L.reshape(int(round(np.sqrt(L.size))), -1)


def rows_from_raws(mean, chol, r, dtype):
    """x_i = mean_i + acc_i, acc_i from +0, + L[i][d] z[d] for d = 0 .. i ascending; rounded once to dtype.  r [N][D]"""
    mean, L = np.asarray(mean, np.float64), lower(chol)
    z = rk.normal_score(p_of(r).ravel()).reshape(r.shape)
    x = np.empty(z.shape)
    for i in range(z.shape[1]):
        acc = np.zeros(z.shape[0])
        for d in range(i + 1):
            acc = acc + L[i, d] * z[:, d]
        x[:, i] = mean[i] + acc
    return x.astype(dtype)


def proposals(mean, chol, N, seed, stream, dtype, first=0):
    """proposals first .. first + N - 1: coordinate d of proposal j takes the raw output at position j D + d"""
    D = len(mean)
    return rows_from_raws(mean, chol, raws(seed, stream, first * D, N * D).reshape(N, D), dtype)


def log_norm(chol):
    """k = -(sum of normal_score_log(L[i][i]), ascending from +0) - D 0.91893853320467274178"""
    L = lower(chol)
    s = np.float64(0.0)
    for i in range(L.shape[0]):
        s = s + rk.normal_score_log(np.array([L[i, i]]))[0]
    return -s - np.float64(L.shape[0]) * HALF_LOG_2PI


def log_q(x, mean, chol):
    """log q of the rows x [N][D] of either dtype, widened exactly"""
    mean, L = np.asarray(mean, np.float64), lower(chol)
    x = np.asarray(x).astype(np.float64)
    z = np.empty(x.shape)
    s = np.zeros(x.shape[0])
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            t = np.zeros(x.shape[0])
            for d in range(i):
                t = t + L[i, d] * z[:, d]
            z[:, i] = ((x[:, i] - mean[i]) - t) / L[i, i]
            s = s + z[:, i] * z[:, i]
        return (-0.5 * s) + log_norm(chol)


def refused(mean, chol):
    """what the call refuses of a Gaussian: None, or (code name, reason)"""
    mean, L = np.asarray(mean, np.float64), lower(chol)
    D = len(mean)
    if D > MAX_D:
        return "E_UNSUPPORTED", "too wide"
    if not np.isfinite(mean).all():
        return "E_ARG", "mean"
    if not np.isfinite(L[np.tril_indices(D)]).all():
        return "E_ARG", "factor"
    if not (np.diag(L) >= np.finfo(np.float64).tiny).all():
        return "E_ARG", "diagonal"
    return None


def evidence_gaussian(logp_proposals, logp_draws, x, y, mean, chol, n, W):
    """logp_proposals [N] on the proposals x [N][D] and logp_draws [N] on the draws y [N][D], N = n W in the order i = s W + w, in
    the handle's dtype.  A dict of log_evidence, mcse, overlap, ess [2], passes, converged, nonfinite [2], num_draws, log_q [2][N]."""
    N = n * W
    lq = np.stack([log_q(np.asarray(x).reshape(N, -1), mean, chol), log_q(np.asarray(y).reshape(N, -1), mean, chol)])
    with np.errstate(all="ignore"):
        u0 = np.asarray(logp_proposals).reshape(N).astype(np.float64) - lq[0]
        u1 = lq[1] - np.asarray(logp_draws).reshape(N).astype(np.float64)
        got = br.pair(u0, u1, n, W)
    out = dict(log_evidence=np.float64(got["log_ratio"]), mcse=np.float64(got["mcse"]), overlap=np.float64(got["overlap"]), ess=got["ess"],
               passes=np.int64(got["passes"]), converged=np.int64(got["converged"]), nonfinite=got["nonfinite"], num_draws=N, log_q=lq, u=(u0, u1))
    if "h" in got:
        out["h"] = got["h"]
    return out


def fit(draws):
    """mean and lower Cholesky factor of the sample covariance (N - 1) of draws [N][D], for the tests of the restatement itself"""
    y = np.asarray(draws, np.float64)
    return y.mean(axis=0), np.linalg.cholesky(np.cov(y.T).reshape(y.shape[1], y.shape[1]))
