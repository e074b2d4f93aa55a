"""The bridge estimate of mcmcpp_amd/csrc/bridge.hip, restated in numpy from the definition in include/mcmcpp_hip.h
(mcmcpp_hip_evidence_bridge) alone, taking the log-posteriors as input: sigma through evidence_exp as its header spells it out
(tests/evidence_restatement.py), sum_tree, the solver pass by pass, the effective sample size of tests/ess_restatement.py on
h_d(c*); every operation a float64 operation rounded on its own.  What the GPU returns equals this bit for bit;
tests/test_evidence_bridge.py checks the restatement itself against long double."""
import numpy as np

from tests import ess_restatement as er
from tests import evidence_restatement as ev
from tests import rank_restatement as rk

TILE, LANES, SLICE_TILES = 1024, 256, 64
BRACKET_PASSES, NEWTON_PASSES = 1100, 200
TOLERANCE = 2.0 ** -40
DBL_MAX = np.finfo(np.float64).max
PAIR_KEYS = ("log_ratio", "mcse", "overlap", "passes", "converged")


def sigma(x):
    """sigma(x) = 1 / (1 + evidence_exp(-x)) for x >= 0, e / (1 + e) with e = evidence_exp(x) for x < 0, on an array of float64"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape)
    up = x >= 0.0
    with np.errstate(all="ignore"):
        out[up] = 1.0 / (1.0 + ev.evidence_exp(-x[up]))
        e = ev.evidence_exp(x[~up])
        out[~up] = e / (1.0 + e)
    return out


def sum_tree(v):
    """tiles of 1024 terms (missing: +0); lane t of 256 forms ((v[2t] + v[2t+1]) + v[2t+512]) + v[2t+513]; s = 128 .. 1:
    p_t = p_t + p_{t+s}; tile sums in ascending order from +0 within slices of 64 tiles; slice sums in ascending order from +0"""
    v = np.asarray(v, dtype=np.float64).ravel()
    tiles = -(-v.size // TILE)
    a = np.zeros(tiles * TILE)
    a[:v.size] = v
    a = a.reshape(tiles, 2, LANES, 2)  # [tile][half][lane][term of the lane's pair]
    p = ((a[:, 0, :, 0] + a[:, 0, :, 1]) + a[:, 1, :, 0]) + a[:, 1, :, 1]
    s = LANES // 2
    while s >= 1:
        p = p[:, :s] + p[:, s:2 * s]
        s //= 2
    p = p[:, 0]
    total = np.float64(0.0)
    for first in range(0, tiles, SLICE_TILES):
        acc = np.float64(0.0)
        for t in p[first:first + SLICE_TILES]:
            acc = acc + t
        total = total + acc
    return np.float64(total)


def one_pass(u0, u1, c, final=False):
    """S_0, S_1, Q_0, Q_1 at c (and, on the final pass, H_0, H_1 and the h themselves)"""
    with np.errstate(all="ignore"):
        h = (sigma(u0 - c), sigma(u1 + c))
        S = [sum_tree(x) for x in h]
        Q = [sum_tree(x * (1.0 - x)) for x in h]
        if not final:
            return S, Q
        return S, Q, [sum_tree(x * x) for x in h], h


def solve(u0, u1):
    """the solver of the header: (c*, passes, converged) in front of the final pass, which the caller makes and counts"""
    passes = 0
    state = {}

    def go(c):
        S, Q = one_pass(u0, u1, c)
        state["g"], state["S"], state["Q"] = S[0] - S[1], S, Q
        return state["g"]

    c = np.float64(0.0)
    g = go(c)
    passes += 1
    if g == 0.0:
        return c, passes, 1
    up = g > 0.0
    step = np.float64(1.0)
    with np.errstate(all="ignore"):
        while True:
            prev = c
            c = prev + step if up else prev - step
            c = np.float64(min(max(c, -DBL_MAX), DBL_MAX))
            step = step + step
            g = go(c)
            passes += 1
            if g == 0.0:
                return c, passes, 1
            if (g > 0.0) != up:
                lo, hi = (prev, c) if up else (c, prev)
                break
            if passes >= BRACKET_PASSES:
                return c, passes, 0
        for _ in range(NEWTON_PASSES):
            mid = 0.5 * lo + 0.5 * hi
            S, Q = state["S"], state["Q"]
            nxt = mid
            if S[0] > 0.0 and S[1] > 0.0:
                ln = rk.normal_score_log(np.array([S[0], S[1]]))
                f, fp = ln[0] - ln[1], -(Q[0] / S[0] + Q[1] / S[1])
                if fp != 0.0:
                    nxt = c - f / fp
            if not (lo < nxt < hi):
                nxt = mid
            if nxt == lo or nxt == hi:
                return c, passes, 1
            if abs(nxt - c) <= TOLERANCE * max(1.0, abs(nxt)):
                return nxt, passes, 1
            c = nxt
            g = go(c)
            passes += 1
            if g == 0.0:
                return c, passes, 1
            if g > 0.0:
                lo = c
            else:
                hi = c
    return c, passes, 0


def pair(u0, u1, n, W):
    """the figures of one pair from u0 [N] (on the draws of rung p + 1) and u1 [N] (on the draws of rung p), N = n W in the order
    i = s W + w: a dict of log_ratio, mcse, overlap, ess [2], passes, converged, nonfinite [2]"""
    u0, u1 = (np.asarray(u, dtype=np.float64) for u in (u0, u1))
    N = n * W
    assert u0.shape == (N,) and u1.shape == (N,) and n >= 4
    nan = np.float64(np.nan)
    out = dict(log_ratio=nan, mcse=nan, overlap=nan, ess=np.array([nan, nan]), passes=0, converged=0,
               nonfinite=np.array([int((~np.isfinite(u)).sum()) for u in (u0, u1)], np.int64))
    if any(np.isnan(u).any() or (u == np.inf).any() for u in (u0, u1)):
        return out
    c, passes, converged = solve(u0, u1)
    S, Q, H, h = one_pass(u0, u1, c, final=True)
    out.update(passes=passes + 1, converged=converged, c=np.float64(c), S=S, Q=Q, h=h)
    if S[0] == 0.0 or S[1] == 0.0:
        out["overlap"] = np.float64(0.0)
        return out
    with np.errstate(all="ignore"):
        Nd = np.float64(N)
        total = np.float64(0.0)
        for d in range(2):
            mean = S[d] / Nd
            var = H[d] / Nd - mean * mean
            rel2 = (var if var > 0.0 else np.float64(0.0)) / (mean * mean)
            ess = np.float64(er.effective_sample_size(h[d].reshape(1, n, W, 1), split=True, max_lag=0)["ess"][0])
            out["ess"][d] = ess
            total = total + (np.float64(0.0) if rel2 == 0.0 else rel2 / ess)
        out.update(log_ratio=np.float64(c), overlap=np.float64((S[0] + S[1]) / Nd), mcse=np.float64(np.sqrt(total)))
    return out


def evidence_bridge(logp_own, logp_lower, logp_upper):
    """logp_own, logp_lower, logp_upper [K][n][W] as for tests/evidence_restatement.py's evidence_ratios.  A dict of log_ratio, mcse,
    overlap [K - 1] float64, passes, converged [K - 1] int64, ess [2][K - 1], nonfinite [2][K - 1] int64, the totals and num_draws."""
    own, lower, upper = (np.asarray(a) for a in (logp_own, logp_lower, logp_upper))
    K, n, W = own.shape
    N = n * W
    out = {key: np.full(K - 1, np.nan) for key in ("log_ratio", "mcse", "overlap")}
    out.update(passes=np.zeros(K - 1, np.int64), converged=np.zeros(K - 1, np.int64), ess=np.full((2, K - 1), np.nan), nonfinite=np.zeros((2, K - 1), np.int64))
    with np.errstate(all="ignore"):
        for p in range(K - 1):
            a, b = p, p + 1
            u0 = (lower[b].astype(np.float64) - own[b].astype(np.float64)).reshape(N)  # on the draws of b
            u1 = (upper[a].astype(np.float64) - own[a].astype(np.float64)).reshape(N)  # on the draws of a
            got = pair(u0, u1, n, W)
            for key in PAIR_KEYS:
                out[key][p] = got[key]
            out["ess"][:, p], out["nonfinite"][:, p] = got["ess"], got["nonfinite"]
        total, squares = np.float64(0.0), np.float64(0.0)
        for p in range(K - 1):
            total = total + out["log_ratio"][p]
            squares = squares + out["mcse"][p] * out["mcse"][p]
        out["log_ratio_total"], out["mcse_total"] = np.float64(total), np.float64(np.sqrt(squares))
    out["num_draws"] = N
    return out


def g_long_double(u0, u1, c):
    """g(c) in long double with libm's exponential: what the restatement's root is measured against"""
    u0, u1, c = np.asarray(u0, np.longdouble), np.asarray(u1, np.longdouble), np.longdouble(c)
    with np.errstate(all="ignore"):
        return (1 / (1 + np.exp(-(u0 - c)))).sum() - (1 / (1 + np.exp(-(u1 + c)))).sum()
