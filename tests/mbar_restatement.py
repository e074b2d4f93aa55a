"""The multistate Bennett acceptance ratio of mcmcpp_amd/csrc/mbar.hip, restated in numpy from the definition in
include/mcmcpp_hip.h (mcmcpp_hip_evidence_mbar) alone, taking the log-posteriors l [K][K N] as input: the weights through
evidence_exp as its header spells it out (tests/evidence_restatement.py), sum_tree (tests/bridge_restatement.py), the Cholesky
solve and the solver pass by pass in the header's order, the effective sample size of tests/ess_restatement.py on each rung's
own weights, the sandwich covariance; every operation a float64 operation rounded on its own.  What the GPU returns equals this
bit for bit; tests/test_evidence_mbar.py checks the restatement itself against the bridge's root, a known answer, the spread
over seeds, and its invariances."""
import numpy as np

from tests import bridge_restatement as br
from tests import ess_restatement as er
from tests import evidence_restatement as ev

SOLVER_PASSES, STEP_CAP, TOLERANCE = 200, 4.0, 2.0 ** -40
PASS_BOUND = SOLVER_PASSES + 1
FLOAT_KEYS = ("log_z", "cov", "log_ratio", "mcse", "ess", "log_ratio_total", "mcse_total")
KEYS = FLOAT_KEYS + ("nonfinite", "passes", "converged")


def weights(l, zeta):
    """w [K][J] of the draws l [K][J] at zeta [K]"""
    K = l.shape[0]
    with np.errstate(all="ignore"):
        a = l - np.asarray(zeta, np.float64).reshape(K, 1)
        m = a[0].copy()
        for k in range(1, K):
            m = np.where(a[k] > m, a[k], m)
        dead = m == -np.inf
        e = np.stack([ev.evidence_exp(a[k] - m) for k in range(K)])
        dn = np.zeros(l.shape[1])
        for k in range(K):
            dn = dn + e[k]
        w = e / dn
    w[:, dead] = 0.0
    return w


def sums(w):
    """S [K], P [K][K] (both triangles) of the weights w [K][J] over the J terms: sum_tree"""
    K = w.shape[0]
    S = np.array([br.sum_tree(w[k]) for k in range(K)])
    P = np.zeros((K, K))
    for k in range(K):
        for l in range(k, K):
            P[k, l] = P[l, k] = br.sum_tree(w[k] * w[l])
    return S, P


def system(S, P, N):
    """A [K-1][K-1], G [K-1]"""
    M = S.size - 1
    A = -P[:M, :M]
    for k in range(M):
        A[k, k] = S[k] - P[k, k]
    return A, S[:M] - np.float64(N)


def factor(A):
    """L with A = L L^T in the header's order, or None where a pivot is not positive"""
    M = A.shape[0]
    L = np.zeros((M, M))
    for i in range(M):
        for j in range(i):
            t = A[i, j]
            for k in range(j):
                t = t - L[i, k] * L[j, k]
            L[i, j] = t / L[j, j]
        d = A[i, i]
        for k in range(i):
            d = d - L[i, k] * L[i, k]
        if not d > 0.0:
            return None
        L[i, i] = np.sqrt(d)
    return L


def substitute(L, b):
    M = L.shape[0]
    y, x = np.zeros(M), np.zeros(M)
    for i in range(M):
        t = b[i]
        for k in range(i):
            t = t - L[i, k] * y[k]
        y[i] = t / L[i, i]
    for i in range(M - 1, -1, -1):
        t = y[i]
        for k in range(i + 1, M):
            t = t - L[k, i] * x[k]
        x[i] = t / L[i, i]
    return x


def solve(l, N):
    """the solver: (zeta [K], passes, converged, failed) in front of the final pass, which the caller makes and counts"""
    K = l.shape[0]
    M = K - 1
    zeta = np.zeros(K)
    passes = 0
    with np.errstate(all="ignore"):
        for _ in range(SOLVER_PASSES):
            S, P = sums(weights(l, zeta))
            passes += 1
            A, G = system(S, P, N)
            L = factor(A)
            if L is None:
                return zeta, passes, 1, True
            delta = substitute(L, G)
            mx = np.abs(delta).max()
            if mx > STEP_CAP:
                delta = delta * (STEP_CAP / mx)
                mx = np.abs(delta).max()
            zeta[:M] = zeta[:M] + delta
            if mx <= TOLERANCE * max(1.0, np.abs(zeta[:M]).max()):
                return zeta, passes, 1, False
    return zeta, passes, 0, False


def covariance(L, rung_S, rung_P, ess, N):
    """cov [K][K] from the factor behind the final pass, the rungs' sums M [K][K] and P^r [K][K][K], and ess [K]"""
    K = rung_S.shape[0]
    M = K - 1
    Nd = np.float64(N)
    with np.errstate(all="ignore"):
        V = np.zeros((M, M))
        for r in range(K):
            f = (Nd * Nd) / ess[r]
            for k in range(M):
                for l in range(k, M):
                    c = rung_P[r, k, l] / Nd - (rung_S[r, k] / Nd) * (rung_S[r, l] / Nd)
                    V[k, l] = V[k, l] + (np.float64(0.0) if c == 0.0 else f * c)
        for k in range(M):
            for l in range(k):
                V[k, l] = V[l, k]
        Y = np.zeros((M, M))
        for c in range(M):
            Y[:, c] = substitute(L, V[:, c])
        cov = np.zeros((K, K))
        for c in range(M):
            cov[c, :M] = substitute(L, Y[c, :])
    return cov


def _root(v):
    with np.errstate(all="ignore"):
        return np.float64(0.0) if v < 0.0 else np.float64(np.sqrt(v))


def mbar(l, n, W):
    """l [K][K N]: l[k][r N + i] the log-posterior of draw i of rung r under chain k, N = n W in the order i = s W + w.  A dict of
    log_z [K], cov [K][K], log_ratio, mcse [K-1], ess [K], nonfinite [K][K] int64, log_ratio_total, mcse_total, passes, converged,
    num_draws."""
    l = np.asarray(l, dtype=np.float64)
    K = l.shape[0]
    N = n * W
    assert l.shape == (K, K * N) and n >= 4 and K >= 2
    nan = np.float64(np.nan)
    out = dict(log_z=np.full(K, nan), cov=np.full((K, K), nan), log_ratio=np.full(K - 1, nan), mcse=np.full(K - 1, nan), ess=np.full(K, nan),
               log_ratio_total=nan, mcse_total=nan, passes=np.int64(0), converged=np.int64(0), num_draws=N,
               nonfinite=np.array([[int((~np.isfinite(l[k, r * N:(r + 1) * N])).sum()) for k in range(K)] for r in range(K)], np.int64))
    if np.isnan(l).any() or (l == np.inf).any():
        return out
    zeta, passes, converged, failed = solve(l, N)
    out.update(passes=np.int64(passes), converged=np.int64(converged))
    if failed:
        return out
    w = weights(l, zeta)
    S, P = sums(w)
    out["passes"] = np.int64(passes + 1)
    L = factor(system(S, P, N)[0])
    if L is None:
        out["converged"] = np.int64(1)
        return out
    rung = [sums(w[:, r * N:(r + 1) * N]) for r in range(K)]
    with np.errstate(all="ignore"):
        ess = np.array([er.effective_sample_size(w[r, r * N:(r + 1) * N].reshape(1, n, W, 1), split=True, max_lag=0)["ess"][0] for r in range(K)], np.float64)
        cov = covariance(L, np.stack([s for s, _ in rung]), np.stack([p for _, p in rung]), ess, N)
        out.update(log_z=zeta.copy(), cov=cov, ess=ess, log_ratio=zeta[:-1] - zeta[1:], log_ratio_total=np.float64(zeta[0]), mcse_total=_root(cov[0, 0]),
                   mcse=np.array([_root((cov[p, p] + cov[p + 1, p + 1]) - 2.0 * cov[p, p + 1]) for p in range(K - 1)]), w=w)
    return out


def from_logp(logp):
    """logp [K chains][K rungs][n][W] as calc_logp(draws of rung r, chain=k) returns them -> l [K][K N], widened to double"""
    logp = np.asarray(logp)
    K = logp.shape[0]
    return logp.astype(np.float64).reshape(K, -1)


def l_of_pair(u0, u1):
    """l [2][2 N] of the pair whose bridge differences are u0 (on the draws of rung 1) and u1 (on the draws of rung 0): each draw's
    own log-posterior is taken as 0, which no weight depends on"""
    N = u0.size
    l = np.zeros((2, 2 * N))
    l[1, :N], l[0, N:] = u1, u0
    return l


def iid_ladder(D, betas, N, seed):
    """l [K][K N] of N iid draws from each exact Gaussian exp(-beta_r |x|^2 / 2) of a ladder: log(Z_p / Z_q) = (D / 2) log(beta_q / beta_p)"""
    rng = np.random.default_rng(seed)
    K = len(betas)
    l = np.zeros((K, K * N))
    for r, b in enumerate(betas):
        r2 = (rng.standard_normal((N, D)) ** 2).sum(axis=1) / b
        for k, bk in enumerate(betas):
            l[k, r * N:(r + 1) * N] = -0.5 * bk * r2
    return l
