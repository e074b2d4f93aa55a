"""The Gelman-Rubin split R-hat of mcmcpp_amd/csrc/rhat.hip, restated in numpy from the definition in include/mcmcpp_hip.h
(mcmcpp_hip_gelman_rubin) alone: the same sequences, the same fixed summation shape (sum_fixed), every operation a float64
operation rounded on its own.  What the GPU returns equals this bit for bit; tests/test_rhat.py checks the restatement itself
against a long-double two-pass computation."""
import numpy as np


def slice_len(N):
    """terms of a slice of a sum over N terms: max(1024, ceil(N / 64) rounded up to a multiple of 64)"""
    per = -(-N // 64)
    per = -(-per // 64) * 64
    return max(1024, per)


def num_slices(N):
    return -(-N // slice_len(N))


def sum_fixed(v, term=None):
    """the sum of v[0], ..., v[N - 1] (v [(N, ...)], summed over axis 0) or, with term given, of term(0), ..., term(v - 1), in
    float64: consecutive slices of slice_len(N) terms, each summed in ascending order from +0, then the slice sums added in
    ascending order"""
    if term is None:
        v = np.asarray(v, dtype=np.float64)
        N, term = v.shape[0], v.__getitem__
    else:
        N = v
    sl = slice_len(N)
    total = None
    for b in range(0, N, sl):
        acc = np.float64(0.0)
        for s in range(b, min(b + sl, N)):
            acc = acc + term(s)
        total = acc if total is None else total + acc
    return total


def halves(n, split):
    """[(first used step, L)] of the halves of n used steps"""
    L = n // 2 if split else n
    return [(0, L), (n - L, L)] if split else [(0, L)]


def gelman_rubin(steps, split=True, slice_interval=1):
    """steps [(K, n, W, P)] or [(n, W, P)] of float32 or float64.  A dict of float64 arrays: rhat, mean, within, between [(P,)];
    chain_mean, chain_within [(K, P)]; sequence_mean, sequence_m2 [(M, P)]; and the ints sequence_length, num_sequences."""
    x = np.asarray(steps)
    if x.ndim == 3:
        x = x[None]
    x = x[:, ::slice_interval]
    K, n, W, P = x.shape
    parts = halves(n, split)
    H, L = len(parts), parts[0][1]
    M = K * H * W
    assert L >= 2 and M >= 2
    seq_mean, seq_m2 = np.empty((K, H, W, P)), np.empty((K, H, W, P))
    with np.errstate(all="ignore"):
        for h, (a, _) in enumerate(parts):
            seq = np.moveaxis(x[:, a:a + L], 1, 0)  # [L][K][W][P]
            c = seq[0].astype(np.float64)  # (an fp32 sample converts exactly)
            S1 = sum_fixed(L, lambda s: seq[s].astype(np.float64) - c)
            S2 = sum_fixed(L, lambda s: (seq[s].astype(np.float64) - c) * (seq[s].astype(np.float64) - c))
            q = S1 / np.float64(L)
            r = S2 - S1 * q
            seq_mean[:, h] = c + q
            seq_m2[:, h] = np.where(r < 0, 0.0, r)
        mean_m, m2_m = seq_mean.reshape(M, P), seq_m2.reshape(M, P)
        v_m = m2_m / np.float64(L - 1)
        within = sum_fixed(v_m) / np.float64(M)
        mean = sum_fixed(mean_m) / np.float64(M)
        e = mean_m - mean
        between = sum_fixed(e * e) / np.float64(M - 1)
        varplus = (within * np.float64(L - 1)) / np.float64(L) + between
        rhat = np.sqrt(varplus / within)
        chain_mean = np.stack([sum_fixed(mean_m[k * H * W:(k + 1) * H * W]) / np.float64(H * W) for k in range(K)])
        chain_within = np.stack([sum_fixed(v_m[k * H * W:(k + 1) * H * W]) / np.float64(H * W) for k in range(K)])
    return dict(rhat=rhat, mean=mean, within=within, between=between, chain_mean=chain_mean, chain_within=chain_within, sequence_mean=mean_m.copy(),
                sequence_m2=m2_m.copy(), sequence_length=L, num_sequences=M)


def two_pass_long_double(steps, split=True, slice_interval=1):
    """the same quantities by the textbook two-pass formulas in long double: what the restatement is measured against"""
    x = np.asarray(steps)
    if x.ndim == 3:
        x = x[None]
    x = x[:, ::slice_interval].astype(np.longdouble)
    K, n, W, P = x.shape
    parts = halves(n, split)
    H, L = len(parts), parts[0][1]
    M = K * H * W
    seqs = np.stack([x[k, a:a + L] for k in range(K) for a, _ in parts])  # [K H][L][W][P]
    seqs = seqs.transpose(0, 2, 1, 3).reshape(M, L, P)
    mean_m = seqs.mean(axis=1)
    v_m = ((seqs - mean_m[:, None, :]) ** 2).sum(axis=1) / (L - 1)
    within, mean = v_m.mean(axis=0), mean_m.mean(axis=0)
    between = ((mean_m - mean) ** 2).sum(axis=0) / (M - 1)
    varplus = within * (L - 1) / L + between
    return dict(rhat=np.sqrt(varplus / within), mean=mean, within=within, between=between, chain_mean=mean_m.reshape(K, H * W, P).mean(axis=1),
                chain_within=v_m.reshape(K, H * W, P).mean(axis=1), sequence_mean=mean_m, sequence_m2=v_m * (L - 1))
