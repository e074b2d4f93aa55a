"""The definition of mcmcpp_hip_normal_scores and mcmcpp_hip_rank_diagnostics (include/mcmcpp_hip.h) restated in numpy, for
tests/test_rank_diagnostics.py: the draws of the sequences, exact average ranks by sort and searchsorted, the normal score of
mcmcpp_amd/csrc/normal_score.hpp in float64 operations (each rounded on its own, as numpy's are), the order statistics in the
total order of the keys, and the diagnostics by composition of tests/rhat_restatement.py and tests/ess_restatement.py."""
import numpy as np

from mcmcpp_amd import capi
from tests import ess_restatement as er
from tests import rhat_restatement as rr

_LN2_HI, _LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
_LG = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01, 1.818357216161805012e-01,
       1.531383769920937332e-01, 1.479819860511658591e-01)
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4, 1.3731693765509461125e+4,
      1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4, 5.3941960214247511077e+3,
      6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0, 3.64784832476320460504e+0,
      5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1, 6.89767334985100004550e-1,
      1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2, 2.96560571828504891230e-1,
      1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4, 1.48753612908506148525e-2,
      1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def normal_score_log(x):
    """normal_score_log of the header: x a float64 array of positive normal numbers"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    k = (bits >> np.uint64(52)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > 1.41421356237309504880
    m = np.where(big, m * 0.5, m)
    dk = (k + big).astype(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * ((w * (w * _LG[5] + _LG[3])) + _LG[1])
    t2 = z * ((w * ((w * (w * _LG[6] + _LG[4])) + _LG[2])) + _LG[0])
    R = t2 + t1
    hfsq = (0.5 * f) * f
    return dk * _LN2_HI + (f - (hfsq - (s * (hfsq + R) + dk * _LN2_LO)))


def _poly(r, k):
    acc = k[0] * r + k[1]
    for c in k[2:]:
        acc = acc * r + c
    return acc


def normal_score(p):
    """normal_score of the header: p a float64 array in (0, 1)"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    q = p - 0.5
    central = np.abs(q) <= 0.425
    r = 0.180625 - q * q
    z_central = (q * _poly(r, _A)) / _poly(r, _B)
    t = np.where(central, 0.25, np.where(q < 0.0, p, 1.0 - p))  # (0.25: any normal number, where the tail is not taken)
    r = np.sqrt(-normal_score_log(t))
    near = r <= 5.0
    rn, rf = r - 1.6, r - 5.0
    z_tail = np.where(near, _poly(rn, _C) / _poly(rn, _D), _poly(rf, _E) / _poly(rf, _F))
    z_tail = np.where(q < 0.0, -z_tail, z_tail)
    return np.where(central, z_central, z_tail)


def score_of_rank(below, equal, S):
    r = below.astype(np.float64) + (equal.astype(np.float64) + 1.0) / 2.0
    return normal_score((r - 0.375) / (np.float64(S) + 0.25))


def draws(steps, split=True, slice_interval=1):
    """the steps that belong to a sequence, [K][H L][W][P] in the chain's type: a chain whose own halves are the sequences"""
    x = np.asarray(steps)
    if x.ndim == 3:
        x = x[None]
    x = x[:, ::slice_interval]
    n = x.shape[1]
    return np.ascontiguousarray(np.concatenate([x[:, a:a + L] for a, L in rr.halves(n, split)], axis=1))


def to_key(x):
    """the order-preserving unsigned keys of float32 / float64 values: -inf < ... < -0 < +0 < ... < +inf"""
    U = np.uint32 if x.dtype == np.float32 else np.uint64
    b = np.ascontiguousarray(x).view(U)
    sign = U(1) << U(8 * b.itemsize - 1)
    return np.where(b & sign, ~b, b ^ sign)


def quantiles_of(x):
    """(median, q05, q95) of the draws x [(S,)] of one parameter, float64, by capi.quantile_rule on the order statistics"""
    xs = x[np.argsort(to_key(x), kind="stable")]
    h, lo, hi = capi.quantile_ranks([0.5, 0.05, 0.95], x.size)
    with np.errstate(invalid="ignore"):  # (-inf + inf between an infinite and a finite order statistic is NaN, and is the answer)
        return capi.quantile_rule(xs[lo][None], xs[hi][None], h, "linear", np.float64)[0]


def average_ranks(v):
    """(below, equal) of every value among the values v [(S,)], compared as numbers"""
    sv = np.sort(v)
    below = np.searchsorted(sv, v, "left")
    return below, np.searchsorted(sv, v, "right") - below


def normal_scores(steps, split=True, fold=False, slice_interval=1):
    d = draws(steps, split, slice_interval)
    K, HL, W, P = d.shape
    if np.isnan(d).any():
        raise ValueError("a NaN draw has no place in the order")
    flat = d.reshape(-1, P)
    S = flat.shape[0]
    scores = np.empty((S, P))
    quant = np.empty((3, P))
    for p in range(P):
        x = np.ascontiguousarray(flat[:, p])
        quant[:, p] = quantiles_of(x)
        v = x.astype(np.float64)
        if fold:
            if not np.isfinite(quant[0, p]):
                raise ValueError("a fold about a median that is not finite has NaN values, which have no place in the order")
            v = np.abs(v - quant[0, p])
        below, equal = average_ranks(v)
        scores[:, p] = score_of_rank(below, equal, S)
    L = HL // 2 if split else HL
    return dict(scores=scores.reshape(K, HL, W, P), median=quant[0], q05=quant[1], q95=quant[2], sequence_length=L, num_sequences=S // L)


def indicators(steps, q, split=True, slice_interval=1):
    """the fp64 chain [K][H L][W][P] of 1.0 / 0.0 of x <= q[p], compared in double"""
    return (draws(steps, split, slice_interval).astype(np.float64) <= q).astype(np.float64)


def compose(ess_of, rhat_of, scores0, scores1, lower, upper, quant):
    """the diagnostics from the four chains: ess_of(chain) and rhat_of(chain) are the existing estimators' dicts"""
    bulk, low, up = ess_of(scores0), ess_of(lower), ess_of(upper)
    folded = rhat_of(scores1)["rhat"]
    a, b = bulk["rhat"], folded
    lo, hi = low["ess"], up["ess"]
    return dict(rhat=np.where(np.isnan(a) | np.isnan(b), np.nan, np.maximum(a, b)), rhat_rank=a, rhat_folded=b, ess_bulk=bulk["ess"],
                ess_tail=np.where(np.isnan(lo) | np.isnan(hi), np.nan, np.minimum(lo, hi)), ess_tail_lower=lo, ess_tail_upper=hi, median=quant["median"],
                q05=quant["q05"], q95=quant["q95"], closed_bulk=bulk["closed"], closed_tail=((low["closed"] != 0) & (up["closed"] != 0)).astype(np.int64),
                sequence_length=bulk["sequence_length"], num_sequences=bulk["num_sequences"])


def rank_diagnostics(steps, split=True, max_lag=0, slice_interval=1):
    s0 = normal_scores(steps, split, False, slice_interval)
    s1 = normal_scores(steps, split, True, slice_interval)
    with np.errstate(all="ignore"):
        return compose(lambda c: er.effective_sample_size(c, split, max_lag), lambda c: rr.gelman_rubin(c, split), s0["scores"], s1["scores"],
                       indicators(steps, s0["q05"], split, slice_interval), indicators(steps, s0["q95"], split, slice_interval), s0)
