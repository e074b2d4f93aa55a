"""A numpy restatement of what mcmcpp_amd/csrc/quantiles.hip computes: the order-preserving integer keys, the most-significant-digit
radix select on them (parameterised by the digit schedule, so that it can be checked with other digit widths than the library's),
the rank counts and the three quantile rules.  No sorting in the select: only counts of digits, as on the device.  Used by
tests/test_quantiles.py, which first checks this file against np.sort."""
import numpy as np


def key_type(dtype):
    return np.uint32 if np.dtype(dtype) == np.float32 else np.uint64


def to_keys(x):
    """bit pattern with all bits flipped if the sign bit is set, else with the sign bit flipped: -inf < ... < -0 < +0 < ... < +inf"""
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.float64)
    U = key_type(x.dtype)
    b = x.view(U)
    sign = U(1) << U(8 * b.itemsize - 1)
    return np.where(b & sign, ~b, b ^ sign).astype(U)


def from_keys(k, dtype):
    k = np.ascontiguousarray(k)
    U = key_type(dtype)
    assert k.dtype == U
    sign = U(1) << U(8 * k.itemsize - 1)
    return np.where(k & sign, k ^ sign, ~k).astype(U).view(dtype)


def schedule(key_bits, digit_bits):
    """[(shift, bits)], most significant digit first; every key bit in exactly one digit"""
    out, top = [], key_bits
    while top > 0:
        bits = min(digit_bits, top)
        out.append((top - bits, bits))
        top -= bits
    return out


def select_key(keys, rank, sched):
    """the key of 0-based rank `rank` among `keys` (one parameter's samples), digit by digit; also the prefix after every pass"""
    U = keys.dtype.type
    key_bits = 8 * keys.itemsize
    assert 0 <= rank < keys.size
    prefix, rem, prefixes = 0, int(rank), []
    for shift, bits in sched:
        if shift + bits >= key_bits:
            mine = keys
        else:
            mine = keys[(keys >> U(shift + bits)) == U(prefix)]
        counts = np.bincount(((mine >> U(shift)) & U((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
        cum = np.cumsum(counts)
        d = int(np.searchsorted(cum, rem, side="right"))  # the digit whose cumulative count first exceeds the remaining rank
        assert d < (1 << bits)
        rem -= int(cum[d - 1]) if d else 0
        prefix = (prefix << bits) | d
        prefixes.append(prefix)
    return prefix, prefixes


def used_samples(steps, slice_interval=1):
    """[N][P]: every slice_interval-th step from the first, walkers in order"""
    steps = np.asarray(steps)
    return steps[::slice_interval].reshape(-1, steps.shape[-1])


def order_statistics(steps, ranks, slice_interval=1, digit_bits=8):
    """values[P][len(ranks)] by radix select"""
    x = used_samples(steps, slice_interval)
    U = key_type(x.dtype)
    sched = schedule(8 * np.dtype(U).itemsize, digit_bits)
    out = np.zeros((x.shape[1], len(ranks)), U)
    for p in range(x.shape[1]):
        keys = to_keys(x[:, p])
        cache = {}
        for k, r in enumerate(ranks):
            if int(r) not in cache:
                cache[int(r)] = select_key(keys, int(r), sched)[0]
            out[p, k] = cache[int(r)]
    return from_keys(out, x.dtype)


def group_counts(steps, ranks, slice_interval=1, digit_bits=8):
    """per pass, the most rank groups of a parameter: distinct prefixes among its ranks going INTO the pass (1 for the first)"""
    x = used_samples(steps, slice_interval)
    sched = schedule(8 * x.itemsize, digit_bits)
    most = [1] * len(sched)
    for p in range(x.shape[1]):
        keys = to_keys(x[:, p])
        prefixes = [select_key(keys, int(r), sched)[1] for r in set(int(r) for r in ranks)]
        for i in range(1, len(sched)):
            most[i] = max(most[i], len({pr[i - 1] for pr in prefixes}))
    return most


def sorted_by_key(column):
    """the column in the total order of the keys (so that -0 comes before +0)"""
    column = np.ascontiguousarray(column)
    return column[np.argsort(to_keys(column), kind="stable")]


def rank_counts(steps, query, slice_interval=1):
    """(below, not_above) [P][Q], compared as numbers"""
    x = used_samples(steps, slice_interval)
    query = np.asarray(query)
    below = np.array([[np.count_nonzero(x[:, p] < v) for v in query[p]] for p in range(x.shape[1])], np.int64).reshape(query.shape)
    not_above = np.array([[np.count_nonzero(x[:, p] <= v) for v in query[p]] for p in range(x.shape[1])], np.int64).reshape(query.shape)
    return below, not_above


def quantiles(steps, q, method="linear", slice_interval=1, digit_bits=8):
    """[P][len(q)]: h = q (N - 1) in float64; "lower" rank floor(h), "higher" rank ceil(h), "linear" x_lo + (x_hi - x_lo)(h - floor(h))
    in float64, rounded once to T"""
    x = used_samples(steps, slice_interval)
    T = x.dtype.type
    q = np.asarray(q, np.float64)
    h = q * np.float64(x.shape[0] - 1)
    lo, hi = np.floor(h).astype(np.int64), np.ceil(h).astype(np.int64)
    x_lo, x_hi = order_statistics(steps, lo, slice_interval, digit_bits), order_statistics(steps, hi, slice_interval, digit_bits)
    if method == "lower":
        return x_lo
    if method == "higher":
        return x_hi
    assert method == "linear"
    out = np.zeros(x_lo.shape, T)
    for p in range(out.shape[0]):
        for k in range(out.shape[1]):
            a, b = np.float64(x_lo[p, k]), np.float64(x_hi[p, k])
            out[p, k] = T(a) if x_lo[p, k] == x_hi[p, k] else T(a + (b - a) * (h[k] - np.floor(h[k])))
    return out
