"""A numpy restatement of the reference's CornerHistograms / PercentileAndMaximumFinder (MCMCpp/Analysis/), exact:
every operation in the chain's element type and in the reference's order, int() truncation, numpy bincount counting.
Where the reference is undefined (a bin outside [0, bins), an index past its cumulative-sum array, a bisection that
never ends) it does what the library and the facade headers do, so it checks them on any input:
  * a bin outside [0, bins) is clamped into bin 0 or bins - 1 and counted per parameter;
  * getPercentileFromValue reads the cumulative sums at a flat index (the reference does not offset by the parameter);
    an index past the end of the array is clamped to its last cell;
  * getValueFromPercentile's bisection stops where the reference's would repeat itself forever: first + 1 == last with
    the cell at `first` below the count (it then uses `last`).
Only this module's conversions to int follow x86's cvttsd2si (INT_MIN outside the int range): that is what the reference
does on the machines the fixtures come from."""
import numpy as np

INT_MIN = -(2 ** 31)


def _t(dtype):
    return np.float32 if np.dtype(dtype) == np.float32 else np.float64


def to_int(v):
    """static_cast<int>(v) as compiled for x86-64 (truncation; INT_MIN for NaN and out-of-range values)"""
    v = float(v)
    if not (-2147483649.0 < v < 2147483648.0):
        return INT_MIN
    return int(v)


def _sign(v, T):
    return int(T(0) < v) - int(v < T(0))


def select_steps(steps, slice_interval=1):
    """the steps the reference's loops use: every slice_interval-th from the first"""
    return steps[::slice_interval]


def find_binning(used, bins):
    """findBinning: used[(n, W, P)] of T -> bounds[(P, 2)] = (low edge, bin width) in T"""
    T = _t(used.dtype)
    P = used.shape[-1]
    x = used.reshape(-1, P)
    assert not np.isnan(x).any(), "NaN samples"
    lo = np.full(P, np.finfo(T).max, T)
    hi = np.full(P, np.finfo(T).tiny, T)  # numeric_limits<T>::min(): the smallest positive normal
    if x.shape[0]:
        lo = np.minimum(lo, x.min(axis=0))
        hi = np.maximum(hi, x.max(axis=0))
    expand, contract, min_size = T(1.001), T(0.999), T(0.001)
    out = np.zeros((P, 2), T)
    for p in range(P):
        l, h = T(lo[p]), T(hi[p])
        if l == h:
            if l != T(0):
                if _sign(l, T) == 1:
                    l, h = T(l * contract), T(h * expand)
                else:
                    l, h = T(l * expand), T(h * contract)
            else:
                l, h = -min_size, min_size
        else:
            s = _sign(l, T)
            l = T(l * expand) if s == -1 else (-min_size if s == 0 else T(l * contract))
            s = _sign(h, T)
            h = T(h * expand) if s == -1 else (min_size if s == 0 else T(h * contract))
        out[p, 0] = l
        out[p, 1] = T(T(h - l) / T(bins))
    return out


def bin_indices(used, bounds, bins):
    """bin of every (sample, parameter) and the per-parameter count of clamped samples"""
    T = _t(used.dtype)
    P = used.shape[-1]
    x = used.reshape(-1, P)
    with np.errstate(all="ignore"):
        q = ((x - bounds[:, 0].astype(T)) / bounds[:, 1].astype(T)).astype(T)
    qd = q.astype(np.float64)
    high = qd >= bins
    low = ~(qd > -1.0)
    ok = ~(high | low)
    b = np.where(ok, qd, 0.0).astype(np.int64)  # truncation toward zero
    b[high] = bins - 1
    b[low] = 0
    return b, (high | low).sum(axis=0).astype(np.int64)


def histograms(steps, bins, slice_interval=1, with_pairs=True):
    """-> dict(num_points, bounds[(P, 2)], single[(P, bins)], pairs[(P(P-1)/2, bins, bins)] or None, clamped[P])"""
    used = select_steps(steps, slice_interval)
    P = steps.shape[-1]
    bounds = find_binning(used, bins)
    b, clamped = bin_indices(used, bounds, bins)
    single = np.stack([np.bincount(b[:, p], minlength=bins) for p in range(P)]).astype(np.int64)
    pairs = None
    if with_pairs:
        b2 = bins * bins
        pairs = np.zeros((P * (P - 1) // 2, bins, bins), np.int64)
        for i in range(1, P):
            # pairs (i, 0) .. (i, i - 1) lie side by side: one count over cell numbers j * bins^2 + bin_i * bins + bin_j
            cells = b[:, i:i + 1] * bins + b[:, :i] + np.arange(i, dtype=np.int64) * b2
            pairs[i * (i - 1) // 2:i * (i + 1) // 2] = np.bincount(cells.ravel(), minlength=i * b2).reshape(i, bins, bins)
    return dict(num_points=b.shape[0], bounds=bounds, single=single, pairs=pairs, clamped=clamped)


# ---- PercentileAndMaximumFinder queries (host arithmetic in T) ----

def cum_sums(single):
    """[P][bins + 1], cell 0 = 0"""
    P, bins = single.shape
    cs = np.zeros((P, bins + 1), np.int64)
    cs[:, 1:] = np.cumsum(single, axis=1)
    return cs


def percentile_from_value(bounds, cs, num_points, p, val, binned=True):
    T = bounds.dtype.type
    P, cb = cs.shape
    bins = cb - 1
    lo, w = T(bounds[p, 0]), T(bounds[p, 1])
    val = T(val)
    if (not binned) or val < lo or val > T(lo + T(w * T(bins + 1))):
        return T(-1)
    bin_num = to_int(T(T(val - lo) / w))
    c = bin_num + 1
    flat = cs.reshape(-1)
    last = flat.size - 1
    x1 = T(T(T(c - 1) * w) + lo)
    x2 = T(T(T(c) * w) + lo)
    y1 = T(flat[min(max(c - 1, 0), last)])
    y2 = T(flat[min(max(c, 0), last)])
    with np.errstate(all="ignore"):
        m = T(T(y2 - y1) / T(x2 - x1))
        b = T(T(T(x2 * y1) - T(x1 * y2)) / T(x2 - x1))
        entries = T(to_int(T(T(val * m) + b)))
        return T(T(100) * T(entries / T(num_points)))


def value_from_percentile(bounds, cs, num_points, p, per, binned=True, report=False):
    """report=True: (value, whether the reference's bisection would never have ended)"""
    T = bounds.dtype.type
    stalled = False
    lo, w = T(bounds[p, 0]), T(bounds[p, 1])
    per = T(per)
    if (not binned) or T(0) > per or T(100) < per:
        v = T(np.float64(lo) - 1e4)
        return (v, False) if report else v
    entries = to_int(T(T(per / T(100)) * T(num_points)))
    c = cs[p]
    first, last = 0, c.size - 1
    if entries == 0:
        first = last = 1
    else:
        while first != last:
            mid = (first + last) // 2
            if c[mid] >= entries:
                if c[mid - 1] <= entries:
                    first = last = mid
                else:
                    last = mid
            else:
                if mid == first:  # the reference repeats this step forever
                    first = last
                    stalled = True
                else:
                    first = mid
    with np.errstate(all="ignore"):
        x1, x2 = T(c[last - 1]), T(c[last])
        y1 = T(T(T(last - 1) * w) + lo)
        y2 = T(T(T(last) * w) + lo)
        m = T(T(y2 - y1) / T(x2 - x1))
        b = T(T(T(x2 * y1) - T(x1 * y2)) / T(x2 - x1))
        v = T(T(T(entries) * m) + b)
    return (v, stalled) if report else v


def value_of_peak(bounds, single, p, binned=True):
    T = bounds.dtype.type
    lo, w = bounds[p, 0], bounds[p, 1]
    if not binned:
        return T(np.float64(lo) - 1e4)
    k = int(np.argmax(single[p]))  # the first maximal bin
    return T((np.float64(k + 0.5) * np.float64(w)) + np.float64(lo))


# ---- CSV files (default ostream formatting: %g) ----

def _g(v):
    return "%g" % float(v)


def _axis(bounds, p, bins):
    T = bounds.dtype.type
    lo, w = T(bounds[p, 0]), T(bounds[p, 1])
    return lo, T(lo + T(T(bins) * w))


HEAD = "# Lines starting with a '#' in the first column are ignored\n"
XAX = "# X-axis: nbins, first bin low edge, last bin high edge\n"


def corner_csv(bounds, single, pairs):
    """{file suffix: text} of CornerHistograms::saveHistsCsvFormat (suffix appended to the file name base)"""
    P, bins = single.shape
    files = {}
    for i in range(P):
        lo, hi = _axis(bounds, i, bins)
        rows = "".join("%d, %d\n" % (k, single[i, k]) for k in range(bins))
        files["_p%d.csv" % i] = HEAD + XAX + "%d, %s, %s\n" % (bins, _g(lo), _g(hi)) + "# bin number, value\n" + rows
        for j in range(i):
            li, hi_i = _axis(bounds, i, bins)
            lj, hj = _axis(bounds, j, bins)
            h = pairs[i * (i - 1) // 2 + j]
            rows = "".join("%d, %d, %d\n" % (a, c, h[a, c]) for a in range(bins) for c in range(bins))
            files["_p%d_p%d.csv" % (i, j)] = (HEAD + XAX + "%d, %s, %s\n" % (bins, _g(li), _g(hi_i)) +
                                              "# Y-axis: nbins, first bin low edge, last bin high edge\n" +
                                              "%d, %s, %s\n" % (bins, _g(lj), _g(hj)) + "# x-bin number, y-bin number, value\n" + rows)
    return files


def percentile_csv(bounds, single):
    """{file suffix: text} of PercentileAndMaximumFinder::writeHistogramsInCsvFormat"""
    T = bounds.dtype.type
    P, bins = single.shape
    cs = cum_sums(single)
    files = {}
    for i in range(P):
        lo, hi = _axis(bounds, i, bins)
        rows = "".join("%d, %d\n" % (k, single[i, k]) for k in range(bins))
        files["_p%d.csv" % i] = HEAD + XAX + "%d, %s, %s\n" % (bins, _g(lo), _g(hi)) + "# bin number, value\n" + rows
        rows = "".join("%d, %d\n" % (k, cs[i, k]) for k in range(bins + 1))
        low = T(T(bounds[i, 0]) - T(bounds[i, 1]))
        files["_cs_p%d.csv" % i] = HEAD + XAX + "%d, %s, %s\n" % (bins + 1, _g(low), _g(hi)) + "# bin number, value\n" + rows
    return files
