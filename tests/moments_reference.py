"""Extended-precision reference for Analysis::CovarianceMatrix and the error bar tests/test_moments.py holds the device to.

exact_moments: the selected samples widened to np.longdouble (64-bit significand), their mean, and the two-pass
covariance ((x - m).T @ (x - m)) / N, rounded to fp64 at the end.  Two passes do not cancel, so its own error is about
2**-64 of |m_i m_j| + s_i s_j: 1/4096 of the unit the bar is stated in.

The bar, for every covariance element (i, j) and every mean element i:

    |cov  - exact| <= MARGIN * max(oracle_cov_err,  U * (|m_i m_j| + s_i s_j))
    |mean - exact| <= MARGIN * max(oracle_mean_err, U * |m_i|)

U = 2**-52; m, s: exact means and standard deviations; oracle_*_err: the largest element error of the oracle's fp64
restatement of the reference (po.chain_covariance) on the same input, measured against exact_moments.  MARGIN = 4: the
oracle and the device both form E[xy] - E[x]E[y] in fp64 and round the quotient, the product and the difference once
each, and the device's per-slot sums are short.  The margin stands over the reference's error, never over the device's.

fp32 chains: the device widens the samples (their products are exact in fp64), accumulates and finishes in fp64, and
narrows once when it writes the result.  So the same fp64 bar applies to the widened data (the oracle error is that of
the fp64 oracle on the widened data), seen through that one narrowing: a float result passes where it is the rounding
of some fp64 value inside the bar, float(exact - bar) <= result <= float(exact + bar) -- rounding is monotone."""
import numpy as np

from oracle import pyoracle as po

U = 2.0 ** -52
MARGIN = 4.0

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than fp64 here: exact_moments would not be a reference"


def _selected(steps, slice_interval):
    return steps[::slice_interval].reshape(-1, steps.shape[2])


def _moments_longdouble(steps, slice_interval):
    x = _selected(steps, slice_interval).astype(np.longdouble)
    mean = x.sum(axis=0) / x.shape[0]
    d = x - mean
    return mean, (d.T @ d) / x.shape[0]


def exact_moments(steps, slice_interval=1):
    """(mean[D], cov[D, D]) of every slice_interval-th step of steps[(n, W, D)], computed in np.longdouble, as fp64."""
    mean, cov = _moments_longdouble(steps, slice_interval)
    return mean.astype(np.float64), cov.astype(np.float64)


def holds(got, exact, bar):
    """elementwise: got is within bar of exact (a float32 result: it is the rounding of a value within the bar)"""
    if got.dtype == np.float32:
        return ((exact - bar).astype(np.float32) <= got) & (got <= (exact + bar).astype(np.float32))
    return np.abs(got - exact) <= bar


def ratio(got, exact, bar):
    """largest error / bar over the elements (what the docstrings record; `holds` is what is asserted).  For a
    float32 result half a float spacing is added to the bar, which is what the narrowing may cost."""
    bar = np.asarray(bar, np.float64) + np.zeros_like(exact)
    err = np.abs(got.astype(np.float64) - exact)
    if got.dtype == np.float32:
        bar = bar + 0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bar > 0, bar, np.finfo(np.float64).tiny))
    return float(r.max()) if r.size else 0.0


class Reference:
    """exact moments of one input, the oracle's results and errors on it, and the bars.  `keep` (bool[D], default all)
    names the parameters the scalar oracle errors are taken over: a test leaves out a parameter that holds a NaN."""

    def __init__(self, steps, slice_interval=1, keep=None):
        D = steps.shape[2]
        keep = np.ones(D, bool) if keep is None else np.asarray(keep, bool)
        self.keep = keep
        self.keep2 = np.outer(keep, keep)
        self.count = _selected(steps, slice_interval).shape[0]
        mean_ld, cov_ld = _moments_longdouble(steps, slice_interval)
        self.mean, self.cov = mean_ld.astype(np.float64), cov_ld.astype(np.float64)
        sd_ld = np.sqrt(np.diag(cov_ld))
        self.sd = sd_ld.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.corr = (cov_ld / np.outer(sd_ld, sd_ld)).astype(np.float64)
        # the oracle in fp64 on the (widened) input, and in the chain's own type
        self.oracle64 = po.chain_covariance(steps.astype(np.float64), slice_interval)
        self.oracle = self.oracle64 if steps.dtype == np.float64 else po.chain_covariance(steps, slice_interval)
        self.oracle_mean_err = float(np.abs(self.oracle64[0] - self.mean)[keep].max())
        self.oracle_cov_err = float(np.abs(self.oracle64[1] - self.cov)[self.keep2].max())
        self.cov_unit = U * (np.abs(np.outer(self.mean, self.mean)) + np.outer(self.sd, self.sd))
        self.mean_unit = U * np.abs(self.mean)
        self.cov_bar = MARGIN * np.maximum(self.oracle_cov_err, self.cov_unit)
        self.mean_bar = MARGIN * np.maximum(self.oracle_mean_err, self.mean_unit)
        # correlation r_ij = c_ij / (s_i s_j): to first order its error is that of c_ij over s_i s_j plus |r_ij| <= 1
        # times half the relative errors of the two variances, plus the roundings of two square roots and two quotients
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.diag(self.cov_bar) / np.diag(self.cov)
            self.corr_bar = self.cov_bar / np.outer(self.sd, self.sd) + 0.5 * (rel[:, None] + rel[None, :]) + MARGIN * U

    def check(self, mean, cov, label, where=None):
        """asserts the bar on the mean and on the covariance (where: bool[D] of the parameters to hold to it; default
        self.keep); prints and returns the ratios (mean, cov)"""
        k = self.keep if where is None else np.asarray(where, bool)
        k2 = np.outer(k, k)
        rm = ratio(mean[k], self.mean[k], self.mean_bar[k])
        rc = ratio(cov[k2], self.cov[k2], self.cov_bar[k2])
        print("moments bar %-40s mean %.3f  cov %.3f  (oracle err: mean %.2e cov %.2e; oracle/bar: mean %.3f cov %.3f)"
              % (label, rm, rc, self.oracle_mean_err, self.oracle_cov_err,
                 ratio(self.oracle64[0][k], self.mean[k], self.mean_bar[k]), ratio(self.oracle64[1][k2], self.cov[k2], self.cov_bar[k2])))
        assert np.all(holds(mean[k], self.mean[k], self.mean_bar[k])), "%s: mean error / bar = %.3f" % (label, rm)
        assert np.all(holds(cov[k2], self.cov[k2], self.cov_bar[k2])), "%s: covariance error / bar = %.3f" % (label, rc)
        return rm, rc
