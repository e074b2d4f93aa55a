"""mcmcpp::beta_quantile (mcmcpp_amd/csrc/beta_quantile.hpp, exported as mcmcpp_hip_beta_quantile) against a 50-digit inverse of
the regularised incomplete Beta function in mpmath.  CPU only: the function opens no device.

The bound is derived, not measured: a parameter has S <= 2^31 - 1 draws, so a relative error below 1e-10 < 1 / S = 4.7e-10
moves u S by less than one rank.  Largest relative error seen over the grid below: 3.4e-14 (p = 0.8413, prob = 0.001,
ess = 10^6); the mirrored call 1 - beta_quantile(1 - p, b, a) stayed within 1.3e-12 of the same reference.

The reference: mpmath.betainc(a, b, 0, x, regularized=True) at 50 digits, inverted by Newton's method from scipy's betaincinv.
mpmath sums a hypergeometric series for it, which it gives up on at a + b = 10^6 ("converges too slowly", after seconds);
above a + b = 10^4 the same regularised integral is therefore taken by mpmath's quadrature of the density at the same 50 digits,
over the 40 standard deviations below x (the mass further out is below 10^-300).  test_the_two_references_agree checks the
quadrature against the series where both work."""
import mpmath as mp
import numpy as np
import pytest
from scipy.special import betaincinv

from mcmcpp_amd import capi

P_TAILS = (0.15865525393145707, 0.8413447460685429)
PROBS = (0.001, 0.05, 0.5, 0.95, 0.999)
ESS = (0.5, 1.0, 7.3, 1.0e3, 1.0e6, 2.0 ** 31)
BOUND = 1e-10
SERIES_LIMIT = 1.0e4  # a + b up to which mpmath.betainc is the reference as it is


@pytest.fixture(scope="module", autouse=True)
def library():
    capi.build_library()


def _density(a, b, t, log_beta):
    return mp.exp((a - 1) * mp.log(t) + (b - 1) * mp.log1p(-t) - log_beta)


def reference_cdf(a, b, x):
    """I_x(a, b) at the working precision"""
    if a + b <= SERIES_LIMIT:
        return mp.betainc(a, b, 0, x, regularized=True)
    else:
        log_beta = mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)
        sigma = mp.sqrt(a * b / ((a + b) ** 2 * (a + b + 1)))
        start = max(mp.mpf(0), x - 40 * sigma)
        cuts = mp.linspace(start, x, 21)  # pieces of two standard deviations: the integrand is smooth on each
        return mp.quad(lambda t: _density(a, b, t, log_beta), cuts)


def reference_quantile(p, a, b):
    """the 50-digit x with I_x(a, b) = p (p, a, b the doubles the library gets)"""
    with mp.workdps(50):
        a, b, p = mp.mpf(a), mp.mpf(b), mp.mpf(p)
        log_beta = mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)
        x = mp.mpf(float(betaincinv(float(a), float(b), float(p))))
        for _ in range(8):
            step = (reference_cdf(a, b, x) - p) / _density(a, b, x, log_beta)
            x -= step
            if abs(step) < mp.mpf(10) ** -40 * x:
                break
        else:
            raise AssertionError("the reference did not converge")
        return x


def _rel(got, want):
    with mp.workdps(50):
        return float(abs(mp.mpf(got) - want) / want)


GRID = [(p, prob, ess) for p in P_TAILS for prob in PROBS for ess in ESS]


@pytest.fixture(scope="module")
def reference():
    return {(p, prob, ess): reference_quantile(p, ess * prob + 1.0, ess * (1.0 - prob) + 1.0) for p, prob, ess in GRID}


def test_relative_error_stays_below_the_rank_bound(reference):
    worst = (0.0, None)
    for key in GRID:
        p, prob, ess = key
        a, b = ess * prob + 1.0, ess * (1.0 - prob) + 1.0
        got = capi.beta_quantile(p, a, b)
        assert 0.0 < got < 1.0
        err = _rel(got, reference[key])
        worst = max(worst, (err, key))
        assert err < BOUND, (key, got, err)
    print("largest relative error %.3g at p, prob, ess = %s" % worst)


def test_the_two_references_agree(monkeypatch):
    """where the series still converges (ess = 1000), the quadrature gives the same 50-digit inverse to 40 digits"""
    for p in P_TAILS:
        for prob in (0.001, 0.5, 0.95):
            a, b = 1.0e3 * prob + 1.0, 1.0e3 * (1.0 - prob) + 1.0
            series = reference_quantile(p, a, b)
            monkeypatch.setattr("tests.test_beta_quantile.SERIES_LIMIT", 0.0)
            quadrature = reference_quantile(p, a, b)
            monkeypatch.undo()
            with mp.workdps(50):
                assert abs(series - quadrature) < mp.mpf(10) ** -38 * series, (p, prob)


def test_symmetry(reference):
    worst = 0.0
    for key in GRID:
        p, prob, ess = key
        a, b = ess * prob + 1.0, ess * (1.0 - prob) + 1.0
        mirrored = 1.0 - capi.beta_quantile(1.0 - p, b, a)
        err = _rel(mirrored, reference[key])  # (1 - p differs from the other tail by an ulp: 1e-16 of p)
        worst = max(worst, err)
        assert err < BOUND, (key, mirrored, err)
        assert abs(mirrored - capi.beta_quantile(p, a, b)) < BOUND * reference[key]
    print("largest relative error of the mirrored call %.3g" % worst)


@pytest.mark.parametrize("prob", PROBS)
@pytest.mark.parametrize("ess", ESS)
def test_monotone_in_p(prob, ess):
    a, b = ess * prob + 1.0, ess * (1.0 - prob) + 1.0
    ps = [1e-6, 0.001, 0.05, P_TAILS[0], 0.3, 0.5, 0.7, P_TAILS[1], 0.95, 0.999, 1 - 1e-6]
    xs = [capi.beta_quantile(p, a, b) for p in ps]
    assert all(0.0 < x < 1.0 for x in xs) and all(x0 < x1 for x0, x1 in zip(xs, xs[1:])), xs


def test_known_values_and_determinism():
    assert abs(capi.beta_quantile(0.5, 1.0, 1.0) - 0.5) < 1e-15            # uniform
    assert abs(capi.beta_quantile(0.25, 1.0, 1.0) - 0.25) < 1e-15
    assert abs(capi.beta_quantile(0.5, 3.0, 3.0) - 0.5) < 1e-15            # symmetric
    assert abs(capi.beta_quantile(0.36, 2.0, 1.0) - 0.6) < 1e-15           # I_x(2, 1) = x^2
    assert abs(capi.beta_quantile(0.19, 1.0, 2.0) - 0.1) < 1e-15           # I_x(1, 2) = 1 - (1 - x)^2
    a, b = 2.0 ** 31 + 2.0, 2.0 ** 31 + 2.0                                # the upper end of the range
    x = capi.beta_quantile(P_TAILS[1], a, b)
    assert x == capi.beta_quantile(P_TAILS[1], a, b)
    assert abs((x - 0.5) * 2.0 * np.sqrt(a + b + 1.0) - 1.0) < 1e-6         # one standard deviation above the mean
    for bad in ((0.0, 2.0, 2.0), (1.0, 2.0, 2.0), (0.5, 0.5, 2.0), (float("nan"), 2.0, 2.0)):
        with pytest.raises(ValueError):
            capi.beta_quantile(*bad)
