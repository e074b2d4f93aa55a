"""mcmcpp::normal_score (mcmcpp_amd/csrc/normal_score.hpp): the inverse normal CDF that turns an average rank into a normal
score, one value in bits on device, host and in numpy.  All on the CPU.

tests/cpp/normal_score_cases.cpp compiles the header with the host compiler alone.  Its values are compared with
statistics.NormalDist().inv_cdf (the same algorithm, AS 241, with the host libm's log) on the probabilities of ranks and on
equally spaced ones; antisymmetry and strict monotonicity over ranks are exact; the logarithm is compared with libm's; and the
numpy restatement of tests/rank_restatement.py returns the compiled header's bits on the same grid: that is what ties the
restatement the GPU tests compare with to the definition.

Measured: the largest difference from the stdlib is MEASURED_ULPS ulp, in the tail branch, where the two
logarithms differ by an ulp before the square root and the rational function; the central branch uses no logarithm and agrees
bit for bit.  The test allows twice that: the stdlib's log is the host libm's and may move by an ulp between glibc versions."""
import os
import statistics
import subprocess

import numpy as np
import pytest

from tests import rank_restatement as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
MEASURED_ULPS = 4   # the largest |header - stdlib| seen on the grid below, in ulps of the stdlib's value
MEASURED_LOG_ULPS = 1  # the largest |normal_score_log - libm log|
SIZES = (2, 3, 64, 10 ** 4, 2 ** 31 - 1)


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "normal_score_cases")
    # the host compiler alone, and no include path but the headers' own directory: normal_score.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "normal_score_cases.cpp"), "-I", CSRC])
    return exe


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def run(exe, mode, values):
    values = np.ascontiguousarray(values, dtype=np.float64)
    out = subprocess.run([exe, mode], input=values.tobytes(), capture_output=True, check=True).stdout
    return np.frombuffer(out, np.float64)


def rank_probabilities(S):
    """p = (r - 0.375) / (S + 0.25) at the half-integer ranks r around both ends, both branch boundaries and the middle"""
    around = [1.0, S, (S + 1) / 2.0, 0.075 * (S + 0.25) + 0.375, 0.925 * (S + 0.25) + 0.375]
    twice = set()
    for c in around:
        for d in range(-6, 7):
            t = int(round(2 * c)) + d
            if 2 <= t <= 2 * S:
                twice.add(t)
    r = np.array(sorted(twice), dtype=np.float64) / 2.0
    return (r - 0.375) / (np.float64(S) + 0.25)


def grid():
    parts = [rank_probabilities(S) for S in SIZES]
    parts.append((np.arange(1, 10 ** 5 + 1, dtype=np.float64)) / np.float64(10 ** 5 + 1))  # equally spaced
    # AS 241's variable r = sqrt(-log p) reaches 5 at p = exp(-25) = 1.4e-11, below the smallest rank probability
    # (0.625 / 2^31 = 2.9e-10): the far branch is exercised on its own
    far = np.exp(-np.linspace(24.0, 700.0, 400))
    parts += [far, 1.0 - far[far > 1e-16]]
    return np.concatenate(parts)


def ulps_apart(a, b):
    """|a - b| in ulps of b (a, b of one sign or zero)"""
    ia, ib = a.view(np.int64), b.view(np.int64)
    same = np.signbit(a) == np.signbit(b)
    assert (same | ((a == 0) & (b == 0))).all()
    return np.abs(ia - ib) * same


def test_normal_score_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "normal_score.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<stdint.h>", "<string.h>"]
    assert "fma" not in text.split("#pragma once")[1]


def test_against_the_stdlib(driver):
    p = grid()
    assert ((p > 0) & (p < 1)).all()
    got = run(driver, "score", p)
    inv = statistics.NormalDist().inv_cdf
    want = np.array([inv(float(v)) for v in p])
    d = ulps_apart(got, want)
    central = np.abs(p - 0.5) <= 0.425
    worst = int(np.argmax(d))
    print("largest difference from the stdlib: %d ulp at p = %r (central branch: %d ulp)" % (d[worst], p[worst], d[central].max()))
    assert d[central].max() == 0  # no logarithm there: the same operations in the same order
    assert d.max() <= 2 * MEASURED_ULPS


def test_antisymmetry_and_monotonicity_are_exact(driver):
    S = 10 ** 4
    r = np.arange(2, 2 * S + 1, dtype=np.float64) / 2.0  # every average rank 1, 1.5, ..., S
    p = (r - 0.375) / (S + 0.25)
    z = run(driver, "score", p)
    assert (np.diff(z) > 0).all()
    assert (np.diff(z[::2]) > 0).all()  # the consecutive integer ranks
    # z(p) = -z(1 - p) wherever 1 - p is exact
    allp = grid()
    exact = (1.0 - (1.0 - allp)) == allp
    assert exact.sum() > 1000
    a, b = run(driver, "score", allp[exact]), run(driver, "score", 1.0 - allp[exact])
    np.testing.assert_array_equal(a, -b)
    # all draws equal: r = (S + 1) / 2 gives p = 0.5 and z = +0
    for S in SIZES:
        z0 = run(driver, "rank", [0, S, S])
        assert z0[0] == 0.0 and not np.signbit(z0[0])


def test_logarithm_against_libm(driver):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(0.0, 1.0, 200000), np.exp(-rng.uniform(0.0, 700.0, 200000)), [0.5, 1.0, 0.625 / 2 ** 31, np.sqrt(0.5), np.sqrt(2.0)]])
    x = x[(x > 2.3e-308)]
    got, want = run(driver, "log", x), run(driver, "liblog", x)
    d = ulps_apart(got, want)
    print("largest difference of normal_score_log from libm: %d ulp" % d.max())
    assert d.max() <= 2 * MEASURED_LOG_ULPS
    np.testing.assert_array_equal(rk.normal_score_log(x), got)


def test_restatement_returns_the_headers_bits(driver):
    p = grid()
    np.testing.assert_array_equal(rk.normal_score(p).view(np.uint64), run(driver, "score", p).view(np.uint64))
    S = 2 ** 31 - 1
    below = np.array([0, 0, 5, S - 1, S // 2, 17], dtype=np.int64)
    equal = np.array([1, S, 2, 1, 3, S - 17], dtype=np.int64)
    got = run(driver, "rank", np.stack([below, equal, np.full(6, S)], axis=1).astype(np.float64).ravel())
    np.testing.assert_array_equal(rk.score_of_rank(below, equal, S).view(np.uint64), got.view(np.uint64))
