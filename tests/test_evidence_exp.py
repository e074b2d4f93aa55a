"""mcmcpp::evidence_exp (mcmcpp_amd/csrc/evidence_exp.hpp): the exponential that turns u - max u into the weight of a draw in
the evidence ratios, one value in bits on device, host and in numpy.  All on the CPU.

tests/cpp/evidence_exp_cases.cpp compiles the header with the host compiler alone.  The numpy restatement of
tests/evidence_restatement.py returns the compiled header's bits on a grid and on random arguments in [-745, 0], at the edges
(0, -0.0, -inf, the flush point and its neighbours) and on both neighbours of every reduction boundary (where k changes:
x = (j - 0.5) ln 2): that is what ties the restatement the GPU tests compare with to the definition.  The values are compared
with the host libm's exp as well.

Measured: the largest difference from libm's exp is 1 ulp (MEASURED_ULPS, already a whole number), over every argument below
that is not flushed; the test fails above MAX_ULPS = 4 whatever was measured."""
import os
import subprocess

import numpy as np
import pytest

from tests import evidence_restatement as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
MEASURED_ULPS = 1  # the largest |evidence_exp - libm exp| seen on the arguments below, in ulps, rounded up to a whole ulp
MAX_ULPS = 4
LN2 = 0.6931471805599453


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "evidence_exp_cases")
    # the host compiler alone, and no include path but the headers' own directory: evidence_exp.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "evidence_exp_cases.cpp"), "-I", CSRC])
    return exe


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def run(exe, mode, values):
    values = np.ascontiguousarray(values, dtype=np.float64)
    out = subprocess.run([exe, mode], input=values.tobytes(), capture_output=True, check=True).stdout
    return np.frombuffer(out, np.float64)


def boundaries():
    """both neighbours of every reduction boundary, and the boundary's nearest double itself: k changes where x / ln 2 - 0.5 is
    an integer; a few doubles on either side cover the rounding of the product"""
    b = (np.arange(0, -1023, -1, dtype=np.float64) - 0.5) * LN2
    parts = [b]
    lo, hi = b, b
    for _ in range(3):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        parts += [lo, hi]
    return np.concatenate(parts)


def edges():
    f = np.float64(ev.FLUSH)
    return np.array([0.0, -0.0, -np.inf, f, np.nextafter(f, 0.0), np.nextafter(f, -np.inf), -708.0, -709.0, -745.0, -1e300, -5e-324, -1e-300, -2.0 ** -53, -2.0 ** -54])


def arguments():
    rng = np.random.default_rng(7)
    return np.concatenate([np.linspace(-745.0, 0.0, 200001), -rng.uniform(0.0, 745.0, 200000), -rng.exponential(2.0, 200000), -np.exp(-rng.uniform(0.0, 80.0, 20000)),
                           edges(), boundaries()])


def test_evidence_exp_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "evidence_exp.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<stdint.h>", "<string.h>"]
    body = text.split("#pragma once")[1]
    assert "fma" not in body and "exp(" not in body.replace("evidence_exp(", "") and "#pragma clang fp contract(off)" in body


def test_the_edges_are_exact(driver):
    f = np.float64(ev.FLUSH)
    got = run(driver, "exp", [0.0, -0.0, -np.inf, np.nextafter(f, -np.inf), -745.0, f])
    assert got[0] == 1.0 and got[1] == 1.0
    assert (got[2:5] == 0.0).all() and not np.signbit(got[2:5]).any()
    # the first argument that is not flushed gives a normal number: nothing between 0 and 2^-1022 is ever returned
    assert got[5] >= 2.0 ** -1022
    x = arguments()
    e = run(driver, "exp", x)
    assert ((e == 0.0) | (e >= 2.0 ** -1022)).all() and (e <= 1.0).all()
    assert ((e == 0.0) == (x < f)).all()
    assert np.isnan(run(driver, "exp", [np.nan]))[0]


def test_restatement_returns_the_headers_bits(driver):
    x = arguments()
    np.testing.assert_array_equal(ev.evidence_exp(x).view(np.uint64), run(driver, "exp", x).view(np.uint64))


def test_against_libm(driver):
    x = arguments()
    x = x[x >= ev.FLUSH]
    got, want = run(driver, "exp", x), run(driver, "libexp", x)
    d = np.abs(got.view(np.int64) - want.view(np.int64))
    worst = int(np.argmax(d))
    print("largest difference from libm's exp: %d ulp at x = %r" % (d[worst], x[worst]))
    assert d.max() <= MEASURED_ULPS <= MAX_ULPS
    # monotone along the grid: the reduction boundaries leave no step backwards
    grid = np.sort(x)
    assert (np.diff(run(driver, "exp", grid)) >= 0).all()
