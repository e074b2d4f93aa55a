"""What summary.hip decides on the host: the plan of mcmcpp_amd/csrc/summary_plan.hpp, checked on the CPU.

tests/cpp/summary_plan_cases.cpp is compiled with the host compiler against summary_plan.hpp and beta_quantile.hpp alone (no HIP
header: that it compiles is an assertion), and a second time as a stand-alone program with the address and undefined-behaviour
sanitizers, which then runs the same commands.  Every window start of the highest-density interval belongs to exactly one block
of the reduction, the grids stay within the launch limits, the argument checks hold at both ends of m, and the host arithmetic
is the restatement's."""
import math
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import summary_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SPAN = 2048  # window starts of a block of the reduction (test_limits pins it)
WINDOWS = (1, 63, 64, 2047, 2048, 2049, 3 * 2048 + 17, 10 ** 6 + 3, 2 ** 31 - 2)


def build_driver(sanitized=False):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "summary_plan_cases" + ("_san" if sanitized else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O1"]
    # the host compiler alone, and no include path but the headers' own directory: the plan must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "summary_plan_cases.cpp"), "-I", CSRC])
    return exe


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def driver(request):
    return build_driver(request.param == "sanitized")


def _run(exe, what, **args):
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout


def test_the_plan_headers_include_no_hip_header():
    for name, own in (("summary_plan.hpp", ['"beta_quantile.hpp"', '"rank_plan.hpp"']), ("beta_quantile.hpp", [])):
        text = open(os.path.join(CSRC, name)).read()
        includes = [line.split()[1] for line in text.split("\n") if line.startswith("#include")]
        assert [i for i in includes if i.startswith('"')] == own and "hip" not in " ".join(includes), name
    assert [line.split()[1] for line in open(os.path.join(CSRC, "beta_quantile.hpp")).read().split("\n") if line.startswith("#include")] == ["<cmath>"]


def test_limits(driver):
    p = dict(f.split("=") for f in _run(driver, "limits").split())
    assert int(p["max_probs"]) == 16 and int(p["threads"]) == 256 and int(p["span"]) == SPAN and int(p["xmax"]) == 2 ** 31 - 1 and int(p["ymax"]) == 65535
    assert float(p["lower"]) == sr.LOWER_TAIL and float(p["upper"]) == sr.UPPER_TAIL and abs(float(p["lower"]) + float(p["upper"]) - 1.0) < 1e-16
    assert int(p["cf_cap"]) == 10 ** 6 and int(p["newton_cap"]) == 200


@pytest.mark.parametrize("windows", WINDOWS)
def test_every_window_start_belongs_to_one_block(driver, windows):
    # the driver walks every block: each span begins where the one before ended, holds 1 .. SPAN starts, and they end at `windows`
    word, blocks, covered, beyond, fits = _run(driver, "hdi", windows=windows, tile=1024).split()
    assert word == "ok" and int(blocks) == -(-windows // SPAN) and int(covered) == windows and int(beyond) == 0 and fits == "1"
    assert int(blocks) <= 2 ** 31 - 1
    if windows <= 10 ** 6 + 3:
        spans = np.array([[int(v) for v in line.split()] for line in _run(driver, "spans", windows=windows).strip().split("\n")])
        assert (spans[:, 0] == np.arange(len(spans)) * SPAN).all() and (spans[:-1, 1] == SPAN).all() and spans[:, 1].sum() == windows
        assert spans[-1, 0] + spans[-1, 1] == windows and 1 <= spans[-1, 1] <= SPAN


def test_a_tile_past_the_grid_limit_does_not_fit(driver):
    assert _run(driver, "hdi", windows=2048, tile=65535).split()[4] == "1" and _run(driver, "hdi", windows=2048, tile=65536).split()[4] == "0"


def _check(exe, S, hdi, probs="0.5", **more):
    p, h, m = _run(exe, "check", S=S, hdi=repr(hdi), probs=probs, **more).split("\n")[:3]
    return p, h, int(m)


@pytest.mark.parametrize("S", (2, 24, 2047, 2048, 2049, 51200, 2 ** 31 - 1))
def test_hdi_check_at_both_ends_of_m(driver, S):
    for m in (1, S - 1):
        p, h, got = _check(driver, S, (m + 0.5) / S)
        assert (p, h, got) == ("-", "-", m), (S, m)
    assert _check(driver, S, 0.5 / S)[1].startswith("1 <= floor(hdi_prob S) <= S - 1") and _check(driver, S, 0.5 / S)[2] == 0   # m = 0
    p, h, m = _check(driver, S, math.nextafter(1.0, 0.0))                                                                       # m = S - 1 still
    assert h == "-" and m == S - 1
    assert _check(driver, S, 0.0)[1] == "-"
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert "0 < hdi_prob < 1" in _check(driver, S, bad)[1], bad


def test_probability_checks(driver):
    assert _check(driver, 100, 0.5, "0.001,0.5,0.999")[0] == "-"
    assert _check(driver, 100, 0.5, ",".join(["0.5"] * 16))[0] == "-"
    assert "n_probs" in _check(driver, 100, 0.5, ",".join(["0.5"] * 17))[0]
    assert "n_probs" in _check(driver, 100, 0.5, "0.5", n_probs=-1)[0]
    assert _check(driver, 100, 0.5, "", n_probs=0, null=1)[0] == "-"
    assert "NULL" in _check(driver, 100, 0.5, "0.5", null=1)[0]
    for bad in ("0", "1", "nan", "-0.5", "1.5", "inf"):
        assert "probs[1]" in _check(driver, 100, 0.5, "0.5," + bad)[0], bad


def test_ranks_and_arithmetic_are_the_restatements(driver):
    capi.build_library()
    for ess, prob, S in ((0.0, 0.5, 1000), (51234.5, 0.05, 51200), (812.25, 0.95, 51200), (1e9, 0.0001, 1000), (1e9, 0.9999, 1000), (3.0, 0.5, 2), (2.0 ** 31, 0.5, 2 ** 31 - 1)):
        lo, hi = (int(v) for v in _run(driver, "ranks", ess=repr(ess), prob=repr(prob), S=S).split())
        assert (lo, hi) == sr.mcse_ranks(ess, prob, S) and 0 <= lo <= hi <= S - 1, (ess, prob, S)
    assert _run(driver, "ranks", ess="nan", prob="0.5", S=100).split() == ["-1", "-1"]
    # the driver's beta_quantile is the library's (one header); the same bits where the libm is the same
    for p, a, b in ((sr.LOWER_TAIL, 1.5, 1.5), (sr.UPPER_TAIL, 2562.7, 48673.3), (0.5, 2.0 ** 31 + 2, 1.0)):
        got = float(_run(driver, "beta", p=repr(p), a=repr(a), b=repr(b)))
        assert abs(got - capi.beta_quantile(p, a, b)) <= 1e-13 * got
    for L, M, within, between, over in ((200, 256, 0.98, 0.004, 51199), (2, 2, 0.5, 0.25, 4), (2 ** 20, 2047, 1.5, 1e-7, 2 ** 20 * 2047 - 1)):
        bits = int(_run(driver, "pooled", L=L, M=M, within=repr(within), between=repr(between), over=over))
        assert bits == int(np.float64(sr.pooled(L, M, np.float64(within), np.float64(between), over)).view(np.uint64))
