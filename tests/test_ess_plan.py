"""How the effective-sample-size kernels are launched and what the host makes of their sums: the plan of
mcmcpp_amd/csrc/ess_plan.hpp, checked on the CPU.

tests/cpp/ess_plan_cases.cpp is compiled with the host compiler against the plan header alone (no HIP header: that it compiles
is an assertion) and prints plans.  Every product e_s e_(s+t) of every lag is taken in exactly one step of one lag block, with
a bounds check wherever one is needed; the rounds cover the lags needed once, in whole blocks, within the two knobs; and the
host's part (gamma, rho, the window walk, tau) equals the restatement (tests/ess_restatement.py) bit for bit."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import ess_restatement as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
B = 32  # lags of a lag block (kEssLagBlock; test_limits pins it)
KNOBS = ("MCMCPP_HIP_ESS_FIRST_LAGS", "MCMCPP_HIP_ESS_WORK_MB")


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "ess_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: ess_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ess_plan_cases.cpp"), "-I", CSRC])
    return exe


def _run(exe, what, env=None, **args):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env or {})
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True, env=e).stdout


def _fields(line):
    return {k: int(v) for k, v in (f.split("=") for f in line.split())}


def rounds_of(exe, first_lags=None, work_mb=None, **args):
    """[(first lag, lags, blocks, grid x, y, z)] of the rounds the host loop takes"""
    env = {}
    if first_lags is not None:
        env[KNOBS[0]] = str(first_lags)
    if work_mb is not None:
        env[KNOBS[1]] = str(work_mb)
    return [tuple(int(v) for v in line.split()) for line in _run(exe, "rounds", env, **args).strip().split("\n")]


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def test_ess_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "ess_plan.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<cmath>", "<cstddef>", "<cstdlib>", '"rhat_plan.hpp"']


def test_the_ess_source_holds_no_threshold_of_its_own():
    text = open(os.path.join(CSRC, "ess.hip")).read()
    for gone in ("1024", "65535", "/ 32", "* 32", "% 32", "atomicAdd", "multiProcessorCount", "getenv", "fma("):
        assert gone not in text, gone
    for used in ('#include "ess_plan.hpp"', '#include "rhat_state.hpp"', '#include "analysis_host.hpp"', "rhat_sequences_state(", "rhat_check_request(", "ess_block_walk(",
                 "ess_round_lags(", "ess_lag_grid(", "ess_walk_window(", "ess_tau(", "ess_knobs_from_env(", "rhat_sum_plan(", "ANALYSIS_TRY(", "mcmcpp::Stream", "mcmcpp::DeviceBuffer"):
        assert used in text, used
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " ess_plan.hpp " in makefile.split("HDRS")[1].split("\n")[0] and " rhat_state.hpp " in makefile.split("HDRS")[1].split("\n")[0]
    assert " ess.o " in makefile.split("OBJS")[1].split("\n")[0] and "-ffp-contract=off" in makefile


def test_limits(driver):
    lim = _fields(_run(driver, "limits").strip())
    assert lim["lag_block"] == B and lim["lag_block"] % lim["rows_in_flight"] == 0 and lim["vector"] == 1
    assert lim["wave"] == 64 and lim["threads"] == lim["wave"] * lim["blocks_per_group"] == 256
    assert lim["first_lags"] == 64 and lim["work_mb"] == 1024
    assert lim["max_round_blocks"] == lim["grid_y"] * lim["blocks_per_group"]


@pytest.mark.parametrize("L,max_lag,nf,want", [
    (2, 0, 0, dict(cap=1, kmax=0, function_lags=0, needed=2, blocks=1)),
    (3, 0, 9, dict(cap=2, kmax=0, function_lags=3, needed=3, blocks=1)),
    (32, 0, 32, dict(cap=31, kmax=15, function_lags=32, needed=32, blocks=1)),
    (33, 0, 33, dict(cap=32, kmax=15, function_lags=33, needed=33, blocks=2)),
    (34, 0, 0, dict(cap=33, kmax=16, function_lags=0, needed=34, blocks=2)),
    (500, 64, 0, dict(cap=64, kmax=31, function_lags=0, needed=64, blocks=2)),
    (500, 1, 5, dict(cap=1, kmax=0, function_lags=2, needed=2, blocks=1)),
    (500, 10 ** 6, 0, dict(cap=499, kmax=249, function_lags=0, needed=500, blocks=16)),
    (2 ** 40, 0, 0, dict(cap=2 ** 40 - 1, kmax=2 ** 39 - 1, function_lags=0, needed=2 ** 40, blocks=2 ** 35)),
])
def test_window_shape(driver, L, max_lag, nf, want):
    got = _fields(_run(driver, "window", L=L, max_lag=max_lag, n_functions=nf).strip())
    assert got == want
    assert (got["cap"], got["kmax"]) == er.window_shape(L, max_lag)


@pytest.mark.parametrize("L", [2, 3, 31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97, 100, 129, 500, 1000])
def test_every_product_in_one_step_of_one_block(driver, L):
    t0s = list(range(0, -(-L // B) * B, B))
    rows = [tuple(int(v) for v in line.split()) for line in _run(driver, "walk", L=L, t0=",".join(map(str, t0s))).strip().split("\n")]
    assert [r[0] for r in rows] == t0s
    for t0, lead_end, full_end in rows:
        assert lead_end == max(L - t0, 0) and full_end % B == 0 and 0 <= full_end <= max(lead_end, 0) + B
        # a group without bounds checks reads rows up to s0 + B - 1 + t0 + B - 1, all of them inside the sequence
        for s0 in range(0, full_end, B):
            assert s0 + 2 * (B - 1) + t0 <= L - 1
        # and the first group with checks is the first that needs them
        assert full_end + 2 * (B - 1) + t0 > L - 1
        # the tail covers the rest: every s < lead_end, in groups that may run past it (the checks stop them)
        assert full_end <= lead_end or lead_end == 0 or full_end - lead_end < B
    # so: lag t = t0 + j gets the products of s in [0, L - t): the groups give s < full_end unchecked, the tail s < lead_end with s + t < L
    for t0, lead_end, full_end in rows:
        for j in (0, 1, B - 1):
            t = t0 + j
            steps = [s for s in range(0, full_end)] + [s for s in range(full_end, max(lead_end, full_end)) if s + t < L]
            assert steps == list(range(0, max(L - t, 0))) or full_end > L - t, (L, t0, j)
            assert all(s + t <= L - 1 for s in range(0, full_end))


@pytest.mark.parametrize("L,max_lag,nf,series,decided,first,mb,want", [
    (500, 0, 0, 1048576, 0, None, None, [(0, 64)]),                              # the windows closed in the first round
    (500, 0, 0, 1048576, 200, None, None, [(0, 64), (64, 128), (192, 128)]),     # doubling, capped at 1 GB / 8 MB = 128 lags
    (500, 0, 0, 1048576, 500, None, None, [(0, 64), (64, 128), (192, 128), (320, 128), (448, 64)]),   # to the cap: 500 lags in 16 blocks
    (500, 0, 0, 1048576, 500, None, 8, [(32 * i, 32) for i in range(16)]),       # 8 MB: one lag fits, so one block a round
    (500, 64, 0, 1048576, 500, None, None, [(0, 64)]),                           # max_lag = 64: kmax = 31, lags 0..63
    (500, 0, 200, 4096, 0, None, None, [(0, 224)]),                              # the functions' lags in the first round
    (500, 0, 200, 4096, 0, None, 1, [(0, 32), (32, 32), (64, 32), (96, 32), (128, 32), (160, 32), (192, 32)]),   # ... unless they do not fit
    (500, 0, 0, 4096, 300, 1, None, [(0, 32), (32, 64), (96, 128), (224, 256)]),
    (500, 0, 0, 4096, 300, 33, None, [(0, 64), (64, 128), (192, 256)]),
    (2, 0, 0, 8, 2, None, None, [(0, 32)]),
    (40, 0, 0, 8, 40, None, None, [(0, 64)]),
])
def test_rounds(driver, L, max_lag, nf, series, decided, first, mb, want):
    rows = rounds_of(driver, first_lags=first, work_mb=mb, L=L, max_lag=max_lag, n_functions=nf, series=series, E=series // 2, zs=2, decided=decided)
    assert [(r[0], r[1]) for r in rows] == want
    cap, kmax = er.window_shape(L, max_lag)
    needed = max(2 * kmax + 2, min(nf, cap + 1))
    done = 0
    for first_lag, lags, blocks, gx, gy, gz in rows:
        assert first_lag == done and lags % B == 0 and blocks == lags // B >= 1
        assert lags == B or lags * series * 8 <= (mb or 1024) << 20
        assert gx == -(-(series // 2) // 64) and (gy - 1) * 4 < blocks <= gy * 4 and gz == 2 and gy <= 65535
        done += lags
    assert done <= -(-needed // B) * B and done >= min(max(decided, min(nf, cap + 1)), needed)


def test_capacity_keeps_grid_y_within_the_launch_limit(driver):
    assert int(_run(driver, "capacity", work_bytes=2 ** 40, series=2)) == 65535 * 4 * B
    assert int(_run(driver, "capacity", work_bytes=0, series=2 ** 42)) == B
    assert int(_run(driver, "capacity", work_bytes=2 ** 30, series=2 ** 20)) == 128


def _hex(v):
    return float(v).hex()


def test_the_hosts_part_is_the_restatements(driver):
    rng = np.random.default_rng(3)
    for trial in range(40):
        kmax = int(rng.integers(0, 12))
        n = int(rng.integers(1, 2 * kmax + 4))
        rho = rng.uniform(-0.2, 1.0, n) * 0.9 ** np.arange(n)
        rho[0] = 1.0
        if trial % 7 == 3 and n > 2:
            rho[int(rng.integers(1, n))] = np.nan
        state, pairs, total = _run(driver, "window_walk", kmax=kmax, have=n, rho=",".join(_hex(v) for v in rho)).split()
        want = er.walk_window(rho, kmax)
        if want is None:
            assert int(state) == -1
            continue
        assert int(state) == want[2] and int(pairs) == want[1]
        if want[1]:
            np.testing.assert_array_equal(float.fromhex(total), want[0])
    for total, N in ((0.3, 1600.0), (10.25, 64000.0), (float("nan"), 100.0), (0.5 + 0.5 / math.log10(640.0), 640.0)):
        tau, ess = (float.fromhex(v) for v in _run(driver, "tau", total=_hex(total), N=_hex(N)).split())
        t = -1.0 + 2.0 * total
        floor = 1.0 / math.log10(N)
        want = floor if t < floor else t
        np.testing.assert_array_equal(tau, want)
        np.testing.assert_array_equal(ess, N / want)
    for S, M, L, within, between in ((123.456, 64.0, 1000.0, 1.7, 0.002), (-3.5, 12.0, 7.0, 0.25, 0.0), (0.0, 8.0, 3.0, 0.0, 0.0)):
        gamma, varplus, rho = (float.fromhex(v) for v in _run(driver, "rho", S=_hex(S), M=_hex(M), L=_hex(L), within=_hex(within), between=_hex(between), t=3).split())
        with np.errstate(all="ignore"):
            g = (np.float64(S) / np.float64(M)) / np.float64(L)
            v = (np.float64(within) * np.float64(L - 1)) / np.float64(L) + np.float64(between)
            np.testing.assert_array_equal([gamma, varplus, rho], [g, v, 1.0 - (np.float64(within) - g) / v])
