"""How rank.hip sorts and ranks: the plan of mcmcpp_amd/csrc/rank_plan.hpp, checked on the CPU.

tests/cpp/rank_plan_cases.cpp is compiled with the host compiler against the plan header alone (no HIP header: that it compiles
is an assertion) and prints plans over a grid of (S, P, key bits, work MB): every draw belongs to exactly one block, every key
bit to exactly one digit, the tiles cover the parameters once, the workspace stays within the budget or is that of one
parameter, its arrays do not overlap, and the grids stay within the launch limits."""
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
KNOB = "MCMCPP_HIP_RANK_WORK_MB"
B = 2048  # draws of a block of a sort pass (rank_items_per_block; test_limits pins it)


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "rank_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: rank_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rank_plan_cases.cpp"), "-I", CSRC])
    return exe


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def _run(exe, what, env=None, **args):
    e = {k: v for k, v in os.environ.items() if k != KNOB}
    e.update(env or {})
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True, env=e).stdout


def plan(exe, S, P, bits, work_mb):
    return {k: int(v) for k, v in (f.split("=") for f in _run(exe, "plan", S=S, P=P, bits=bits, work_mb=work_mb).split())}


def test_rank_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "rank_plan.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<cstddef>", "<cstdint>", "<cstdlib>", '"rhat_plan.hpp"']


def test_limits(driver):
    p = plan(driver, 1000, 1, 32, 1)
    assert p["items"] == B == p["threads"] * p["rounds"] and p["threads"] == 256 and p["digits"] == 256
    assert p["maxdraws"] == 2 ** 31 - 1 and p["xmax"] == 2 ** 31 - 1 and p["ymax"] == 65535 and p["default_mb"] == 1024


SIZES = (2, 63, 64, B - 1, B, B + 1, 3 * B + 17, 57600, 10 ** 6 + 3, 33554432, 2 ** 31 - 1)


@pytest.mark.parametrize("S", SIZES)
def test_every_draw_belongs_to_one_block(driver, S):
    if S > 10 ** 7:  # (millions of lines: the blocks are checked through their count and the arithmetic of a span)
        p = plan(driver, S, 1, 64, 1)
        assert p["blocks"] == -(-S // B) and p["draw_blocks"] == -(-S // 256) and p["blocks"] <= p["xmax"] and p["draw_blocks"] <= p["xmax"]
        return
    spans = np.array([[int(v) for v in line.split()] for line in _run(driver, "spans", S=S).strip().split("\n")])
    assert (spans[:, 0] == np.arange(len(spans)) * B).all() and (spans[:, 1] >= 1).all() and (spans[:, 1] <= B).all()
    assert (spans[:-1, 1] == B).all() and spans[:, 1].sum() == S and spans[-1, 0] + spans[-1, 1] == S


@pytest.mark.parametrize("bits", (32, 64))
def test_every_key_bit_belongs_to_one_digit(driver, bits):
    shifts = [int(v) for v in _run(driver, "digits", bits=bits).split()]
    covered = sorted(b for s in shifts for b in range(s, s + 8))
    assert covered == list(range(bits)) and shifts == sorted(shifts) and len(shifts) % 2 == 0  # (even: the sorted keys end where they began)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("bits", (32, 64))
def test_tiles_and_workspace(driver, S, bits):
    for P in (1, 3, 5, 32, 1024):
        for work_mb in (1, 3, 64, 1024, 65536):
            p = plan(driver, S, P, bits, work_mb)
            tile, tiles = p["tile"], p["tiles"]
            assert 1 <= tile <= P and tile <= p["ymax"]
            assert (tiles - 1) * tile < P <= tiles * tile  # the tiles cover the parameters once, none is empty
            assert p["bytes"] <= work_mb << 20 or (tile == 1 and p["bytes"] == p["one"])
            if tile < P:  # the next larger tile would not fit
                assert plan(driver, S, tile + 1, bits, 1 << 30)["bytes"] > work_mb << 20 or tile == 1
            # the arrays of the workspace follow each other, aligned, and hold what the kernels index
            order = [p[k] for k in ("keys_a", "keys_b", "idx_a", "idx_b", "table", "totals", "bytes")]
            assert order[0] == 0 and all(v % p["align"] == 0 for v in order)
            need = [S * (bits // 8) * tile] * 2 + [S * 4 * tile] * 2 + [p["blocks"] * 256 * 4 * tile, 256 * 4 * tile]
            assert all(order[i + 1] - order[i] >= need[i] for i in range(6))
            assert p["blocks"] <= p["xmax"] and p["draw_blocks"] <= p["xmax"] and p["passes"] == bits // 8


def test_the_tiles_of_the_gpu_cases(driver):
    """tests/test_rank_diagnostics.py's case "tiles" (S = 57600, P = 5, 64-bit keys): 3 MB hold two parameters, 1 MB one, the
    default all five"""
    assert plan(driver, 57600, 5, 64, 3)["tile"] == 2 and plan(driver, 57600, 5, 64, 1)["tile"] == 1 and plan(driver, 57600, 5, 64, 1024)["tile"] == 5


def test_grids_are_counted_in_64_bits_and_refused_past_the_limit(driver):
    for S, P in ((2, 1), (57600, 5), (2 ** 31 - 1, 1), (2 ** 31 - 1, 256), (2 ** 30, 511), (2 ** 30, 512), (2 ** 30, 1024), (2 ** 31 - 1, 1024)):
        blocks, fits = (int(v) for v in _run(driver, "grids", S=S, P=P).split())
        assert blocks == -(-S * P // 256) and fits == (blocks <= 2 ** 31 - 1), (S, P)
    assert _run(driver, "grids", S=2 ** 30, P=511).split()[1] == "1" and _run(driver, "grids", S=2 ** 30, P=512).split()[1] == "0"


def test_knob_and_key_bits(driver):
    assert _run(driver, "env").split() == [str(1024 << 20), "32", "128"]
    assert _run(driver, "env", {KNOB: "7"}).split()[0] == str(7 << 20)
    assert _run(driver, "env", {KNOB: "0"}).split()[0] == str(1024 << 20)  # (not a size: the default)


@pytest.mark.parametrize("S", SIZES)
def test_quantile_ranks_are_those_of_capi(driver, S):
    for q in (0.5, 0.05, 0.95):
        bits, lo, hi = (int(v) for v in _run(driver, "quantile", S=S, q=repr(q)).split())
        h, wlo, whi = capi.quantile_ranks([q], S)
        assert bits == int(h.view(np.uint64)[0]) and lo == wlo[0] and hi == whi[0]
