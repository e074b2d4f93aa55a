"""How the order-statistics kernels are launched: the plan of mcmcpp_amd/csrc/quantile_plan.hpp, checked on the CPU over a grid of
shapes, the ones no GPU test of a few seconds reaches included (2^31 - 1 samples in a chunk, 1024 parameters of 64 rank groups).

tests/cpp/quantile_plan_cases.cpp is compiled with the host compiler against the plan headers alone (no HIP header: that it
compiles is an assertion) and prints plans.  Every plan has to count every sample of every parameter in exactly one block, keep
its LDS within the limit and its grid within the launch limits, and index nothing past 32 bits; the digit schedule has to take
every key bit exactly once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

NS = [1, 255, 256, 257, 9000, 2 ** 31 - 1]
PS = [1, 2, 33, 130, 1024]
GROUPS = [1, 5, 8, 9, 64]
KEY_BITS = [32, 64]
CUS = [1, 256, 304]
LDS = 65536
U32 = 2 ** 32
UNROLL = 8  # kQuantUnroll of quantiles.hip: a thread looks this many strides of rows ahead of its sample


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "quantile_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: quantile_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "quantile_plan_cases.cpp"),
                           "-I", CSRC])
    return exe


def _fields(line):
    return {k: int(v) for k, v in (f.split("=") for f in line.split())}


def plan_of(exe, **args):
    out = subprocess.run([exe, "plan"] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout
    return _fields(out.strip())


def digits_of(exe, key_bits, digit_bits=None):
    args = ["key_bits=%d" % key_bits] + (["digit_bits=%d" % digit_bits] if digit_bits else [])
    out = subprocess.run([exe, "digits"] + args, capture_output=True, text=True, check=True).stdout
    return [tuple(int(v) for v in d.split(":")) for d in out.split()]


@pytest.fixture(scope="module")
def driver():
    return build_driver()


@pytest.fixture(scope="module")
def limits(driver):
    return _fields(subprocess.run([driver, "limits"], capture_output=True, text=True, check=True).stdout.strip())


def _slices_cover(n, blocks, per, slices):
    """block b takes samples [b * per, min(n, (b + 1) * per)): every sample once, no block empty"""
    assert per >= 1 and 1 <= blocks <= slices
    assert (blocks - 1) * per < n <= blocks * per
    assert blocks * per < U32          # blockIdx.x * per is a 32-bit product in the kernels
    assert n + 256 * UNROLL < U32      # and a thread's look-ahead past the end of its slice does not wrap


def _tiles_cover(P, tile, ptiles):
    """block y takes parameters [y * tile, min(P, (y + 1) * tile)): every parameter once, no block empty, a thread for each"""
    assert 1 <= tile <= 256 and (ptiles - 1) * tile < P <= ptiles * tile


def check(p, limits):
    n, P, G, kb = p["n"], p["P"], p["groups"], p["key_bits"]
    assert p["digit_bits"] == limits["digit_bits"] and p["cells"] == 2 ** p["digit_bits"]
    assert p["counters"] == P * G * p["cells"]
    set_bytes = p["cells"] * 4 + kb // 8
    _tiles_cover(P, p["tile"], p["ptiles"])
    _slices_cover(n, p["blocks"], p["per"], p["slices"])
    fit = p["lds_limit"] // (G * set_bytes)
    if p["lds"]:
        assert p["lds_bytes"] == p["tile"] * G * set_bytes <= p["lds_limit"]
        assert fit >= min(P, limits["min_tile"]) and p["tile"] >= min(P, limits["min_tile"])  # (evening out never narrows below the rule)
        assert p["tile"] * G * p["cells"] < 2 ** 31  # the kernel's LDS index is an int
        assert (p["tile"] * G * p["cells"] * 4) % 8 == 0  # the prefixes behind the counters are aligned for 64-bit keys
    else:
        assert p["lds_bytes"] == 0 and fit < min(P, limits["min_tile"])
        assert p["tile"] == min(P, 256)
    # grid (blocks, ptiles, 1)
    assert p["blocks"] <= limits["grid_x"] and p["ptiles"] <= limits["grid_y"] and 1 <= limits["grid_z"]
    # the rank pass
    _tiles_cover(P, p["rank_tile"], p["rank_ptiles"])
    _slices_cover(n, p["rank_blocks"], p["rank_per"], p["rank_slices"])
    assert p["rank_tile"] == -(-P // p["rank_ptiles"]) and p["rank_ptiles"] == -(-P // 256)
    assert p["rank_blocks"] <= limits["grid_x"] and p["rank_ptiles"] <= limits["grid_y"]
    assert p["query_tile"] == limits["query_tile"] >= 1


def test_quantile_plan_header_includes_no_hip_header():
    for name, want in (("quantile_plan.hpp", ["<cstddef>", "<cstdint>", '"hist_plan.hpp"']), ("hist_plan.hpp", ["<cstddef>", "<cstdint>"])):
        text = open(os.path.join(CSRC, name)).read()
        assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == want


def test_the_quantile_source_holds_no_launch_arithmetic():
    text = open(os.path.join(CSRC, "quantiles.hip")).read()
    for gone in ("65536", "1 << 31", "cus * ", "+ 255) / 256", "1024 +", "<= src.lds_limit", "lds_limit /", "hist_slices_for", "kQuantMinTile", "> 64", "> 1024"):
        assert gone not in text, gone
    assert '#include "quantile_plan.hpp"' in text and "quantile_plan(" in text and "quantile_rank_plan(" in text and "quantile_digit(" in text
    assert "quantile_steps_per_chunk(" in text and "hist_lds_limit(" in text
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " quantile_plan.hpp " in makefile.split("HDRS")[1].split("\n")[0] and " quantiles.o " in makefile.split("OBJS")[1].split("\n")[0]
    assert "-ffp-contract=off" in makefile


def test_plan_over_the_grid_counts_every_sample_once_within_the_limits(driver, limits):
    args = ["n=" + ",".join(map(str, NS)), "P=" + ",".join(map(str, PS)), "groups=" + ",".join(map(str, GROUPS)), "key_bits=" + ",".join(map(str, KEY_BITS)),
            "cus=" + ",".join(map(str, CUS)), "lds=%d" % LDS]
    out = subprocess.run([driver, "grid"] + args, capture_output=True, text=True, check=True).stdout
    plans = [_fields(line) for line in out.strip().split("\n")]
    assert len(plans) == len(NS) * len(PS) * len(GROUPS) * len(KEY_BITS) * len(CUS)
    assert {(p["n"], p["P"], p["groups"], p["key_bits"], p["cus"]) for p in plans} == {(n, P, g, k, c) for n in NS for P in PS for g in GROUPS for k in KEY_BITS
                                                                                      for c in CUS}
    for p in plans:
        check(p, limits)
    # the grid holds what it was chosen for
    assert any(p["lds"] and p["ptiles"] == 1 for p in plans) and any(p["lds"] and p["ptiles"] > 1 for p in plans)
    assert any(not p["lds"] and p["ptiles"] == 1 for p in plans) and any(not p["lds"] and p["ptiles"] > 1 for p in plans)
    assert any(p["blocks"] > 1 for p in plans) and any(p["blocks"] == 1 and p["n"] > 256 for p in plans)
    assert any(p["lds_bytes"] > LDS - 2048 for p in plans)
    # with the limits of the entry points (64 ranks, 1024 parameters) at the corner of the grid
    assert limits["max_ranks"] == max(GROUPS) and limits["max_params"] == max(PS) and limits["threads"] == 256


@pytest.mark.parametrize("P,groups,key_bits,lds_limit,want", [
    (32, 1, 64, 65536, dict(lds=1, tile=32, ptiles=1, lds_bytes=32 * 1032)),       # the first pass of 32 parameters: one tile
    (32, 5, 64, 65536, dict(lds=1, tile=11, ptiles=3, lds_bytes=11 * 5 * 1032)),   # 12 sets of five fit: three tiles, evened out
    (32, 15, 64, 65536, dict(lds=1, tile=4, ptiles=8)),                            # four parameters of 15 groups just fit
    (32, 16, 64, 65536, dict(lds=0, tile=32, ptiles=1, lds_bytes=0)),              # 63 sets in all: three parameters of 16 would be too narrow
    (32, 16, 32, 65536, dict(lds=0, tile=32, ptiles=1)),
    (3, 16, 64, 65536, dict(lds=1, tile=3, ptiles=1)),                             # (but all of three parameters fit)
    (1, 63, 64, 65536, dict(lds=1, tile=1, lds_bytes=63 * 1032)),
    (1, 64, 64, 65536, dict(lds=0, tile=1, lds_bytes=0)),                          # 64 sets and their prefixes are 512 bytes too many
    (1024, 1, 32, 65536, dict(lds=1, tile=61, ptiles=17)),
    (1024, 64, 64, 65536, dict(lds=0, tile=256, ptiles=4)),
    (32, 5, 64, 32768, dict(lds=1, tile=6, ptiles=6)),                             # a device that offers 32 KiB
])
def test_the_paths_of_the_selection_pass(driver, P, groups, key_bits, lds_limit, want):
    p = plan_of(driver, n=100000, P=P, groups=groups, key_bits=key_bits, cus=256, lds=lds_limit)
    assert {k: p[k] for k in want} == want, p


@pytest.mark.parametrize("key_bits,digit_bits", [(32, None), (64, None), (32, 8), (64, 8), (32, 11), (64, 11), (64, 64), (32, 5)])
def test_the_digits_take_every_key_bit_exactly_once(driver, limits, key_bits, digit_bits):
    digits = digits_of(driver, key_bits, digit_bits)
    width = digit_bits or limits["digit_bits"]
    assert len(digits) == -(-key_bits // width)
    taken = []
    for shift, bits in digits:  # most significant first
        assert 1 <= bits <= width and shift >= 0
        taken += list(range(shift + bits - 1, shift - 1, -1))
    assert taken == list(range(key_bits - 1, -1, -1))


@pytest.mark.parametrize("chunk_bytes,step_bytes,W,want", [
    (1 << 30, 16384 * 32 * 8, 16384, 256),      # the chunk size bounds it
    (1 << 20, 512 * 33 * 8, 512, 7),
    (1 << 20, 2000 * 33 * 8, 2000, 1),          # one step at the least
    (2 ** 63 - 1, 16384 * 32 * 8, 16384, 2 ** 17 - 1),  # a device chain: 32-bit sample indexing alone bounds it
    (2 ** 63 - 1, 3 * 1 * 8, 3, 2 ** 31 // 3 - 1),
])
def test_steps_per_chunk(driver, chunk_bytes, step_bytes, W, want):
    out = subprocess.run([driver, "chunk", "chunk_bytes=%d" % chunk_bytes, "step_bytes=%d" % step_bytes, "W=%d" % W], capture_output=True, text=True, check=True)
    k = int(out.stdout)
    assert k == want and k * W < 2 ** 31
