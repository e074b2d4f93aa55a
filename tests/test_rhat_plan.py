"""How the Gelman-Rubin kernels are launched: the plan of mcmcpp_amd/csrc/rhat_plan.hpp, checked on the CPU over a grid of
shapes, the ones no GPU test of a few seconds reaches included.

tests/cpp/rhat_plan_cases.cpp is compiled with the host compiler against the plan header alone (no HIP header: that it compiles
is an assertion) and prints plans.  The slices are those of the restatement (tests/rhat_restatement.py); every step of every
sequence is walked in exactly one slice by exactly one block; whatever the chunks, a slice's sums start fresh once, at its
first step, are carried through every later chunk and close once, at its last; and the grids stay within the launch limits."""
import os
import subprocess

import pytest

from tests import rhat_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

NS = [2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 65536, 65537, 70000, 140001, 10 ** 6, 2 ** 31 - 1, 2 ** 40]
ES = [1, 2, 3, 4, 30, 256, 257, 512, 513, 65541, 524288, 2 ** 31 - 2]
LS = [2, 1024, 1025, 70000, 2 ** 22]
ZS = [1, 2, 6, 32, 2048]
CUS = [1, 256, 304]


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "rhat_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: rhat_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rhat_plan_cases.cpp"), "-I", CSRC])
    return exe


def _run(exe, what, **args):
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout


def _fields(line):
    return {k: int(v) for k, v in (f.split("=") for f in line.split())}


def plan_of(exe, **args):
    return _fields(_run(exe, "plan", **args).strip())


@pytest.fixture(scope="module")
def driver():
    return build_driver()


@pytest.fixture(scope="module")
def limits(driver):
    return _fields(_run(driver, "limits").strip())


def test_rhat_plan_header_includes_no_hip_header():
    for name, want in (("rhat_plan.hpp", ["<cstddef>", "<cstdint>", '"step_chunks.hpp"']), ("step_chunks.hpp", ["<cstddef>", "<cstdlib>"])):
        text = open(os.path.join(CSRC, name)).read()
        assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == want


def test_the_rhat_source_holds_no_threshold_of_its_own():
    text = open(os.path.join(CSRC, "rhat.hip")).read()
    for gone in ("1024", "65535", "+ 63", "/ 64", "* cus", "multiProcessorCount *", ", prop.multiProcessorCount)", "% 16", "atomicAdd"):
        assert gone not in text.replace("default 1024", "").replace('"MCMCPP_HIP_RHAT_CHUNK_MB", 1024', ""), gone
    for used in ('#include "rhat_plan.hpp"', '#include "analysis_host.hpp"', "rhat_series_plan(", "rhat_sum_plan(", "rhat_slice_walk(", "rhat_block_slices(",
                 "rhat_half_begin(", "rhat_vector_width(", "rhat_steps_per_chunk(", "rhat_shape(", "rhat_plan_cus(prop.multiProcessorCount)", "check_device_steps(", "StepSource<T>", "ANALYSIS_TRY(",
                 "mcmcpp::Stream", "mcmcpp::DeviceBuffer"):
        assert used in text, used
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " rhat_plan.hpp " in makefile.split("HDRS")[1].split("\n")[0] and " rhat.o " in makefile.split("OBJS")[1].split("\n")[0]
    assert "-ffp-contract=off" in makefile


def test_slice_len_is_the_restatements(driver, limits):
    out = _run(driver, "slices", N=",".join(map(str, NS)))
    rows = [tuple(int(v) for v in line.split()) for line in out.strip().split("\n")]
    assert [r[0] for r in rows] == NS
    for N, slen, slices in rows:
        assert slen == rr.slice_len(N) and slices == rr.num_slices(N)
        assert slen >= limits["min_slice"] and slen % 64 == 0 and 1 <= slices <= limits["max_slices"]
        assert (slices - 1) * slen < N <= slices * slen
    assert rr.slice_len(70000) == 1152 and rr.num_slices(70000) == 61 and rr.slice_len(1025) == 1024 and rr.num_slices(1025) == 2


@pytest.mark.parametrize("K,n,W,split,want", [
    (1, 4, 4, 1, dict(H=2, L=2, M=8, begin0=0, begin1=2, last=7)),
    (1, 5, 4, 1, dict(H=2, L=2, M=8, begin0=0, begin1=3, last=7)),     # the middle step is dropped
    (3, 7, 6, 1, dict(H=2, L=3, M=36, begin0=0, begin1=4, last=35)),
    (3, 7, 6, 0, dict(H=1, L=7, M=18, begin0=0, begin1=0, last=17)),
    (1024, 2 ** 40, 2 ** 31 - 1, 1, dict(H=2, L=2 ** 39, M=2048 * (2 ** 31 - 1), begin1=2 ** 39, last=2048 * (2 ** 31 - 1) - 1)),
])
def test_sequences_and_halves(driver, K, n, W, split, want):
    got = _fields(_run(driver, "shape", K=K, n=n, W=W, split=split).strip())
    assert {k: got[k] for k in want} == want
    assert [(a, L) for a, L in rr.halves(n, split)] == [(got["begin0"], got["L"]), (got["begin1"], got["L"])][:got["H"]]


def _check_walk(lines, n, split, own):
    """every used step of every half once, in one slice of one block; every slice fresh once, carried, closed once"""
    halves = rr.halves(n, split)
    L = halves[0][1]
    slen, slices = rr.slice_len(L), rr.num_slices(L)
    by_slice = {}
    for h, g0, g1, y, t, s, f, fresh, closes in lines:
        a = halves[h][0]
        b, e = a + t * slen, min(a + (t + 1) * slen, a + L)
        assert g0 <= s < f <= g1 and b <= s and f <= e, "a block walks only its slice's steps, and only steps of the chunk"
        assert y == (0 if own else t) and 0 <= t < slices
        assert fresh == (s == b) and closes == (f == e)
        by_slice.setdefault((h, t), []).append((g0, s, f, fresh, closes))
    assert set(by_slice) == {(h, t) for h in range(len(halves)) for t in range(slices)}
    for (h, t), walks in by_slice.items():
        a = halves[h][0]
        b, e = a + t * slen, min(a + (t + 1) * slen, a + L)
        assert [w[0] for w in walks] == sorted({w[0] for w in walks}), "one block per (chunk, slice), chunks in order"
        assert walks[0][1] == b and walks[-1][2] == e
        assert all(x[2] == y[1] for x, y in zip(walks, walks[1:])), "a later chunk goes on where the one before stopped"
        assert [w[3] for w in walks] == [1] + [0] * (len(walks) - 1) and [w[4] for w in walks] == [0] * (len(walks) - 1) + [1]
    return slices


@pytest.mark.parametrize("n", [4, 5, 7, 2048, 2049, 2050, 2051, 2101, 5000, 140001])
@pytest.mark.parametrize("split", [1, 0])
def test_every_step_in_one_slice_of_one_block_whatever_the_chunks(driver, n, split):
    pers = sorted(({1, 2, 3} if n <= 5000 else {n // 37}) | {n // 3 + 1, n // 2, n // 2 + 1, 256, 1024, 1199, n - 1, n, n + 5})
    for per in pers:
        for own in (1, 0):
            out = _run(driver, "walk", n=n, split=split, per=per, own=own)
            lines = [tuple(int(v) for v in line.split()) for line in out.strip().split("\n")]
            _check_walk(lines, n, split, own)


def test_plan_over_the_grid_stays_within_the_launch_limits(driver, limits):
    out = _run(driver, "grid", E=",".join(map(str, ES)), L=",".join(map(str, LS)), zs=",".join(map(str, ZS)), cus=",".join(map(str, CUS)), elem_bytes="4,8",
               base="0,8,16,4096")
    plans = [_fields(line) for line in out.strip().split("\n")]
    assert len(plans) == len(ES) * len(LS) * len(ZS) * len(CUS) * 2 * 4
    for p in plans:
        E, eb = p["E"], p["elem_bytes"]
        whole = (E * eb) % 16 == 0 and p["base"] % 16 == 0
        assert p["vec"] == (16 // eb if whole else 1) and E % p["vec"] == 0
        assert p["lanes"] == E // p["vec"] and (p["etiles"] - 1) * 256 < p["lanes"] <= p["etiles"] * 256
        assert p["slen"] == rr.slice_len(p["L"]) and p["slices"] == rr.num_slices(p["L"])
        assert p["waves"] == -(-p["lanes"] // 64) * p["zs"]
        assert p["own"] == int(p["slices"] == 1 or p["waves"] >= limits["own_waves_per_cu"] * p["cus"])
        assert p["slots"] == (2 if p["own"] else p["slices"]) and p["slice_blocks"] == (1 if p["own"] else p["slices"])
        assert p["etiles"] <= limits["grid_x"] and p["slice_blocks"] <= limits["grid_y"] and p["grid_z"] == p["zs"] <= limits["grid_z"]
    assert any(p["own"] and p["slices"] > 1 for p in plans) and any(not p["own"] for p in plans)
    assert any(p["vec"] == 4 for p in plans) and any(p["vec"] == 2 for p in plans) and any(p["vec"] == 1 and p["elem_bytes"] == 8 for p in plans)
    # the entry points' limits at the corner of the grid: 1024 chains of two halves along z
    assert limits["max_chains"] * 2 == max(ZS) and limits["max_params"] == 1024 and limits["threads"] == 256 and limits["vector_bytes"] == 16


@pytest.mark.parametrize("N,P,G", [(2, 1, 1), (8, 3, 1), (1025, 1024, 1), (2 ** 42, 1024, 1), (2 * (2 ** 31 - 1), 1, 1024), (128, 4, 16)])
def test_the_combines_launch(driver, limits, N, P, G):
    p = _fields(_run(driver, "sum", N=N, P=P, G=G).strip())
    assert p["slen"] == rr.slice_len(N) and p["slices"] == rr.num_slices(N) and p["segments"] == G
    assert (p["blocks"] - 1) * 256 < p["slices"] * P <= p["blocks"] * 256  # a thread for every (slice, parameter)
    assert p["blocks"] <= limits["grid_x"] and G <= limits["grid_y"]


@pytest.mark.parametrize("chunk_bytes,step_bytes,want", [
    (1 << 30, 16384 * 32 * 8, 256),
    (1 << 20, 4096, 256),
    (1 << 20, 2000 * 33 * 8, 1),      # one step at the least
    (1 << 20, 262164, 3),
])
def test_steps_per_chunk(driver, chunk_bytes, step_bytes, want):
    assert int(_run(driver, "chunk", chunk_bytes=chunk_bytes, step_bytes=step_bytes)) == want
