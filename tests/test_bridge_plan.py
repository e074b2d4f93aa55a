"""mcmcpp_amd/csrc/bridge_plan.hpp: the host's decisions of the bridge estimate (mcmcpp_hip_evidence_bridge), on the CPU.
tests/cpp/bridge_plan_cases.cpp compiles the header with the host compiler alone and prints what it plans: the tiles and
slices of sum_tree, the launch shapes, the buffers of raw u in flight; and it runs the header's own sum_tree, sigma and solver
on the host, which must equal the numpy restatement (tests/bridge_restatement.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import bridge_restatement as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SLICE = 1024 * 64  # terms of a whole slice
SIZES = [1, 1023, 1024, 1025, SLICE, SLICE + 1, 2 ** 24]


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "bridge_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: bridge_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "bridge_plan_cases.cpp"), "-I", CSRC])
    return exe


def _run(exe, what, **args):
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]


def _bits(x):
    return "%016x" % int(np.array([x], np.float64).view(np.uint64)[0])


@pytest.mark.parametrize("N", SIZES)
def test_tiles_slices_and_launch_shapes(driver, N):
    lines = _run(driver, "plan", N=N)
    head = {k: int(v) for k, v in (kv.split("=") for kv in lines[0].split())}
    tiles = -(-N // 1024)
    slices = -(-tiles // 64)
    assert head == dict(tiles=tiles, slices=slices, grid_x=tiles, grid_y=2, tile_sums=6 * tiles, slice_sums=6 * slices, fits=1)
    spans = [tuple(int(v) for v in line.split()) for line in lines[1:]]
    assert [s[0] for s in spans] == list(range(slices))
    at = 0
    for _, first, count in spans:  # the slices tile [0, tiles): none empty, only the last short
        assert first == at and 1 <= count <= 64
        at += count
    assert at == tiles and all(s[2] == 64 for s in spans[:-1])
    # the expected counts at the sizes the issue names
    assert (tiles, slices) == {1: (1, 1), 1023: (1, 1), 1024: (1, 1), 1025: (2, 1), SLICE: (64, 1), SLICE + 1: (65, 2), 2 ** 24: (16384, 256)}[N]


def test_limits_and_grid_bound(driver):
    assert _run(driver, "limits") == ["threads=256 tile=1024 slice_tiles=64 bracket=1100 newton=200 tolerance=%s" % _bits(2.0 ** -40)]
    most = (2 ** 31 - 1) * 1024  # the tiles are the launch grid's x
    assert _run(driver, "plan", N=most)[0].endswith("fits=1") and _run(driver, "plan", N=most + 1)[0].endswith("fits=0")


@pytest.mark.parametrize("K", [2, 3, 16])
def test_buffers_in_flight(driver, K):
    lines = _run(driver, "buffers", K=K)
    assert int(lines[0]) == (2 if K == 2 else 3)
    rows = [tuple(int(v) for v in line.split()) for line in lines[1:]]
    assert [(d, p) for d, p, _ in rows] == [(d, p) for p in range(K - 1) for d in range(2)]
    where = {(d, p): b for d, p, b in rows}
    assert all(0 <= b < int(lines[0]) for b in where.values())
    for k in range(K):
        # what is alive while rung k's draws are evaluated: u(0, k - 1) and u(1, k) are written, u(1, k - 1) is still held
        alive = [(d, p) for d, p in ((0, k - 1), (1, k), (1, k - 1)) if 0 <= p < K - 1]
        assert len({where[x] for x in alive}) == len(alive)


@pytest.mark.parametrize("N", SIZES)
def test_host_sum_tree_equals_the_restatement(driver, tmp_path, N):
    rng = np.random.default_rng(N % 1000)
    v = rng.random(N) * np.exp(rng.standard_normal(N) * 3.0)
    path = tmp_path / "v.bin"
    v.tofile(str(path))
    assert _run(driver, "sum", file=path) == [_bits(br.sum_tree(v))]


def test_host_sigma_equals_the_restatement(driver, tmp_path):
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal(2000) * 30.0, [0.0, -0.0, np.inf, -np.inf, 708.0, -708.0, -709.0, 745.0, -745.0, 1e300, -1e300]])
    path = tmp_path / "x.bin"
    x.tofile(str(path))
    want = br.sigma(x)
    assert _run(driver, "sigma", file=path) == [_bits(h) for h in want]
    assert want[2000] == 0.5 and want[2001] == 0.5 and want[2002] == 1.0 and want[2003] == 0.0 and not np.signbit(want[2003])
    assert ((0.0 <= want) & (want <= 1.0)).all()


@pytest.mark.parametrize("name, N, shift", [("near", 1500, 0.3), ("far", 1025, 40.0), ("below", 70000, -6.0)])
def test_host_solver_equals_the_restatement(driver, tmp_path, name, N, shift):
    rng = np.random.default_rng(len(name))
    u0 = rng.standard_normal(N) * 2.0 + shift
    u1 = rng.standard_normal(N) * 2.0 - shift - 1.0
    path = tmp_path / "u.bin"
    np.concatenate([u0, u1]).tofile(str(path))
    c, passes, converged = br.solve(u0, u1)
    S, Q, H, _ = br.one_pass(u0, u1, c, final=True)
    lines = _run(driver, "solve", file=path)
    assert lines[0].split() == [_bits(c), str(passes + 1), str(converged)]
    assert lines[1].split() == [_bits(x) for x in (S[0], S[1], Q[0], Q[1], H[0], H[1])]
    assert converged == 1 and abs(c - (shift + 0.5)) < 1.0
