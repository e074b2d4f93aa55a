"""mcmcpp_amd/csrc/mbar_plan.hpp: the host's decisions of the multistate Bennett acceptance ratio (mcmcpp_hip_evidence_mbar), on
the CPU.  tests/cpp/mbar_plan_cases.cpp compiles the header with the host compiler alone (no HIP header: that it compiles is an
assertion), and a second time as a stand-alone program with the address and undefined-behaviour sanitizers, which then runs the
same commands.  It prints what the header plans -- the numbering of the sums, the joint tree and a rung's, the buffers -- and
runs the header's own sum_tree, Cholesky solve, solver and covariance on the host with a host pass, which must equal the numpy
restatement (tests/mbar_restatement.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import bridge_restatement as br
from tests import mbar_restatement as mr
from tests.test_evidence_bridge import _iid_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def build_driver(sanitized=False):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "mbar_plan_cases" + ("_san" if sanitized else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O1"]
    # the host compiler alone, and no include path but the headers' own directory: mbar_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "mbar_plan_cases.cpp"), "-I", CSRC])
    return exe


@pytest.fixture(scope="module", params=("plain", "sanitized"))
def driver(request):
    return build_driver(request.param == "sanitized")


def _run(exe, what, **args):
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]


def _bits(x):
    return "%016x" % int(np.array([x], np.float64).view(np.uint64)[0])


def _row(v):
    return [_bits(x) for x in np.asarray(v, np.float64).ravel()]


def test_the_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "mbar_plan.hpp")).read()
    includes = [line.split()[1] for line in text.split("\n") if line.startswith("#include")]
    assert [i for i in includes if i.startswith('"')] == ['"bridge_plan.hpp"'] and "hip" not in " ".join(includes)


def test_limits(driver):
    assert _run(driver, "limits") == ["max_chains=16 batch=4 solver_passes=%d cap=%s tolerance=%s threads=256 tile=1024 slice_tiles=64"
                                      % (mr.SOLVER_PASSES, _bits(mr.STEP_CAP), _bits(mr.TOLERANCE))]
    assert mr.PASS_BOUND == 201


@pytest.mark.parametrize("K, N", [(2, 32), (2, 512), (3, 342), (3, 2560), (2, 67200), (16, 64), (8, 4200000)])
def test_trees_and_buffers(driver, K, N):
    p = {k: int(v) for k, v in (kv.split("=") for kv in _run(driver, "plan", K=K, N=N)[0].split())}
    Q = K + K * (K + 1) // 2
    tiles = lambda terms: -(-terms // 1024)
    slices = lambda terms: -(-tiles(terms) // 64)
    assert p == dict(Q=Q, joint_terms=K * N, joint_tiles=tiles(K * N), joint_slices=slices(K * N), rung_terms=N, rung_tiles=tiles(N), rung_slices=slices(N),
                     l=K * K * N, series=K * N, tile_sums=K * Q * tiles(N), slice_sums=K * Q * slices(N), totals=(K + 1) * Q, fits=1)
    # one pair of buffers serves the joint launch and the rungs' launch
    assert p["tile_sums"] >= Q * p["joint_tiles"] and p["slice_sums"] >= Q * p["joint_slices"]


def test_grid_bound(driver):
    most = (2 ** 31 - 1) * 1024  # the tiles of the joint tree are the launch grid's x
    assert _run(driver, "plan", K=2, N=most // 2)[0].endswith("fits=1") and _run(driver, "plan", K=2, N=most // 2 + 1)[0].endswith("fits=0")


@pytest.mark.parametrize("K", [2, 3, 16])
def test_every_sum_has_one_place(driver, K):
    lines = _run(driver, "index", K=K)
    groups = [tuple(int(v) for v in line.split()[1:]) for line in lines if line.startswith("group")]
    assert groups == [(k, 1 + K - k) for k in range(K)]
    rows = [tuple(int(v) for v in line.split()) for line in lines if not line.startswith("group")]
    assert [(k, l) for k, l, _ in rows] == [(k, l) for k in range(K) for l in range(k, K)]
    assert [i for _, _, i in rows] == list(range(K, K + K * (K + 1) // 2))  # behind the K sums S_k, row by row, without a gap


@pytest.mark.parametrize("KN", [1023, 1024, 1025, 65537])
def test_host_sum_tree_equals_the_restatement(driver, tmp_path, KN):
    rng = np.random.default_rng(KN % 1000)
    v = rng.random(KN) * np.exp(rng.standard_normal(KN) * 3.0)
    path = tmp_path / "v.bin"
    v.tofile(str(path))
    assert _run(driver, "sum", file=path) == [_bits(br.sum_tree(v))]


@pytest.mark.parametrize("M", [1, 2, 15])
def test_cholesky_solve_against_numpy(driver, tmp_path, M):
    rng = np.random.default_rng(M)
    B = rng.standard_normal((M, M))
    A = B @ B.T + M * np.eye(M)
    b = rng.standard_normal(M)
    path = tmp_path / "a.bin"
    np.concatenate([[float(M)], A.ravel(), b]).tofile(str(path))
    lines = _run(driver, "chol", file=path)
    assert lines[0] == "1"
    assert lines[1].split() == _row(mr.substitute(mr.factor(A), b))  # the header's order, in bits
    x = np.array([int(h, 16) for h in lines[1].split()], np.uint64).view(np.float64)
    want = np.linalg.solve(A, b)
    # the condition number of B B^T + M I is below 1 + 4 M here; 64 ulp of the largest component leaves a wide margin
    assert np.abs(x - want).max() <= 64 * np.finfo(np.float64).eps * (1 + 4 * M) * np.abs(want).max()
    # a matrix that is not positive definite is refused
    A[M - 1, M - 1] = -1.0
    np.concatenate([[float(M)], A.ravel(), b]).tofile(str(path))
    assert _run(driver, "chol", file=path) == ["0"] and mr.factor(A) is None


def _solve_case(driver, tmp_path, l, n, W):
    K, N = l.shape[0], n * W
    want = mr.mbar(l, n, W)
    path, ess_path = tmp_path / "l.bin", tmp_path / "ess.bin"
    np.concatenate([[float(K), float(N)], l.ravel()]).tofile(str(path))
    np.asarray(want["ess"], np.float64).tofile(str(ess_path))
    lines = _run(driver, "solve", file=path, ess=ess_path)
    failed = int(np.isnan(want["log_z"]).all())
    assert lines[0].split() == [str(want["passes"]), str(want["converged"]), str(failed)]
    if failed:
        return want
    assert lines[1].split() == _row(want["log_z"])
    w = want["w"]
    S, P = mr.sums(w)
    tri = lambda P: [P[k, l] for k in range(K) for l in range(k, K)]
    assert lines[2].split() == _row(np.concatenate([S, tri(P)]))
    rung = [mr.sums(w[:, r * N:(r + 1) * N]) for r in range(K)]
    assert lines[3].split() == _row(np.concatenate([np.concatenate([s, tri(p)]) for s, p in rung]))
    assert lines[4].split() == _row(np.concatenate([w[r, r * N:(r + 1) * N] for r in range(K)]))
    assert lines[5].split() == _row(want["cov"]) and lines[6].split() == _row(want["log_ratio"]) and lines[7].split() == _row(want["mcse"])
    assert lines[8].split() == _row([want["log_ratio_total"], want["mcse_total"]])
    return want


@pytest.mark.parametrize("D, beta", [(8, 0.9), (32, 0.5), (8, 0.15)])
def test_host_solver_equals_the_restatement_on_a_pair(driver, tmp_path, D, beta):
    n, W = 256, 16
    want = _solve_case(driver, tmp_path, mr.l_of_pair(*_iid_pair(D, beta, n * W, 7)), n, W)
    assert want["converged"] == 1 and 3 <= want["passes"] <= mr.PASS_BOUND and want["mcse"][0] > 0


def test_host_solver_equals_the_restatement_on_a_ladder_and_at_the_edges(driver, tmp_path):
    n, W = 19, 18  # N = 342: the rungs' trees are short tiles that do not align with the joint tree's
    l = mr.iid_ladder(4, (1.0, 0.5, 0.25), n * W, 3)
    want = _solve_case(driver, tmp_path, l, n, W)
    assert want["converged"] == 1 and np.isfinite(want["cov"]).all()
    dead = l.copy()
    dead[:, 5] = -np.inf  # a draw outside every rung's support
    dead[1, 400] = -np.inf
    want = _solve_case(driver, tmp_path, dead, n, W)
    assert np.isfinite(want["log_z"]).all() and (want["w"][:, 5] == 0.0).all() and want["nonfinite"].sum() == 4
    disjoint = np.zeros((2, 2 * 64))
    disjoint[1, :64], disjoint[0, 64:] = -3000.0, -2000.0
    want = _solve_case(driver, tmp_path, disjoint, 8, 8)
    assert want["converged"] == 1 and want["passes"] == 1 and np.isnan(want["log_z"]).all()
    want = _solve_case(driver, tmp_path, np.zeros((2, 2 * 64)), 8, 8)
    assert want["passes"] == 2 and (want["log_z"] == 0.0).all() and (want["mcse"] == 0.0).all()
