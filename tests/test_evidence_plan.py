"""mcmcpp_amd/csrc/evidence_plan.hpp: the host's decisions of the evidence ratios (mcmcpp_hip_evidence_ratios), on the CPU.
tests/cpp/evidence_plan_cases.cpp compiles the header with the host compiler alone and prints what it plans: the numbering of
pairs and directions, which rungs' parameters a rung's draws are evaluated with, the steps of a chunk in both regimes, and the
launch shapes of the two kernels."""
import os
import subprocess

import pytest

from tests import rhat_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
KNOB = "MCMCPP_HIP_EVIDENCE_CHUNK_MB"


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "evidence_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: evidence_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "evidence_plan_cases.cpp"), "-I", CSRC])
    return exe


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def _run(exe, what, env=None, **args):
    e = {k: v for k, v in os.environ.items() if k != KNOB}
    e.update(env or {})
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True, env=e).stdout.split("\n")[:-1]


@pytest.mark.parametrize("K", [2, 3, 16])
def test_pairs_and_directions(driver, K):
    rows = [tuple(int(v) for v in line.split()) for line in _run(driver, "pairs", K=K)]
    want = []
    for d in range(2):
        for p in range(K - 1):
            # d-major; the stepping-stone direction takes the draws of the flatter rung p + 1 and evaluates them under p
            want.append((d, p, d * (K - 1) + p, p + 1 if d == 0 else p, p if d == 0 else p + 1))
    assert rows == want
    assert [r[2] for r in rows] == list(range(2 * (K - 1)))


@pytest.mark.parametrize("K", [2, 3, 16])
def test_a_rung_is_evaluated_once_under_its_own_parameters(driver, K):
    served = set()
    for line in _run(driver, "rungs", K=K):
        k, evals, uses = line.split()
        k = int(k)
        evals = [int(v) for v in evals.split("=")[1].split(",")]
        uses = [tuple(int(v) for v in u.split(":")) for u in uses.split("=")[1].split(",")]
        # its own parameters first and once, then each neighbour's: three launches at the most, two at the ends
        assert evals[0] == k and evals.count(k) == 1 and len(evals) == len(set(evals))
        assert sorted(evals[1:]) == [j for j in (k - 1, k + 1) if 0 <= j < K]
        assert len(evals) == (2 if k in (0, K - 1) else 3) and len(uses) == len(evals) - 1
        for other, (d, p) in zip(evals[1:], uses):
            # the (d, p) whose draws are this rung's and whose other rung is the neighbour evaluated
            assert (p + 1 if d == 0 else p) == k and (p if d == 0 else p + 1) == other
            served.add((d, p))
    assert served == {(d, p) for d in range(2) for p in range(K - 1)}


def test_chunks_in_both_regimes(driver):
    step_bytes = 64 * 4 * 8
    # one chunk: the default knob holds every step
    lines = _run(driver, "chunks", n=40, step_bytes=step_bytes)
    assert lines == [str((1024 << 20) // step_bytes), "0 40"]
    # several chunks of a size that does not divide n; host steps and a device chain alike
    for on_device in (0, 1):
        lines = _run(driver, "chunks", env={KNOB: "1"}, n=1300, step_bytes=step_bytes, on_device=on_device)
        assert lines == ["512", "0 512", "512 512", "1024 276"]
    # a step larger than the knob: a step at a time
    assert _run(driver, "chunks", env={KNOB: "1"}, n=3, step_bytes=3 << 20) == ["1", "0 1", "1 1", "2 1"]
    # a device chain of which every third step is used: rows of two used steps do not follow each other
    assert _run(driver, "chunks", n=3, step_bytes=step_bytes, on_device=1, slice=3) == ["1", "0 1", "1 1", "2 1"]
    assert _run(driver, "chunks", n=3, step_bytes=step_bytes, on_device=0, slice=3)[1:] == ["0 3"]  # (host steps are gathered by the upload)


@pytest.mark.parametrize("N, slen, slices", [(1, 1024, 1), (1024, 1024, 1), (1025, 1024, 2), (65600, 1088, 61), (2 ** 22, 65536, 64)])
def test_launch_shapes(driver, N, slen, slices):
    lines = _run(driver, "weights", N=N)
    head = dict(kv.split("=") for kv in lines[0].split())
    assert (int(head["slen"]), int(head["slices"])) == (slen, slices) == (rr.slice_len(N), rr.num_slices(N))
    assert int(head["blocks"]) == slices and int(head["fits"]) == 1
    assert int(head["tiles"]) == -(-min(N, slen) // 1024) and int(head["diff_blocks"]) == -(-N // 256)
    spans = [tuple(int(v) for v in line.split()) for line in lines[1:]]
    assert [s[0] for s in spans] == list(range(slices))
    at = 0
    for _, first, count in spans:  # the slices tile [0, N): none empty, only the last short
        assert first == at and 1 <= count <= slen
        at += count
    assert at == N and all(s[2] == slen for s in spans[:-1])
    assert _run(driver, "limits") == ["threads=256 tile=1024 grid_x=2147483647"]
