"""The arithmetic the analysis entry points share when they take stored steps a chunk at a time (mcmcpp_amd/csrc/step_chunks.hpp),
checked on the CPU: the walk over the chunks, which steps of a chunk go in one copy, and the *_CHUNK_MB knob.

tests/cpp/step_chunks_cases.cpp is compiled with the host compiler against the header alone (no HIP header: that it compiles is
an assertion) and prints what the header computes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

STEP = 48  # bytes of a step: W = 3, P = 2, fp64
A = 4096   # the address of the first step


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "step_chunks_cases")
    # the host compiler alone, and no include path but the header's own directory: step_chunks.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", out, os.path.join(ROOT, "tests", "cpp", "step_chunks_cases.cpp"), "-I", CSRC])
    return out


def lines(exe, *args, env=None):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True, env=env).stdout
    return [tuple(int(x) for x in line.split()) for line in out.splitlines()]


def test_the_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "step_chunks.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<cstddef>", "<cstdlib>"]


@pytest.mark.parametrize("used", [0, 1, 7])
@pytest.mark.parametrize("per", [1, 2, 3, 7, 9])
def test_the_walk_covers_every_step_exactly_once(exe, used, per):
    chunks = lines(exe, "walk", used, per)
    assert len(chunks) == -(-used // per)
    covered = []
    for i, (k0, now) in enumerate(chunks):
        assert k0 == i * per and 1 <= now <= per
        assert now == per or i == len(chunks) - 1  # only the last chunk is ragged
        covered += range(k0, k0 + now)
    assert covered == list(range(used))


def addresses(run_lengths, gap=STEP):
    """steps laid out in runs of these lengths, `gap` bytes of something else between two runs"""
    out, at = [], A
    for n in run_lengths:
        out += [at + STEP * i for i in range(n)]
        at += STEP * n + gap
    return out


LAYOUTS = {
    "contiguous": (addresses([7]), [7]),
    "scattered": (addresses([1] * 7), [1] * 7),
    "runs_2_1_3_1": (addresses([2, 1, 3, 1]), [2, 1, 3, 1]),
    "descending": ([A + STEP * (6 - i) for i in range(7)], [1] * 7),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_contiguous_run_on_a_pointer_list(exe, name):
    addrs, want = LAYOUTS[name]
    assert len(addrs) == 7 and sum(want) == 7
    copies = lines(exe, "runs", STEP, 7, *addrs)
    assert [run for _, run in copies] == want
    assert [k for k, _ in copies] == [sum(want[:i]) for i in range(len(want))]
    # a chunk that ends inside a run: the run ends with the chunk
    for end in range(1, 8):
        copies = lines(exe, "runs", STEP, end, *addrs)
        assert sum(run for _, run in copies) == end and all(k + run <= end for k, run in copies)
        clipped, left = [], end
        for n in want:
            if left > 0:
                clipped.append(min(n, left))
            left -= n
        assert [run for _, run in copies] == clipped


def test_a_gap_of_any_other_size_breaks_a_run(exe):
    for gap in (8, STEP - 8, 2 * STEP):
        assert [run for _, run in lines(exe, "runs", STEP, 4, *addresses([2, 2], gap=gap))] == [2, 2]
    # a step that starts where the one before it started does not continue it either
    assert [run for _, run in lines(exe, "runs", STEP, 3, A, A, A + STEP)] == [1, 2]


@pytest.mark.parametrize("end", [1, 2, 7])
def test_contiguous_run_on_a_strided_chain(exe, end):
    # stride 1: the chunk is one run, which stops at the chunk's end although the chain goes on behind it
    assert lines(exe, "strided", 1, end, STEP) == [(0, end)]
    # stride 3: a copy per step
    assert lines(exe, "strided", 3, end, STEP) == [(k, 1) for k in range(end)]


@pytest.mark.parametrize("value,want_mb", [(None, 64), ("1", 1), ("0", 64), ("-5", 64), ("abc", 64), ("4096", 4096)])
def test_the_chunk_knob(exe, value, want_mb):
    env = {k: v for k, v in os.environ.items() if k != "STEP_CHUNKS_TEST_MB"}
    if value is not None:
        env["STEP_CHUNKS_TEST_MB"] = value
    assert lines(exe, "knob", "STEP_CHUNKS_TEST_MB", 64, env=env) == [(want_mb << 20,)]
    assert lines(exe, "knob", "STEP_CHUNKS_TEST_MB", 1024, env=env) == [((want_mb if want_mb != 64 else 1024) << 20,)]
