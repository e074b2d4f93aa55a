"""The source of stored steps the analysis entry points share (mcmcpp::StepSource and the device range check of
mcmcpp_amd/csrc/analysis_host.hpp), driven directly on a device by tests/cpp/step_source_device.hip: host pointer lists in four
layouts and a sliced device chain, for chunks of 1, 2, 3, 7 and 9 of the 7 steps, both element types; an empty selection; the
rule that a selection of one chunk is uploaded once; and what the range check says about a pointer with exactly enough room, one
byte too little, and host memory.  The arithmetic underneath is tests/test_step_chunks.py's, on the CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


@pytest.fixture(scope="module")
def program():
    """tests/cpp/step_source_device.hip with the flags of mcmcpp_amd/csrc/Makefile"""
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "step_source_device.hip")
    out = os.path.join(BUILD, "step_source_device")
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc", ".h")))
    if not os.path.exists(out) or os.path.getmtime(out) < max(newest, os.path.getmtime(src)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                               "-Wno-unused-function", "-Wno-unused-value", "-I" + CSRC, src, "-o", out])
    return out


def test_the_program_compiles(program):
    assert os.access(program, os.X_OK)


@pytest.mark.gpu
def test_step_source_and_range_check_on_the_device(program):
    run = subprocess.run([program], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    lines = run.stdout.splitlines()
    assert run.returncode == 0 and lines[-1] == "0 failed", run.stdout + run.stderr
    cases = [line for line in lines if line.startswith("ok  ")]
    assert len(cases) == len(lines) - 1
    # 2 types x (4 layouts + 3 slices) x 5 chunk sizes, the empty and the failing source of each type, 8 lines of the range check
    assert len(cases) == 2 * (4 + 3) * 5 + 2 * 2 + 8
