"""The HIP resources of the library have one owner each (CPU test: no GPU needed).  Device buffers, pinned host buffers,
events, instantiated graphs and streams are held by the owner types of mcmcpp_amd/csrc/sampler_base.hpp, which are the only code
that gives them back to the runtime; a hand-written free anywhere else is a second free list to keep in step."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
OWNER_HEADER = "sampler_base.hpp"
FREES = re.compile(r"hipFree\(|hipHostFree\(|hipEventDestroy|hipGraphExecDestroy|hipStreamDestroy")


def test_only_the_owner_header_frees():
    sources = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp")))
    assert OWNER_HEADER in sources and len(sources) > 10
    offenders = []
    for name in sources:
        if name == OWNER_HEADER:
            continue
        with open(os.path.join(CSRC, name)) as f:
            for number, line in enumerate(f, 1):
                if FREES.search(line):
                    offenders.append("%s:%d: %s" % (name, number, line.strip()))
    assert not offenders, "HIP resources freed outside %s:\n%s" % (OWNER_HEADER, "\n".join(offenders))
    with open(os.path.join(CSRC, OWNER_HEADER)) as f:
        header = f.read()
    assert all(s in header for s in ("hipFree(", "hipHostFree(", "hipEventDestroy", "hipGraphExecDestroy", "hipStreamDestroy"))


def test_owners_are_move_only(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "owners_static.hip")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-I" + CSRC, src], cwd=str(tmp_path))
