"""A device-resident Chain for the C++ facade (MCMCPP_CHAIN_MEMORY=device): the reference-style program -- runMCMC,
sliceAndBurnChain, AutoCorrCalc, CovarianceMatrix, CornerHistograms, PercentileAndMaximumFinder -- with every stored step left
in GPU memory.

CPU: the new C functions are declared, exported and bound; the driver and the example compile against the facade as C++11; the
wave schedule of the in-place compaction (mcmcpp_amd/csrc/chain_compact_plan.hpp, no HIP include) is race-free and equals a copy
to a fresh array for every small case; the Chain's new host code runs under AddressSanitizer and UBSan against a fake backend.

GPU: tests/cpp/device_facade.cpp runs every case twice, with a host chain and with a device chain, and the files the two runs
write are compared byte for byte.  The host run is pinned to the oracle and the reference's fixtures by tests/test_facade.py,
test_diffevo.py and test_batch_calc.py, so equality with it is equality with the reference.  What differs by design -- the
memory kind, hostBytesFetched() -- comes back as key=value lines."""
import os
import re
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
INC = ["-I" + os.path.join(ROOT, "include", "MCMCpp"), "-I" + os.path.join(ROOT, "include")]
LINK = ["-L" + os.path.join(ROOT, "mcmcpp_amd"), "-lmcmcpp_hip", "-Wl,-rpath," + os.path.join(ROOT, "mcmcpp_amd")]
NEW_FUNCTIONS = ["mcmcpp_hip_device_alloc", "mcmcpp_hip_device_free", "mcmcpp_hip_device_copy", "mcmcpp_hip_device_chain_last_error",
                 "mcmcpp_hip_device_chain_compact"]
HIPCC = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"]


def _newer_than_sources(exe, sources):
    dirs = [os.path.join(ROOT, "include"), CSRC]
    newest = max([os.path.getmtime(s) for s in sources] + [os.path.getmtime(os.path.join(dp, f)) for d in dirs for dp, _, fs in os.walk(d) for f in fs
                                                            if f.endswith((".h", ".hpp"))])
    return os.path.exists(exe) and os.path.getmtime(exe) >= newest


def _compile(src, out, extra=()):
    """g++ -std=c++11 -Wall -Wextra (-Werror) against the facade and libmcmcpp_hip.so"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, out)
    if not _newer_than_sources(exe, [src]):
        capi.build_library()
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"] + INC + [src, "-o", exe] + LINK + list(extra))
    return exe


def _driver():
    return _compile(os.path.join(ROOT, "tests", "cpp", "device_facade.cpp"), "device_facade", ["-ldl"])


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_new_c_functions_are_declared_exported_and_plain_c(tmp_path):
    header = open(os.path.join(ROOT, "include", "mcmcpp_hip.h")).read()
    capi.build_library()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTS
        assert getattr(capi.lib(), name) is not None
    src = tmp_path / "uses.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int main(void) { int64_t kept = 0; void* p = mcmcpp_hip_device_alloc(-1, 64); int rc = mcmcpp_hip_device_copy(p, p, 0);\n'
                   '  rc += mcmcpp_hip_device_chain_compact(MCMCPP_HIP_F64, -1, p, 0, 1, 0, 1, &kept); mcmcpp_hip_device_free(p);\n'
                   '  return rc + (int)kept + (mcmcpp_hip_device_chain_last_error() == 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "uses.o")])


def test_driver_and_example_compile_and_link_as_cxx11():
    """Fails to compile without the feature: both use Chain::memoryKind(), deviceSteps() and hostBytesFetched()."""
    _driver()
    _compile(os.path.join(ROOT, "examples", "skewed_gaussian_device_chain.cpp"), "skewed_gaussian_device_chain")


def test_the_facade_needs_no_hip_header_and_names_the_device_entry_points():
    text = ""
    for dp, _, fs in os.walk(os.path.join(ROOT, "include", "MCMCpp")):
        for f in fs:
            text += open(os.path.join(dp, f)).read()
    assert "hip/hip_runtime" not in text and "#include <hip" not in text
    for name in ("mcmcpp_hip_run_device(", "mcmcpp_hip_run_device_async(", "mcmcpp_hip_moments_add_device_steps_strided(", "mcmcpp_hip_histograms_compute_device(",
                 "mcmcpp_hip_autocorr_times_device(", "mcmcpp_hip_device_chain_compact(", "mcmcpp_hip_device_alloc(", "mcmcpp_hip_device_free(", "mcmcpp_hip_device_copy("):
        assert name in text, name
    # the Chain itself reaches the library through function pointers only (tests/cpp/chain_test.cpp links against nothing)
    for name in ("Chain.h", "ChainBlock.h", "ChainStepIterator.h", "ChainPsetIterator.h"):
        assert not re.search(r"mcmcpp_hip_\w+\(", open(os.path.join(ROOT, "include", "MCMCpp", "Chain", name)).read()), name


def test_compact_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "chain_compact_plan.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<cstdint>"]
    source = open(os.path.join(CSRC, "chain_ops.hip")).read()
    assert '#include "chain_compact_plan.hpp"' in source and "chain_compact_wave(" in source and "chain_compact_kept(" in source
    assert "asm" not in source  # plain loads and stores
    assert " chain_compact_plan.hpp " in open(os.path.join(CSRC, "Makefile")).read().split("HDRS")[1].split("\n")[0]


def _host_rule(n, burn, interval):
    """Chain::resetChainForSubSampling of the host chain (reference Chain.h:268-305): the source step of every kept step"""
    if burn == 0 and interval == 1:
        return list(range(n))
    if n <= burn or n - burn < interval:
        return []
    return list(range(burn, n, interval))


def test_wave_schedule_is_race_free_and_equals_a_copy_for_every_small_case():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "chain_compact_plan_cases")
    # the host compiler alone, and no include path but the header's own directory
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "chain_compact_plan_cases.cpp"), "-I", CSRC])
    lines = subprocess.run([exe, "40", "7"], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    seen, most_waves = set(), 0
    for line in lines:
        head, tail = line.split("|")
        n, burn, interval, kept = (int(x) for x in head.split())
        waves = [tuple(int(x) for x in w.split(":")) for w in tail.split()]
        seen.add((n, burn, interval))
        sources = _host_rule(n, burn, interval)
        assert kept == len(sources), line
        # execute the schedule on an array of step labels: a wave reads all its sources, then writes all its destinations
        chain = list(range(n))
        written = set()   # steps some wave has written so far
        moved = set()
        at = 0
        for first, count in waves:
            assert count >= 1 and first >= at, line  # ascending, no destination twice
            at = first + count
            dests = range(first, first + count)
            reads = [burn + j * interval for j in dests]
            assert all(r < n for r in reads), line
            # no wave reads a step that an earlier wave -- or this one -- writes ...
            assert not (set(reads) & (written | set(dests))), line
            values = [chain[r] for r in reads]
            for j, v in zip(dests, values):
                chain[j] = v
            written |= set(dests)
            moved |= set(dests)
        # ... and the destinations no wave moves are their own sources
        assert at <= kept and all(sources[j] == j for j in range(kept) if j not in moved), line
        assert chain[:kept] == sources, line   # = the copy to a fresh array
        most_waves = max(most_waves, len(waves))
    assert seen == {(n, b, i) for n in range(41) for b in range(n + 1) for i in range(1, 8)}
    assert most_waves >= 30  # (a shift by one step is one launch per step: the schedule's worst case is in the grid)


def test_chain_host_code_under_address_and_ub_sanitizers_with_a_fake_backend():
    """reserve, grow, commit, compact and iterate with malloc / free / memcpy behind the chain's function pointers: a stand-alone
    program of its own, mirrored on a host Chain"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "device_chain_host_san")
    src = os.path.join(ROOT, "tests", "cpp", "device_chain_host.cpp")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include", "MCMCpp"), "-I" + CSRC, src, "-o", exe, "-pthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "device_chain_host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- GPU: the driver, host chain against device chain -------------------------------------------------------------------

def _env(memory, **more):
    env = {k: v for k, v in os.environ.items() if k not in ("MCMCPP_CHAIN_MEMORY", "MCMCPP_DEVICE_ANALYSIS", "MCMCPP_CHAIN_DEVICE_FIRST_STEPS", "MCMCPP_DEVICES")}
    if memory:
        env["MCMCPP_CHAIN_MEMORY"] = memory
    env.update(more)
    return env


def _run(case, tmp_path, memory, tag=None, extra=(), **more):
    out = tmp_path / ("%s_%s.bin" % (case, tag or memory or "host"))
    r = subprocess.run([_driver(), case, str(out)] + list(extra), capture_output=True, text=True, env=_env(memory, **more), timeout=300)
    assert r.returncode == 0 and "device_facade OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    facts = dict(line.split("=", 1) for line in r.stdout.split("\n") if "=" in line)
    return out.read_bytes(), facts, out


def _both(case, tmp_path, extra=(), **more):
    host, host_facts, _ = _run(case, tmp_path, None, extra=extra, **more)
    dev, dev_facts, _ = _run(case, tmp_path, "device", extra=extra, **more)
    assert host_facts["kind"] == "heap" and dev_facts["kind"] == "device"
    assert len(host) > 1000 and host == dev, "%s: the device chain's run differs from the host chain's (%d and %d bytes)" % (case, len(host), len(dev))
    return host_facts, dev_facts


@pytest.mark.gpu
@pytest.mark.parametrize("case,stored", [("stretch", 201), ("stretch_f32_96x16", 61), ("stretch_f32_80x5", 61), ("diffevo", 101)])
def test_sampling_into_a_device_chain_equals_the_host_chain(case, stored, tmp_path):
    """every step through both iterators, accepted and total counts, getStoredSteps; then reset, storeCurrentWalkerPositions, run"""
    host_facts, dev_facts = _both(case, tmp_path)
    assert int(dev_facts["device_steps"]) == stored and int(host_facts["device_steps"]) == 0
    assert int(dev_facts["fetched_after_sampling"]) == 0


@pytest.mark.gpu
def test_batch_calculator_into_a_device_chain_equals_the_host_chain(tmp_path):
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "batch_calc.hip")
    lib = os.path.join(BUILD, "libbatch_calc.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(HIPCC + [src, "-o", lib])
    _, dev_facts = _both("batch", tmp_path, extra=[lib])
    assert int(dev_facts["device_steps"]) == 101 and int(dev_facts["fetched_after_sampling"]) == 0


@pytest.mark.gpu
def test_post_step_action_sees_the_same_steps_on_a_device_chain(tmp_path):
    """a PostStepAction that records the first walker of every step it sees, at every call (run_device_async + wait_stored)"""
    _both("action", tmp_path)


@pytest.mark.gpu
def test_a_device_chain_grows_once_and_fills_its_budget_like_the_host_chain(tmp_path):
    """a first reservation of 64 steps (the facade's test knob), runs of 20, 20 and 40 behind the initial placement: 81 steps, one
    reallocation.  Then a budget of 50 steps: the run that fills it returns false at 50 stored steps in both."""
    host_facts, dev_facts = _both("growth", tmp_path, MCMCPP_CHAIN_DEVICE_FIRST_STEPS="64")
    assert int(dev_facts["reallocations"]) == 1 and int(host_facts["reallocations"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["compact_64x4", "compact_80x5_f32"])
def test_slice_and_burn_on_the_device_equals_the_host_chain(case, tmp_path):
    """(burnIn, interval) in (0,1), (20,1), (0,5), (7,3), (n-1,1), (3,n) at n = 61: the chain afterwards, getStoredSteps, and the
    chain two more steps later; the call itself brings nothing to the host"""
    host_facts, dev_facts = _both(case, tmp_path)
    n = 61
    want = [len(_host_rule(n, b, i)) for b, i in ((0, 1), (20, 1), (0, 5), (7, 3), (n - 1, 1), (3, n))]
    assert want == [61, 41, 13, 18, 1, 0]
    for facts in (host_facts, dev_facts):
        assert [int(facts["stored_after_case_%d" % c]) for c in range(6)] == want
    assert int(dev_facts["fetched_by_slicing"]) == 0


@pytest.mark.gpu
def test_analysis_on_a_device_chain_equals_the_host_chain_and_fetches_nothing(tmp_path):
    """AutoCorrCalc, CovarianceMatrix, CornerHistograms (CSV files and bins) and PercentileAndMaximumFinder (its queries) behind
    burn-in and slicing, over the whole chain and over a range that starts inside it, slice intervals 1 and 3: bit for bit.
    Sampling, slicing and all four analyses copy no stored step to the host; one dereference then copies exactly one step."""
    host, host_facts, host_path = _run("analysis", tmp_path, None)
    dev, dev_facts, dev_path = _run("analysis", tmp_path, "device")
    assert host_facts["kind"] == "heap" and dev_facts["kind"] == "device"
    assert len(host) > 10000 and host == dev
    host_cov, dev_cov = open(str(host_path) + ".cov", "rb").read(), open(str(dev_path) + ".cov", "rb").read()
    assert len(host_cov) == 2 * 2 * 16 * 16 and host_cov == dev_cov
    assert int(dev_facts["fetched_after_analysis"]) == 0
    assert int(dev_facts["fetched_by_one_dereference"]) == 64 * 4 * 8
    assert int(host_facts["fetched_after_analysis"]) == 0 and int(host_facts["fetched_by_one_dereference"]) == 0
    # Mixed use.  MCMCPP_DEVICE_ANALYSIS=0 switches the classes' device path off.  A host chain's iterator pair never took it:
    # its results do not change.  A device chain's steps are then downloaded and go through the host entry points: the same
    # histograms and autocorrelation times (both bit-reproducible), and the download shows in the counter.
    host_off, _, host_off_path = _run("analysis", tmp_path, None, tag="host_off", MCMCPP_DEVICE_ANALYSIS="0")
    assert host_off == host and open(str(host_off_path) + ".cov", "rb").read() == host_cov
    dev_off, dev_off_facts, _ = _run("analysis", tmp_path, "device", tag="device_off", MCMCPP_DEVICE_ANALYSIS="0")
    assert dev_off == host and int(dev_off_facts["fetched_after_analysis"]) > 0


# ---- GPU: the kernel through the C ABI, at the shapes where it takes another path ---------------------------------------------

def _labelled(torch, n, W, D, dtype):
    """steps whose every element tells its step and its place (exact in float32 up to 2^24)"""
    place = (torch.arange(W * D, device="cuda", dtype=torch.float64) % 1021).reshape(1, W, D)
    return (torch.arange(n, device="cuda", dtype=torch.float64).reshape(n, 1, 1) * 1024 + place).to(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,D,dtype,what", [
    (61, 64, 4, "float64", "2 KiB steps: one block along a step, its unrolled loop never runs"),
    (61, 80, 5, "float32", "1600-byte steps"),
    (37, 10, 3, "float32", "120-byte steps: no whole number of 16-byte pieces, moved element by element"),
    (9, 1030, 7, "float64", "3605 pieces: four blocks along a step, unrolled loop and remainder loop both run"),
    (4, 2 ** 20 + 8, 4, "float64", "2 097 168 pieces: past 2048 blocks of 1024 pieces, the blocks stride over the step"),
])
def test_compact_kernel_equals_a_strided_copy(n, W, D, dtype, what):
    import torch
    dt = getattr(torch, dtype)
    cases = [(0, 1), (1, 1), (2, 1), (0, 2), (0, 5), (3, 2), (7, 3), (n - 1, 1), (3, n), (n, 1), (0, n)]
    for burn, interval in cases:
        steps = _labelled(torch, n, W, D, dt)
        want = steps[burn::interval].clone() if _host_rule(n, burn, interval) else steps[:0]
        kept = capi.device_chain_compact(steps, burn, interval)
        assert kept == len(_host_rule(n, burn, interval)) == want.shape[0], (burn, interval)
        assert torch.equal(steps[:kept], want), (what, burn, interval)
        if (burn, interval) == (0, 1):
            assert torch.equal(steps, _labelled(torch, n, W, D, dt))


@pytest.mark.gpu
def test_compact_kernel_behind_two_to_the_31_elements():
    """35 steps of 2^26 floats (8.75 GiB): the sources of burn 1, interval 2 reach element 33 * 2^26 > 2^31"""
    import torch
    n, elems = 35, 2 ** 26
    steps = torch.empty((n, elems // 4, 4), dtype=torch.float32, device="cuda")
    place = (torch.arange(elems, device="cuda", dtype=torch.int32) % 1021).to(torch.float32).reshape(elems // 4, 4)
    for k in range(n):
        torch.add(place, float(k * 1024), out=steps[k])
    assert capi.device_chain_compact(steps, 1, 2) == 17
    for j in range(17):
        assert torch.equal(steps[j], place + float((1 + 2 * j) * 1024)), j


@pytest.mark.gpu
def test_compact_refuses_what_is_not_one_device_allocation():
    import torch
    steps = torch.zeros((8, 16, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(capi.HipError) as e:  # more steps than the allocation holds: refused before anything is launched
        capi.device_chain_compact(steps.data_ptr(), 1, 1, n_steps=1 << 40, step_elems=32, dtype=capi.F64, device=steps.device.index)
    assert e.value.code == 1 and "allocation" in str(e.value)
    host = np.zeros((8, 32))
    with pytest.raises(capi.HipError) as e:
        capi.device_chain_compact(host.ctypes.data, 1, 1, n_steps=8, step_elems=32, dtype=capi.F64, device=steps.device.index)
    assert e.value.code == 1 and "device memory" in str(e.value)
    for bad in (dict(burn_in=-1, interval=1), dict(burn_in=0, interval=0)):
        with pytest.raises(capi.HipError):
            capi.device_chain_compact(steps, **bad)
