"""The schedule of a run whose stored steps stay in device memory (mcmcpp_hip_run_device): the `Device` delivery of
mcmcpp_amd/csrc/run_plan.hpp, checked on the CPU.

tests/cpp/device_chain_plan_cases.cpp is compiled with the host compiler against run_plan.hpp alone and prints the plan of one
request, chain k's offsets in the destination and a simulated run: the driver plays the host loop of
Sampler::run_into_device_chain with "process the oldest chunk" as the only way to make progress.

What must hold: a device destination needs no host ring, no staging bytes and no sub-chunks, whichever kernels step the handle;
stored step k is written whole by ensemble step (k + 1) * interval - 1, so a chunk that ended at step `end` has completed
exactly end // interval stored steps, and wait_stored may hear of those and no more; chain k starts k * n_saved stored steps
into the destination; and a request with a host destination is planned as it was before the destination existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

S64 = 64 * 4 * 8         # one stored step of 64 x 4 fp64
S14 = 14 * 3 * 4         # 168 bytes: no multiple of 16
S16384 = 16384 * 32 * 8  # 4 MiB


def _build(name):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-I", CSRC])

    def run(what, **args):
        return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return run


@pytest.fixture(scope="module")
def driver():
    return _build("device_chain_plan_cases")


@pytest.fixture(scope="module")
def earlier_driver():
    # the existing cases' driver, unchanged: it knows nothing of the destination and calls plan_chain as it always did
    return _build("run_plan_cases")


def _fields(line):
    return {k: v for k, v in (f.split("=") for f in line.split())}


def _expected_chunk(graph_steps, interval):
    """A graph replay's worth of steps in whole intervals, at least one interval (64 steps where graphs are off)."""
    return max(1, (graph_steps if graph_steps > 0 else 64) // interval) * interval


def _check_sim(line, n_saved, interval, chunk):
    head, *events = line.split(" | ")
    assert head == "sim interval=%d n_saved=%d chunk_steps=%d" % (interval, n_saved, chunk)
    total, announced, enqueued, ends = n_saved * interval, 0, 0, []
    for e in events:
        kind, v = e.split()[0], [int(x) for x in e.split()[1:]]
        if kind == "E":
            enq, now, seen, in_flight = v
            assert enq == enqueued and seen == announced
            assert now == min(chunk, total - enq) and now >= 1
            assert in_flight + 1 <= 2, "more than two chunks in flight: their events rotate over four slots"
            enqueued += now
            ends.append(enqueued)
        else:
            assert kind == "O"
            a, b, end = v
            assert end == ends.pop(0), "chunks finish in the order they were enqueued"
            assert a == announced, "stored steps are announced in order, each once"
            # stored step k is complete when ensemble step (k + 1) * interval - 1 has finished: exactly end // interval of them
            assert b == end // interval, "wait_stored hears of every stored step the finished chunk completed, and of no other"
            announced = b
    assert enqueued == total and not ends
    assert announced == n_saved, "nothing is left behind the final synchronisation"


@pytest.mark.parametrize("full_step", [1, 0])
@pytest.mark.parametrize("chains", [1, 3])
@pytest.mark.parametrize("n_saved", [1, 9, 70])
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("graph_steps", [300, 4, 0, -1])
def test_device_destination_plan_and_announcements(driver, graph_steps, interval, n_saved, chains, full_step):
    plan, offsets, sim = driver("device", step_bytes=S64, chains=chains, n_saved=n_saved, interval=interval, graph_steps=graph_steps, full_step=full_step)
    p = _fields(plan)
    assert p["mode"] == "device"
    # no host ring, no staging bytes, no sub-chunks, nothing forwarded, and the pinned question is not even asked
    assert p["need_host_ring"] == "0" and p["ring"] == "0" and p["ring_bytes"] == "0"
    assert p["half_bytes"] == "0" and p["n_sub"] == "0" and p["slice_bytes"] == "0"
    assert p["direct"] == "0" and p["ask_pinned"] == "0"
    assert int(p["acc_entries"]) == n_saved * interval * chains
    chunk = _expected_chunk(graph_steps, interval)
    assert int(p["chunk_steps"]) == chunk
    assert offsets == "offsets=" + ",".join(str(k * n_saved * S64) for k in range(chains))
    _check_sim(sim, n_saved, interval, chunk)


def test_device_destination_ignores_the_host_path_knobs(driver):
    """The host paths choose by the kernels, the size of a stored step and two knobs; a device destination by none of them."""
    want = None
    for kw in (dict(), dict(full_step=0), dict(trickle=0), dict(pinned_direct=0), dict(pinned=1), dict(subchunk_mb=1)):
        got = driver("device", step_bytes=S16384, n_saved=2000, interval=1, **kw)
        want = want or got
        assert got == want, kw
    p = _fields(want[0])
    assert p["mode"] == "device" and p["chunk_steps"] == "300" and p["need_host_ring"] == "0" and p["half_bytes"] == "0"
    # a stored step that no 16-byte pieces cover (the host path that can never trickle) is a device destination like any other
    p = _fields(driver("device", step_bytes=S14, n_saved=9, interval=2)[0])
    assert p["mode"] == "device" and p["n_sub"] == "0" and p["chunk_steps"] == "300"
    # an interval beyond a graph replay: a chunk is one interval, so that every chunk ends on a stored step
    plan, _, sim = driver("device", step_bytes=S64, n_saved=5, interval=1000)
    assert _fields(plan)["chunk_steps"] == "1000"
    _check_sim(sim, 5, 1000, 1000)


def test_no_accepted_counters_and_no_chain(driver):
    assert _fields(driver("device", step_bytes=S64, n_saved=9, interval=3, want_accepted=0)[0])["acc_entries"] == "0"
    # (a request without a chain is `nothing`, whatever the destination would have been)
    assert _fields(driver("device", step_bytes=S64, n_saved=9, chain_out=0)[0])["mode"] == "nothing"


HOST_CASES = [
    dict(step_bytes=S64, n_saved=70, interval=1),
    dict(step_bytes=S64, n_saved=9, interval=3, pinned=1),
    dict(step_bytes=S64, n_saved=9, interval=3, chains=3),
    dict(step_bytes=S16384, n_saved=2000, interval=1, pinned=1),
    dict(step_bytes=S16384, n_saved=20, interval=100),
    dict(step_bytes=S64, n_saved=9, interval=2, full_step=0),
    dict(step_bytes=S14, n_saved=9, interval=2),
    dict(step_bytes=S64, n_saved=9, interval=2, trickle=0),
    dict(step_bytes=S64, n_saved=9, interval=2, pinned_direct=0, pinned=1),
    dict(step_bytes=S64, n_saved=9, interval=2, chain_out=0),
    dict(step_bytes=S64, n_saved=9, interval=2, graph_steps=-1, subchunk_mb=1),
]


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
def test_host_destinations_are_planned_as_before(driver, earlier_driver, case):
    """The same request through plan_chain as the existing cases call it (run_plan_cases.cpp never sets the destination)."""
    assert driver("host", **case)[0] == earlier_driver("chain", **case)[0]
    assert _fields(driver("host", **case)[0])["mode"] in ("nothing", "subchunks", "trickle")


def test_the_sampler_holds_no_device_schedule_arithmetic():
    text = open(os.path.join(CSRC, "mcmcpp_hip.hip")).read()
    body = text[text.index("int run_into_device_chain("):text.index("// Device-visible address of")]
    for gone in ("/ interval", "/ (int64_t)interval", "% interval", "graph_steps", ">= 2"):
        assert gone not in body, gone
    assert "DeviceWindow" in body and "device_chain_offset" in body
