"""How a run() delivers its stored steps and cuts itself into chunks: the schedules of mcmcpp_amd/csrc/run_plan.hpp, checked on
the CPU.  The GPU suite reaches this arithmetic only through whole runs with the few knob settings its tests happen to make; a
mistake in it corrupts stored chains or deadlocks a split run.

tests/cpp/run_plan_cases.cpp is compiled with the host compiler against run_plan.hpp alone (no HIP header: that it compiles is
an assertion) and prints the plan of one case given on its command line.  For the trickle window it prints a whole simulated
run: the driver plays the host loop of Sampler::run_trickle with "process the oldest chunk" as the only way to make progress.

The expected values were worked from the arithmetic run_whole / run_trickle / run_split held before it moved into the header
(by hand; _earlier_trickle_chunks below is a transcription of that loop, kept as the second opinion of the sweep).  The header
has to reproduce them.  A split run's whole schedule is SplitWindow's: the driver plays Sampler::run_split through it, with the
chunk tries that overflow and what each held chunk reports as the only inputs (split_sim, split_sweep).  fp64, one chain, graph_steps = 300 and a 32 MiB budget unless the case says otherwise."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

S2050 = 2050 * 32 * 8    # 524 800 bytes: one stored step of 2050 x 32 fp64
S16384 = 16384 * 32 * 8  # 4 MiB
S64 = 64 * 4 * 8


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "run_plan_cases")
    # the host compiler alone, and no include path but the header's own directory: run_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "run_plan_cases.cpp"), "-I", CSRC])

    def run(what, **args):
        return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return run


def test_run_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "run_plan.hpp")).read()
    includes = [line.split()[1] for line in text.split("\n") if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"]


def _body(text, head):
    """the braces that follow the one occurrence of `head` in `text`, and what they hold"""
    assert text.count(head) == 1, head
    at = text.index("{", text.index(head))
    depth = 0
    for i in range(at, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[at:i + 1]
    raise AssertionError("unbalanced braces behind " + head)


def test_the_sampler_holds_no_schedule_arithmetic():
    text = open(os.path.join(CSRC, "mcmcpp_hip.hip")).read()
    for gone in ("ring *= 2", "(ring - 2) / 2", "(copied + ring + 1)", "/ 8 + 64", "(size_t)256 << 20"):
        assert gone not in text, gone
    # the exchange side of a split handle holds none of it either
    exchange = open(os.path.join(CSRC, "split_exchange.hpp")).read()
    for gone in ("/ 8 + 64", "(size_t)256 << 20", "% interval", "% sample_stride"):
        assert gone not in exchange, gone
    # run_split asks SplitWindow: no sampling or storing arithmetic, no staging bookkeeping, and the slot bound is never assigned
    body = _body(text, "int run_split(")
    assert "SplitWindow win(" in body
    for gone in ("% interval", "% sample_stride", "staged - handed", "cap =", "cap_full;", "split_next_cap", "split_bytes_", "samples_before"):
        assert gone not in body, gone
    for used in ("win.chunk_overflowed()", "win.chunk_held(", "win.hand_out()", "win.take_sample(", "win.stores_step(", "win.take_stage_slot()"):
        assert used in body, used


# ---- simulated trickle runs ------------------------------------------------------------------------------------------------

class Sim:
    """One `sim ...` line of the driver."""

    def __init__(self, line):
        head, *events = line.split(" | ")
        assert head.startswith("sim ")
        self.p = {k: int(v) for k, v in (f.split("=") for f in head.split()[1:])}
        self.events = [(e.split()[0], [int(x) for x in e.split()[1:]]) for e in events]
        self.chunks = [v[1] for k, v in self.events if k == "E"]

    def check(self):
        """What must hold for every schedule, whatever its numbers."""
        p = self.p
        interval, n_saved, ring = p["interval"], p["n_saved"], p["ring"]
        announced = 0
        for kind, v in self.events:
            if kind == "E":
                enq, now, copied, in_flight = v
                assert now >= 1
                assert in_flight + 1 <= 2, "more than two chunks in flight"
                if not p["direct"]:
                    # the launches of this chunk forward stored steps up to (enq + now) / interval - 2 and write the device
                    # slot of stored step (enq + now) / interval - 1: none of their ring slots may still be waiting for its copy
                    assert enq + now <= (copied + ring + 1) * interval, "a launch would forward into a slot that is not copied out yet"
                assert copied == announced
            elif kind == "O":
                a, b, end = v
                assert a == announced and b >= a, "stored steps are announced in order, each once"
                assert b <= end // interval - 1, "a stored step was announced before the launches had forwarded all of it"
                announced = b
            else:
                a, b = v
                assert a == announced, "stored steps are announced in order, each once"
                assert (a, b) == (n_saved - 1, n_saved), "exactly the last stored step is left for the copy behind the final synchronisation"
                announced = b
        assert announced == n_saved
        assert self.events[-1][0] == "T" and [k for k, _ in self.events].count("T") == 1
        assert sum(self.chunks) == n_saved * interval
        return self


def _earlier_trickle_chunks(n_saved, interval, ring, chunk_steps, direct):
    """The host loop run_trickle held before the window moved into run_plan.hpp, transcribed: the chunk lengths it enqueued."""
    total = n_saved * interval
    enq = copied = next_chunk = oldest = 0
    chunk_end = [0, 0, 0, 0]
    chunks = []
    while enq < total:
        now = min(total - enq, chunk_steps)
        if not direct and now == total - enq and now > interval:
            now -= interval
        while next_chunk > oldest and (next_chunk - oldest >= 2 or (not direct and enq + now > (copied + ring + 1) * interval)):
            copied = max(copied, chunk_end[oldest & 3] // interval - 1)
            oldest += 1
        enq += now
        chunk_end[next_chunk & 3] = enq
        next_chunk += 1
        chunks.append(now)
    return chunks


def _fields(line):
    return dict(f.split("=") for f in line.split())


TRICKLE_CASES = [
    # name, driver arguments, plan fields, chunk lengths enqueued
    ("2050x32_32mb_interval_1_100_stored_pageable", dict(step_bytes=S2050, n_saved=100),
     "mode=trickle ask_pinned=1 direct=0 sub_saved=13 n_sub=0 ring=64 chunk_steps=31 acc_entries=100 half_bytes=0 ring_bytes=33587200 need_host_ring=1 slice_bytes=524800",
     [31, 31, 31, 6, 1]),
    ("2050x32_1mb_interval_1_100_stored_pageable", dict(step_bytes=S2050, n_saved=100, subchunk_mb=1),
     "mode=trickle ask_pinned=1 direct=0 sub_saved=1 n_sub=0 ring=4 chunk_steps=1 acc_entries=100 half_bytes=0 ring_bytes=2099200 need_host_ring=1 slice_bytes=524800",
     [1] * 100),
    ("2050x32_1mb_interval_3_10_stored_pageable", dict(step_bytes=S2050, n_saved=10, interval=3, subchunk_mb=1),
     "mode=trickle ask_pinned=1 direct=0 sub_saved=1 n_sub=0 ring=4 chunk_steps=3 acc_entries=30 half_bytes=0 ring_bytes=2099200 need_host_ring=1 slice_bytes=174944",
     [3] * 10),
    ("16384x32_32mb_interval_5_40_stored_pageable", dict(step_bytes=S16384, n_saved=40, interval=5),
     "mode=trickle ask_pinned=1 direct=0 sub_saved=5 n_sub=0 ring=16 chunk_steps=35 acc_entries=200 half_bytes=0 ring_bytes=67108864 need_host_ring=1 slice_bytes=838864",
     [35] * 5 + [20, 5]),
    ("16384x32_32mb_interval_5_40_stored_pinned", dict(step_bytes=S16384, n_saved=40, interval=5, pinned=1),
     "mode=trickle ask_pinned=1 direct=1 sub_saved=5 n_sub=0 ring=16 chunk_steps=300 acc_entries=200 half_bytes=0 ring_bytes=67108864 need_host_ring=0 slice_bytes=838865",
     [200]),
    ("2050x32_32mb_graph_steps_8_interval_1_20_stored_pinned", dict(step_bytes=S2050, n_saved=20, graph_steps=8, pinned=1),
     "mode=trickle ask_pinned=1 direct=1 sub_saved=3 n_sub=0 ring=64 chunk_steps=8 acc_entries=20 half_bytes=0 ring_bytes=33587200 need_host_ring=0 slice_bytes=524801",
     [8, 8, 4]),
    ("64x4_32mb_interval_400_3_stored_pageable", dict(step_bytes=S64, n_saved=3, interval=400),
     "mode=trickle ask_pinned=1 direct=0 sub_saved=1 n_sub=0 ring=64 chunk_steps=400 acc_entries=1200 half_bytes=0 ring_bytes=131072 need_host_ring=1 slice_bytes=16",
     [400, 400, 400]),
    ("64x4_interval_1_1_stored_pageable", dict(step_bytes=S64, n_saved=1),
     "mode=trickle ask_pinned=1 direct=0 sub_saved=1 n_sub=0 ring=64 chunk_steps=31 acc_entries=1 half_bytes=0 ring_bytes=131072 need_host_ring=1 slice_bytes=2048",
     [1]),
    # graph replays off (plain launches): 64 steps stand in for a replay; three chains, no per-step counts
    ("3_chains_no_graphs_no_counts", dict(step_bytes=S2050, n_saved=12, interval=2, chains=3, graph_steps=-1, want_accepted=0),
     "mode=trickle ask_pinned=1 direct=0 sub_saved=2 n_sub=0 ring=64 chunk_steps=62 acc_entries=0 half_bytes=0 ring_bytes=100761600 need_host_ring=1 slice_bytes=262400",
     [22, 2]),
    # the knob says no to forwarding in place: the question is not asked, a pinned chain_out goes through the ring
    ("pinned_direct_0", dict(step_bytes=S2050, n_saved=20, graph_steps=8, pinned=1, pinned_direct=0),
     "mode=trickle ask_pinned=0 direct=0 sub_saved=3 n_sub=0 ring=64 chunk_steps=8 acc_entries=20 half_bytes=0 ring_bytes=33587200 need_host_ring=1 slice_bytes=524800",
     [8, 8, 3, 1]),
]


@pytest.mark.parametrize("name,args,plan,chunks", TRICKLE_CASES, ids=[c[0] for c in TRICKLE_CASES])
def test_trickle_plan_and_simulated_run(driver, name, args, plan, chunks):
    out = driver("chain", **args)
    assert _fields(out[0]) == _fields(plan)
    sim = Sim(out[1]).check()
    assert sim.chunks == chunks
    p = sim.p
    assert sim.chunks == _earlier_trickle_chunks(p["n_saved"], p["interval"], p["ring"], p["chunk_steps"], p["direct"])
    # a stored step's ring slot: its number modulo the ring
    assert _fields(out[2]) == {"ring_slot_of_last": str((p["n_saved"] - 1) % p["ring"])}


def test_trickle_window_over_a_sweep(driver):
    """interval 1..7 x 1..40 stored steps x rings of 4..64 slots (chunk_steps as planned for each) x both destinations."""
    sims = [Sim(line).check() for line in driver("sweep")]
    assert len(sims) == 5 * 7 * 40 * 2
    seen = set()
    for s in sims:
        p = s.p
        seen.add((p["ring"], p["interval"], p["n_saved"], p["direct"]))
        per_chunk = 300 // p["interval"] if p["direct"] else min(300 // p["interval"], (p["ring"] - 2) // 2)
        assert p["chunk_steps"] == max(per_chunk, 1) * p["interval"]
        assert s.chunks == _earlier_trickle_chunks(p["n_saved"], p["interval"], p["ring"], p["chunk_steps"], p["direct"])
    assert len(seen) == len(sims)


OTHER_DELIVERIES = [
    # the half-step kernels forward nothing: sub-chunks through staging
    ("half_steps_1mb_25_stored", dict(step_bytes=S2050, n_saved=25, subchunk_mb=1, full_step=0),
     "mode=subchunks ask_pinned=0 direct=0 sub_saved=1 n_sub=25 ring=0 chunk_steps=0 acc_entries=25 half_bytes=524800 ring_bytes=0 need_host_ring=1 slice_bytes=0",
     ",".join("%d:%d" % (c, c + 1) for c in range(25))),
    ("half_steps_32mb_25_stored_pinned", dict(step_bytes=S2050, n_saved=25, full_step=0, pinned=1),
     "mode=subchunks ask_pinned=0 direct=0 sub_saved=4 n_sub=7 ring=0 chunk_steps=0 acc_entries=25 half_bytes=2099200 ring_bytes=0 need_host_ring=1 slice_bytes=0",
     "0:4,4:8,8:12,12:16,16:20,20:24,24:25"),
    ("trickle_knob_0", dict(step_bytes=S2050, n_saved=25, interval=2, trickle=0),
     "mode=subchunks ask_pinned=0 direct=0 sub_saved=4 n_sub=7 ring=0 chunk_steps=0 acc_entries=50 half_bytes=2099200 ring_bytes=0 need_host_ring=1 slice_bytes=0",
     "0:4,4:8,8:12,12:16,16:20,20:24,24:25"),
    # 518 x 5 fp32: 10 360-byte steps, a multiple of 8 and not of 16 -- the launches cannot forward them
    ("step_bytes_no_multiple_of_16", dict(step_bytes=10360, n_saved=9, interval=2),
     "mode=subchunks ask_pinned=0 direct=0 sub_saved=2 n_sub=5 ring=0 chunk_steps=0 acc_entries=18 half_bytes=20720 ring_bytes=0 need_host_ring=1 slice_bytes=0",
     "0:2,2:4,4:6,6:8,8:9"),
    ("3_chains_half_steps", dict(step_bytes=S2050, n_saved=1000, chains=3, full_step=0),
     "mode=subchunks ask_pinned=0 direct=0 sub_saved=21 n_sub=48 ring=0 chunk_steps=0 acc_entries=3000 half_bytes=33062400 ring_bytes=0 need_host_ring=1 slice_bytes=0",
     None),
    # nothing stored: the steps run as one sub-chunk
    ("no_chain_out", dict(step_bytes=S2050, n_saved=25, interval=4, chain_out=0),
     "mode=nothing ask_pinned=0 direct=0 sub_saved=25 n_sub=1 ring=0 chunk_steps=0 acc_entries=100 half_bytes=0 ring_bytes=0 need_host_ring=1 slice_bytes=0",
     "0:25"),
]


@pytest.mark.parametrize("name,args,plan,subchunks", OTHER_DELIVERIES, ids=[c[0] for c in OTHER_DELIVERIES])
def test_delivery_without_forwarding(driver, name, args, plan, subchunks):
    out = driver("chain", **args)
    assert _fields(out[0]) == _fields(plan)
    if subchunks is not None:
        assert out[1] == "subchunks=" + subchunks


# ---- the sub-chunk path ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("budget,stored_step_bytes,n_saved,want", [
    (1 << 20, 4 << 20, 100, 1),          # a budget smaller than a step: one step all the same
    (32 << 20, S2050, 100, 13),          # 63 would fit; an eighth of the run (rounded up) bounds it
    (32 << 20, S2050, 1000, 63),         # the budget bounds it
    (32 << 20, 3 * S2050, 1000, 21),     # three chains: a stored step is three ensembles
    (32 << 20, S2050, 1, 1),
])
def test_stored_steps_per_subchunk(driver, budget, stored_step_bytes, n_saved, want):
    assert driver("subchunk", budget=budget, stored_step_bytes=stored_step_bytes, n_saved=n_saved) == [str(want)]


def test_offsets_of_chain_2_of_3(driver):
    """Steps of 1000 bytes, 12 stored steps in sub-chunks of 5: chain 2's steps [5, 10) lie 2 x 12 + 5 steps into the caller's
    array and 2 x 5 steps into staging; the last sub-chunk (2 steps) uses two whole chain strides of a half and 2 steps."""
    got = _fields(driver("offsets", step_bytes=1000, sub_saved=5, n_saved=12, first=5, count=5, k=2, now=2, chains=3)[0])
    assert got == dict(dst="29000", src="10000", bytes="5000", chain_offset="10000", half_used="12000")
    got = _fields(driver("offsets", step_bytes=1000, sub_saved=5, n_saved=12, first=10, count=2, k=0, now=2, chains=1)[0])
    assert got == dict(dst="10000", src="0", bytes="2000", chain_offset="0", half_used="2000")


# ---- split runs -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step_bytes,n_saved,want", [
    (131072 * 64 * 8, 10, 4),   # 64 MiB steps: 256 MiB hold four
    (131072 * 64 * 8, 2, 2),    # at most the run's
    (300 << 20, 5, 1),          # at least one
])
def test_split_staging_slots(driver, step_bytes, n_saved, want):
    assert driver("split_stage", step_bytes=step_bytes, n_saved=n_saved) == [str(want)]


@pytest.mark.parametrize("args,want", [
    (dict(total=1000, compact=1, learning=1), [16, 256, 256, 256, 216]),                        # learning: a short first chunk
    (dict(total=1000, compact=1), [256, 256, 256, 232]),
    (dict(total=1000, compact=1, compact_chunk=64, learning=1), [16] + [64] * 15 + [24]),
    (dict(total=1000), [1000]),                                                                 # whole slices, nothing stored: one chunk
    (dict(total=600, compact=1, stores=1, stage_slots=100), [100] * 6),                         # the staging buffer fills inside a compact chunk
    (dict(total=700, compact=1, stores=1, stage_slots=300), [256, 256, 188]),
    (dict(total=600, compact=1, learning=1, stores=1, interval=3, stage_slots=50), [16, 149, 150, 150, 135]),  # a chunk that starts inside an interval
    (dict(total=70, stores=1, interval=7, stage_slots=4), [28, 28, 14]),                        # whole slices: a staging buffer per chunk
])
def test_split_chunk_lengths(driver, args, want):
    assert driver("split_chunks", **args) == ["chunks=" + ",".join(map(str, want))]


@pytest.mark.parametrize("args,want", [
    (dict(cap_full=4096, max_count=0), dict(cap_set="0", first="4096", next="64")),
    (dict(cap_full=4096, max_count=1000), dict(cap_set="0", first="4096", next="1216")),        # 1000 + 125 + 64 = 1189, rounded up to 64
    (dict(cap_full=4096, max_count=4000), dict(cap_set="0", first="4096", next="4096")),        # 4564 reaches cap_full
    (dict(cap_full=4096, learned=1216, max_count=960), dict(cap_set="0", first="1216", next="1152")),
    (dict(cap_full=4096, learned=5000), dict(cap_set="0", first="4096", next="64")),
    (dict(cap_full=4096, knob=512, learned=1216), dict(cap_set="512", first="512", next="64")),
    (dict(cap_full=4096, knob=10000), dict(cap_set="4096", first="4096", next="64")),
    (dict(cap_full=4096, knob=512, compact=0), dict(cap_set="512", first="4096", next="64")),   # whole slices: blocks are not used
])
def test_split_slot_bound(driver, args, want):
    assert _fields(driver("cap", **args)[0]) == want


# ---- simulated split runs ---------------------------------------------------------------------------------------------------
# (cap_full 200, 5 fp64 dimensions, 4 ranks: a block of 200 slots is 10 416 bytes, one of 192 slots 10 000, one of 128 slots 6 672, one of 64 slots 3 344)

SPLIT_SIMS = [
    # a learning run that stores every 3rd step into two staging slots; the second chunk overflows once
    (dict(total=12, interval=3, compact=1, compact_chunk=4, stores=1, stage_slots=2, cap_full=200, overflow="1", max_counts="50,10"),
     "C 0 6 200 | X 0 0 | X 1 1 | X 2 2 | S 2 0 | X 3 3 | X 4 4 | X 5 5 | S 5 1 | K 50 128 | H 0 2 | "
     "C 6 4 128 | X 6 6 | X 7 7 | X 8 8 | S 8 0 | X 9 9 | R 6 | "
     "C 6 4 200 | X 6 6 | X 7 7 | X 8 8 | S 8 0 | X 9 9 | K 10 128 | H 2 3 | "
     "C 10 2 128 | X 10 10 | X 11 11 | S 11 0 | K 10 128 | H 3 4 | "
     "end rollbacks=1 cap_slots=128 cap_to_keep=128 samples=12 bytes_per_step=29376"),   # (6 x 10416 + 4 x 10416 + 2 x 6672) x 3 / 12
    # held, repeated, held, repeated: a bound of the last run, nothing stored, half-step scheme (two exchanges per step)
    (dict(total=10, compact=1, compact_chunk=3, learned=64, cap_full=200, full_step=0, overflow="1,4", max_counts="0,100,0,0"),
     "C 0 3 64 | X 0 0 | X 1 1 | X 2 2 | K 0 64 | C 3 3 64 | X 3 3 | X 4 4 | X 5 5 | R 3 | C 3 3 200 | X 3 3 | X 4 4 | X 5 5 | K 100 192 | "
     "C 6 3 192 | X 6 6 | X 7 7 | X 8 8 | K 0 64 | C 9 1 64 | X 9 9 | R 9 | C 9 1 200 | X 9 9 | K 0 64 | "
     "end rollbacks=2 cap_slots=64 cap_to_keep=64 samples=10 bytes_per_step=%.17g" % ((3 * 3344 + 3 * 10416 + 3 * 10000 + 1 * 10416) * 2 * 3 / 10)),
    # whole slices, another rank stores: the chunks end where that rank's staging buffer is full, this one stages nothing
    (dict(total=70, interval=7, any_rank_stores=1, stage_slots=4, shard_count=100),
     "C 0 28 4096 | " + "".join("X %d %d | " % (k, 2 * k) for k in range(14)) + "K 0 4096 | C 28 28 4096 | " + "".join("X %d %d | " % (k, 2 * k) for k in range(14, 28))
     + "K 0 4096 | C 56 14 4096 | " + "".join("X %d %d | " % (k, 2 * k) for k in range(28, 32)) + "K 0 4096 | "
     "end rollbacks=0 cap_slots=0 cap_to_keep=0 samples=32 bytes_per_step=28800"),     # 3 x 100 x 2 x (5 + 1) x 8
]


@pytest.mark.parametrize("args,want", SPLIT_SIMS, ids=["learning_stores_one_repeat", "mixed_held_and_repeated", "whole_slices_another_rank_stores"])
def test_split_window_simulated_runs(driver, args, want):
    assert driver("split_sim", **args) == [want]


def _next_cap(max_count, cap_full):
    """split_next_cap, from the arithmetic run_split held: what the chunk needed, an eighth and 64 more, in whole 64s"""
    want = (max_count + max_count // 8 + 64 + 63) // 64 * 64
    return np.minimum(want, cap_full)


def _block_bytes(cap, dims, elem):
    a16 = lambda b: (b + 15) // 16 * 16
    return 16 + a16(cap * 4) + a16(cap * elem) + a16(cap * dims * elem)


def test_split_window_over_a_sweep(driver):
    """Every schedule of: 1..60 steps x interval 1..7 (total // interval stored steps) x compact_chunk 3, 4, 7, 256 x 1, 2, 4 or
    n_saved staging slots x {nobody stores, this rank stores, only another rank does} x {whole slices; moved rows with the bound set
    by the knob or learned, and the first try of no chunk, of every chunk, of every 2nd or of every 3rd chunk overflowing}.  The
    driver plays each through SplitWindow as run_split does and writes rows of 12 integers (run_plan_cases.cpp: sweep_one); the
    properties are checked here over all of them at once."""
    exe = os.path.join(BUILD, "run_plan_cases")  # (built by the fixture; this case's output is binary)
    rows = np.frombuffer(subprocess.run([exe, "split_sweep"], capture_output=True, check=True).stdout, dtype=np.int32).reshape(-1, 12).astype(np.int64)
    kind, sid = rows[:, 0], rows[:, 1]
    H, E = rows[kind == 0], rows[kind == 3]
    S = len(H)
    assert (H[:, 1] == np.arange(S)).all() and (E[:, 1] == np.arange(S)).all()
    total, interval, compact, chunk, slots, any_stores, stores, knob, pattern, cap_full = (H[:, c] for c in range(2, 12))
    # the sweep is the one the docstring states: whole slices 60 x 7 x (1 + 2 x 4), moved rows 60 x 7 x 8 x 4 x (1 + 2 x 4)
    assert S == 60 * 7 * 9 + 60 * 7 * 8 * 4 * 9
    assert set(zip(total, interval)) == {(t, i) for t in range(1, 61) for i in range(1, 8)}
    assert set(chunk[compact == 1]) == {3, 4, 7, 256} and set(pattern[compact == 1]) == {0, 1, 2, 3} and set(knob[compact == 1]) == {0, 96}
    assert set(pattern[compact == 0]) == {0} and set(cap_full) == {200}
    n_stored = np.where(stores == 1, total // interval, 0)
    assert set(slots[any_stores == 1] - np.maximum(total // interval, 1)[any_stores == 1]) >= {0} and {1, 2, 4} <= set(slots)

    T = rows[kind == 1]
    t_sid, s0, length, cap, failed, smp_before, smp_after, staged, left, max_count, cap_next = (T[:, c] for c in range(1, 12))
    end = s0 + length
    same = t_sid[1:] == t_sid[:-1]  # a try and the next one belong to the same run
    assert (length >= 1).all() and (end <= total[t_sid]).all()

    # the held chunks cover [0, total) exactly once, in order
    held = failed == 0
    h_sid, h_s0, h_end = t_sid[held], s0[held], end[held]
    first = np.r_[True, h_sid[1:] != h_sid[:-1]]
    last = np.r_[h_sid[1:] != h_sid[:-1], True]
    assert (h_sid[first] == np.arange(S)).all(), "every run has held chunks, and the runs come in order"
    assert (h_s0[first] == 0).all() and (h_end[last] == total).all()
    assert (h_s0[1:] == h_end[:-1])[~first[1:]].all()

    # a repeated try covers the same steps as the failed one, with blocks of cap_full slots, and holds
    f = np.flatnonzero(failed == 1)
    assert len(f) > 100000 and (compact[t_sid[f]] == 1).all()
    assert same[f].all() and (s0[f + 1] == s0[f]).all() and (length[f + 1] == length[f]).all() and (cap[f + 1] == cap_full[t_sid[f]]).all() and (failed[f + 1] == 0).all()
    # ... the sample count is restored by it (and never exceeds 32), nothing of the failed try stays staged
    assert (smp_before[f + 1] == smp_before[f]).all() and (smp_after[f + 1] == smp_after[f]).all()
    assert (smp_after <= 32).all() and (smp_after >= smp_before).all() and (left[f] == 0).all()
    h = np.flatnonzero(held)
    carries = h[:-1][t_sid[h[:-1] + 1] == t_sid[h[:-1]]]
    assert (smp_before[carries + 1] == smp_after[carries]).all()
    stride = np.where(total > 32, total // 32, 1)
    assert (E[:, 6] == np.minimum(32, (total + stride - 1) // stride)).all()
    # rollbacks counts the failed tries: those the pattern asked for
    assert (E[:, 2] == np.bincount(t_sid[f], minlength=S)).all()
    n_chunks = np.bincount(h_sid, minlength=S)
    assert (E[:, 2] == np.where(pattern > 0, n_chunks // np.maximum(pattern, 1), 0)).all()

    # the bound: whole slices never use one; moved rows start with the set bound, or -- learning -- with whole-slice blocks and
    # at most 16 steps; behind a held chunk it is the set bound or split_next_cap of what the chunk reported
    first_try = np.r_[True, ~same]
    assert (cap[compact[t_sid] == 0] == 200).all() and (E[:, 3][compact == 0] == 0).all()
    learning_run = (compact == 1) & (knob == 0)
    assert (cap[first_try] == np.where(compact == 0, 200, np.where(knob > 0, 96, 200))[t_sid[first_try]]).all()
    learning = (s0 == 0) & learning_run[t_sid]  # (the tries of the first chunk of a run that knows no bound)
    assert (length[learning] <= 16).all() and (cap[learning] == 200).all()
    later = (compact[t_sid] == 1) & ~learning
    assert (length[later] <= chunk[t_sid][later]).all()
    hc = held & (compact[t_sid] == 1)
    assert (cap_next[hc] == np.where(knob[t_sid[hc]] > 0, 96, _next_cap(max_count[hc], 200))).all()
    assert (cap[carries + 1] == cap_next[carries]).all(), "the next chunk runs with the bound the held one left"
    assert (cap_next[f] == 200).all()
    last_try = np.r_[~same, True]
    assert (E[:, 3][compact == 1] == cap_next[last_try][compact == 1]).all()                                # cap_slots
    assert (E[:, 4][learning_run] == _next_cap(max_count[last_try], 200)[learning_run]).all()              # the bound to keep
    assert (E[:, 4][~learning_run] == 0).all()

    # staging: never more than stage_slots steps staged, nothing without `stores`, nothing left behind a chunk of moved rows
    assert (staged <= slots[t_sid]).all() and (staged >= 0).all() and (staged[stores[t_sid] == 0] == 0).all()
    assert (left[compact[t_sid] == 1] == 0).all() and (left < np.maximum(slots[t_sid], 1)).all()
    # every stored step is handed out exactly once, in order, and only behind a held chunk that completed it
    at = np.flatnonzero(kind == 2)
    G = rows[at]
    g_sid, g_from, g_to = G[:, 1], G[:, 2], G[:, 3]
    g_first = np.r_[True, g_sid[1:] != g_sid[:-1]]
    g_last = np.r_[g_sid[1:] != g_sid[:-1], True]
    assert (np.unique(g_sid) == np.flatnonzero(n_stored > 0)).all()
    assert (g_from[g_first] == 0).all() and (g_to[g_last] == n_stored[g_sid[g_last]]).all() and (g_to > g_from).all()
    assert (g_from[1:] == g_to[:-1])[~g_first[1:]].all()
    before = rows[at - 1]
    assert (before[:, 0] == 1).all() and (before[:, 1] == g_sid).all() and (before[:, 5] == 0).all()
    assert (g_to == (before[:, 2] + before[:, 3]) // interval[g_sid]).all() and (g_to - g_from <= slots[g_sid]).all()

    # for a given any_rank_stores the cuts do not depend on whether this rank stores (the driver puts the two side by side)
    mine, theirs = np.flatnonzero((any_stores == 1) & (stores == 1)), np.flatnonzero((any_stores == 1) & (stores == 0))
    assert (theirs == mine + 1).all() and (H[mine][:, [2, 3, 4, 5, 6, 9, 10]] == H[theirs][:, [2, 3, 4, 5, 6, 9, 10]]).all()
    cuts = [2, 3, 4, 5, 6, 7, 10, 11]
    a, b = T[np.isin(t_sid, mine)][:, cuts], T[np.isin(t_sid, theirs)][:, cuts]
    assert a.shape == b.shape and (a == b).all()

    # bytes_per_step x total: the sum of split_bytes_* over the held chunks (4 ranks, 5 fp64 dimensions; full-step scheme when total is odd)
    full = (total % 2)[h_sid]
    assert (E[:, 7] == total % 2).all()
    per_step = np.where(compact[h_sid] == 1, np.where(full == 1, 1, 2) * 3 * _block_bytes(cap[held], 5, 8), 3 * np.where(full == 1, 100, 200) * 2 * (5 + full) * 8)
    assert (E[:, 5] == np.bincount(h_sid, weights=(h_end - h_s0) * per_step, minlength=S).astype(np.int64)).all()


def test_split_bytes_received(driver):
    # 10 steps, 4 ranks: three blocks of 1000 bytes per exchange, one exchange per step (full-step kernels) or two
    assert _fields(driver("bytes", len=10, world=4, block_bytes=1000, full_step=1, shard_count=100, dims=64)[0]) == dict(compact="30000", whole="3120000")
    assert _fields(driver("bytes", len=10, world=4, block_bytes=1000, full_step=0, shard_count=100, dims=64)[0]) == dict(compact="60000", whole="3072000")
