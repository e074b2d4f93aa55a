"""How diffevo.hip sizes the stream planner of the differential-evolution mover: mcmcpp_amd/csrc/de_batch_plan.hpp on the CPU.

tests/cpp/de_batch_plan_cases.cpp is compiled with the host compiler against the plan header alone (no HIP header: that it
compiles is an assertion) and prints the plan of every shape of a grid.  Checked here:
  * equality with a transcription of the arithmetic DeSampler::init and launch_boundary held inline before the header;
  * the 32-bit quantities of the device code: positions, scan positions, the resolver's keys q << 8 | e;
  * the LDS of a launch against the 64 KiB a launch may ask for without an attribute;
  * the table lengths against every index the three roles form;
  * the capacities against the number of bad positions a batch lists: a condition (8 binomial standard deviations above the
    mean), not a measurement;
  * the refusal: exactly where no half-step fits, and named after the bound that fired."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

NS = (2, 3, 4, 5, 7, 8, 63, 64, 65, 1000, 32768, 65536, 2 ** 20, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1)
DS = (1, 2, 3, 61, 62, 200, 509, 1021, 1022, 1024)
KNOBS = (None, 1, 3, 64, 1000)

# the planner's constants, as diffevo_kernel.hpp had them (test_constants pins the header's to these)
BATCH_MAX, SHIFT_MAX, WINDOW, OVERRUN, SEGMENTS, MAX_BAD, MAX_EVENTS, SCAN_RUN, THREADS = 64, 4095, 32, 255, 64, 8192, 1024, 8, 256
LDS_LIMIT = 65536


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "de_batch_plan_cases")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "de_batch_plan_cases.cpp"), "-I", CSRC])
    return exe


def parse(line):
    head, text = line.split(" text=")
    d = {k: int(v) for k, v in (f.split("=") for f in head.split())}
    d["text"] = text
    return d


def plans(exe, shapes):
    """{(n, D, knob, scan_run): plan} in one run of the driver"""
    text = "".join("%d %d %s %s\n" % (n, D, "-" if b is None else b, "-" if r is None else r) for n, D, b, r in shapes)
    out = subprocess.run([exe, "grid"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(shapes)
    return dict(zip(shapes, (parse(line) for line in out)))


@pytest.fixture(scope="module")
def grid(driver):
    return plans(driver, [(n, D, b, r) for n in NS for D in DS for b in KNOBS for r in (None, 1, 5)])


def inline_arithmetic(n, D, knob, scan_run):
    """DeSampler::init and launch_boundary as they were before de_batch_plan.hpp, line for line (C integer division on
    non-negative numbers is Python's //); None: the shape is refused"""
    scan_run = SCAN_RUN if scan_run is None else scan_run
    if scan_run < 1:
        scan_run = 1
    batch_max = BATCH_MAX if knob is None else knob
    per = D + 3
    b = 1 if batch_max < 1 else (BATCH_MAX if batch_max > BATCH_MAX else batch_max)
    by_positions = ((1 << 30) - 2 * (SHIFT_MAX + 1)) // (per * n)
    by_lists_num = MAX_BAD * 5 // 8 - 2 * (SHIFT_MAX + 1) // n
    assert by_lists_num >= 0  # (C truncates towards zero: the same as // only here)
    by_lists = by_lists_num // per
    by_records = (8 << 20) // n
    b = min(b, by_positions, by_lists, by_records)
    if b < 1:
        return None
    batch_max = b
    updates_max = batch_max * n
    positions_max = per * (updates_max - 1) + 2 * (SHIFT_MAX + 1)
    expected = positions_max // n + 1
    bad_capacity = 4 * ((expected + SEGMENTS - 1) // SEGMENTS) + 64
    cap = 2 * expected + 512
    resolve_capacity = MAX_BAD if cap > MAX_BAD else cap
    scan_blocks = ((positions_max + scan_run - 1) // scan_run + THREADS - 1) // THREADS
    scan_lanes = (positions_max + scan_run - 1) // scan_run
    want = dict(batch_max=batch_max, updates_max=updates_max, positions_max=positions_max, expected=expected, bad_capacity=bad_capacity, resolve_capacity=resolve_capacity,
                scan_blocks=scan_blocks, scan_lanes=scan_lanes, scan_run=scan_run, small_len=SHIFT_MAX + D + 2, lo_len=256, hi_len=(updates_max + 255) // 256, scan_lo_len=256,
                scan_hi_len=(scan_lanes + 255) // 256, threshold=(2 ** 64 - n) % n)
    # launch_boundary
    updates = n * batch_max
    positions = per * (updates - 1) + SHIFT_MAX + 1
    scan_positions = positions + SHIFT_MAX + 1
    resolve_lds = 4 * (resolve_capacity + 2 * per + 2 + SEGMENTS)
    records_lds = 8 * MAX_EVENTS
    want.update(updates=updates, positions=positions, scan_positions=scan_positions, seg_len=(scan_positions + SEGMENTS - 1) // SEGMENTS,
                record_blocks=(updates + THREADS - 1) // THREADS, resolve_lds=resolve_lds, records_lds=records_lds, lds_both=max(resolve_lds, records_lds),
                lds_resolve=resolve_lds, lds_records=records_lds, lds_scan=0)
    return want


def test_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "de_batch_plan.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<cstddef>", "<cstdint>"]
    # and diffevo.hip keeps no threshold of its own
    host = open(os.path.join(CSRC, "diffevo.hip")).read()
    for gone in ("by_positions", "by_lists", "kDeMaxBad", "kDeShiftMax + 1", "1LL << 30", "8LL << 20", "de_resolve_lds_bytes"):
        assert gone not in host, gone


def test_constants(driver):
    out = subprocess.run([driver, "constants"], capture_output=True, text=True, check=True).stdout
    assert {k: int(v) for k, v in (f.split("=") for f in out.split())} == dict(
        batch_max=BATCH_MAX, shift_max=SHIFT_MAX, window=WINDOW, overrun=OVERRUN, segments=SEGMENTS, count_stride=32, max_bad=MAX_BAD, max_events=MAX_EVENTS,
        scan_run=SCAN_RUN, threads=THREADS, record_updates=8 << 20, event_bytes=8)


def test_the_plan_is_the_inline_arithmetic(grid):
    refused = 0
    for (n, D, knob, run), p in grid.items():
        want = inline_arithmetic(n, D, knob, run)
        assert (want is not None) == bool(p["ok"]), (n, D, knob, run)
        if want is None:
            refused += 1
            continue
        assert {k: p[k] for k in want} == want, (n, D, knob, run)
    assert refused  # (the grid does reach the refusal)


def test_the_refusal_happens_exactly_where_no_half_step_fits(grid):
    for (n, D, knob, run), p in grid.items():
        bounds = {1: p["by_positions"], 2: p["by_lists"], 3: p["by_records"]}
        least = min(bounds.values())
        assert bool(p["ok"]) == (least >= 1), (n, D, knob)
        asked = 64 if knob is None else min(max(knob, 1), 64)
        if least < asked:  # the bound named is the one that is smallest
            assert bounds[p["bound"]] == least, (n, D, knob)
        else:
            assert p["bound"] == 0 and p["batch_max"] == asked
        if p["ok"]:
            assert p["batch_max"] == min(asked, least)
    # two walkers per half are cut by the lists, and refused from D = 1022 on for that reason and no other
    assert [grid[(2, D, None, None)].get("batch_max") for D in (200, 509, 1021)] == [5, 2, 1]
    for D in (1022, 1024):
        p = grid[(2, D, None, None)]
        assert not p["ok"] and p["bound"] == 2 and "lists" in p["text"] and "8 Mi updates" not in p["text"]
    p = grid[(2 ** 23 + 1, 1, None, None)]
    assert not p["ok"] and p["bound"] == 3 and "8 Mi updates" in p["text"]
    assert grid[(2 ** 23, 1, None, None)]["batch_max"] == 1
    p = grid[(2 ** 20, 1024, None, None)]
    assert not p["ok"] and p["bound"] == 1 and "2^30" in p["text"]


def test_device_integers_fit(grid):
    for key, p in grid.items():
        if not p["ok"]:
            continue
        n, D = key[0], key[1]
        per = D + 3
        assert 0 < p["positions"] < p["scan_positions"] == p["positions_max"] <= 2 ** 31 - 1, key
        assert p["updates"] == p["updates_max"] <= 2 ** 23, key  # (the walk's key: m << 8 | E with m < updates, never the ~0 that means "none")
        # a scanning lane forms t * run + i with t < scan_blocks * 256, i < run, in an int; its early exit compares in 64 bits
        assert p["scan_lanes"] * p["scan_run"] + p["scan_run"] <= 2 ** 31 - 1, key
        # resolver keys: q = p / per for p < positions, then q << 8 | e with e <= 255
        q_max = (p["positions"] - 1) // per
        assert ((q_max << 8) | 0xFF) < 2 ** 32, key
        # the lists: seg = p / seg_len < kDeSegments for every scanned p
        assert (p["scan_positions"] - 1) // p["seg_len"] < SEGMENTS, key
        assert 2 * SEGMENTS * p["bad_capacity"] * 8 < 2 ** 31, key


def test_lds_stays_within_a_plain_launch(grid):
    for key, p in grid.items():
        if p["ok"]:
            assert max(p["lds_both"], p["lds_resolve"], p["lds_records"]) <= LDS_LIMIT, key
            assert p["resolve_capacity"] <= MAX_BAD


def test_tables_cover_every_index(grid):
    for key, p in grid.items():
        if not p["ok"]:
            continue
        D = key[1]
        assert p["hi_len"] > (p["updates"] - 1) >> 8, key                      # jump_hi[mm >> 8], mm < updates
        assert p["scan_hi_len"] > (p["scan_lanes"] - 1) >> 8, key               # scan_hi[t >> 8], t a lane with a position
        assert p["lo_len"] == 256 and p["scan_lo_len"] == 256                      # [mm & 255], [t & 255]
        assert p["small_len"] > SHIFT_MAX and p["small_len"] > D, key              # jump_small[c], c <= kDeShiftMax; jump_small[dims]
        assert p["small_len"] > D  # the update kernel's jump_small[i0 + 1], i0 + 1 <= dims


def test_scan_lanes_past_the_table_leave_before_they_use_it(grid):
    """de_scan_lane loads scan_hi[t >> 8] BEFORE its early exit, for every lane of every scanning workgroup: the table must hold
    an entry for the last lane of the last workgroup, not only for the last lane with a position."""
    for key, p in grid.items():
        if p["ok"]:
            assert p["scan_hi_len"] > (p["scan_blocks"] * THREADS - 1) >> 8, key


def test_capacity_margins(grid):
    """B, the listed positions of a batch: binomial over scan_positions trials with probability 1 / n at a production threshold
    (n = 2: every second position; otherwise at most one in n plus the 2 threshold / 2^64 < 2^-33 of bounded_rand)."""
    worst = math.inf
    for key, p in grid.items():
        if not p["ok"]:
            continue
        n = key[0]
        trials, q = p["scan_positions"], 1.0 / n
        mean, sd = trials * q, math.sqrt(trials * q * (1 - q))
        for cap in (p["resolve_capacity"], SEGMENTS * p["bad_capacity"]):
            assert cap >= mean + 8 * sd, (key, cap, mean, sd)
            worst = min(worst, (cap - mean) / sd)
        mean1, sd1 = p["seg_len"] * q, math.sqrt(p["seg_len"] * q * (1 - q))
        assert p["bad_capacity"] >= mean1 + 8 * sd1, (key, mean1, sd1)
        worst = min(worst, (p["bad_capacity"] - mean1) / sd1)
    assert worst >= 8


def test_the_shapes_of_the_gpu_cases(driver):
    """what tests/test_de_planner.py and the end-to-end cases of tests/test_diffevo.py rely on"""
    p = plans(driver, [(2, 200, None, None), (3, 1021, None, None), (3, 1024, None, 5), (2, 1, None, None), (3, 1024, None, None)])
    assert p[(2, 200, None, None)]["batch_max"] == 5 and p[(2, 200, None, None)]["bound"] == 2
    assert p[(3, 1021, None, None)]["per"] == 1024 and p[(3, 1024, None, 5)]["per"] == 1027
    assert p[(3, 1024, None, 5)]["scan_positions"] % 5 != 0
    assert p[(2, 1, None, None)]["resolve_capacity"] == MAX_BAD
