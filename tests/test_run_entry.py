"""The run entry the three movers share, checked on the CPU: how the differential-evolution and the batch mover cut a run into
pieces (mcmcpp_amd/csrc/run_plan.hpp: plan_de_pieces, plan_batch_pieces) and which run() / run_device() call a handle refuses
(mcmcpp_amd/csrc/run_refusal.hpp).  The GPU suite reaches a piece boundary of the DE mover in one test and most refusals not at
all; a mistake here corrupts a stored chain or changes what a caller is told.

tests/cpp/run_entry_cases.cpp is compiled with the host compiler against the two headers alone (no HIP header: that it compiles
is an assertion).  The expected values are the rules DeSampler::run_steps, BatchSampler::run_to / run_steps and the six run
entries held inline before they moved into the headers, restated below."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

NONE, HOST, DEVICE = 0, 1, 2
E_ARG, E_UNSUPPORTED, E_STATE = 1, 4, 5


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "run_entry_cases")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "run_entry_cases.cpp"), "-I", CSRC])

    def run(what, **lists):
        args = ["%s=%s" % (k, ",".join(map(str, v))) for k, v in lists.items()]
        return subprocess.run([exe, what] + args, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return run


def test_the_headers_include_no_hip_header():
    text = open(os.path.join(CSRC, "run_refusal.hpp")).read()
    includes = [line.split()[1] for line in text.split("\n") if line.startswith("#include")]
    assert includes == ['"../../include/mcmcpp_hip.h"']  # (the C header of the ABI: <stdint.h> and <stddef.h> alone)


def test_the_movers_hold_no_size_rule():
    for name, gone in (("diffevo.hip", ("256 << 20", "64 << 20", "piece = ", "first += ")), ("batch.hip", ("stored_steps_per_subchunk", "n_sub = ", "chain_slot_base = -"))):
        text = open(os.path.join(CSRC, name)).read()
        for g in gone:
            assert g not in text, (name, g)


# ---- piece plans ----------------------------------------------------------------------------------------------------------------

def _earlier_de(step_bytes, n_saved, interval, dest, counters):
    """DeSampler::run_steps before the plan: (stored steps per piece, bytes of d_chain grown, entries of d_acc grown)."""
    piece = n_saved
    if counters:
        fit = (64 << 20) // (interval * 4)
        if piece > fit:
            piece = 1 if fit < 1 else fit
    chain_bytes = 0
    if dest == HOST:
        fit = (256 << 20) // step_bytes
        if piece > fit:
            piece = 1 if fit < 1 else fit
        chain_bytes = piece * step_bytes
    return piece, chain_bytes, piece * interval if counters else 0


def _earlier_batch(budget, step_bytes, n_saved, interval, dest, counters):
    """BatchSampler::run_to before the plan: (stored steps per sub-chunk, bytes of d_chain ensured, entries of d_acc ensured)."""
    sub_saved, chain_bytes = n_saved, 0
    if dest == HOST:
        sub_saved = max(min(budget // step_bytes, (n_saved + 7) // 8), 1)  # stored_steps_per_subchunk
        chain_bytes = step_bytes * sub_saved
    return sub_saved, chain_bytes, n_saved * interval if counters else 0


def _earlier_pieces(n_saved, piece):
    """Both movers' loops: pieces of `piece` stored steps from 0, the last one shorter.  (Neither loop ever saw a run of nothing:
    run returned before.  The plan has no piece for one.)  -> (number of pieces, piece 0, piece 1, the last piece)"""
    if n_saved == 0:
        return 0, (-1, -1), (-1, -1), (-1, -1)
    count = (n_saved + piece - 1) // piece
    at = lambda c: (c * piece, min((c + 1) * piece, n_saved))
    return count, at(0), at(1) if count > 1 else (-1, -1), at(count - 1)


# one stored step of 64 x 4 fp64, 518 x 5 fp32, 2050 x 32 fp64, 2050 x 1024 fp64 (15.98 of them are 256 MiB), and sizes that
# divide neither budget; 300 MiB: no stored step fits a piece
STEP_BYTES = [16, 24, 2048, 10360, 100003, 524800, 16793600, 32 << 20, 300 << 20]
N_SAVED = [0, 1, 2, 7, 9, 15, 16, 17, 65537, 10 ** 6]
# 2^24 is the first interval of which 64 MiB of counters hold exactly one stored step; above it the bound falls below one and
# clamps to one (10^7 still fits one whole)
INTERVAL = [1, 2, 3, 1000, 1 << 20, 10 ** 7, 1 << 24, (1 << 24) + 1, 3 * 10 ** 7]
BUDGET = [1 << 20, 32 << 20]


def _pair(text):
    a, b = text.split(":")
    return int(a), int(b)


def test_piece_plans_over_the_grid(driver):
    out = driver("pieces", step_bytes=STEP_BYTES, n_saved=N_SAVED, interval=INTERVAL, budget=BUDGET)
    assert dict(f.split("=") for f in out[-1].split()) == dict(device_piece_offset="15000", subchunk_slot_base="-6")
    seen = set()
    for line in out[:-1]:
        f = dict(kv.split("=") for kv in line.split())
        mover = f.pop("mover")
        p0, p1, last = _pair(f.pop("p0")), _pair(f.pop("p1")), _pair(f.pop("last"))
        f = {k: int(v) for k, v in f.items()}
        budget, step_bytes, n_saved, interval, dest, counters = (f[k] for k in ("budget", "step_bytes", "n_saved", "interval", "dest", "counters"))
        seen.add((mover, budget, step_bytes, n_saved, interval, dest, counters))
        if mover == "de":
            piece, chain_bytes, acc_entries = _earlier_de(step_bytes, n_saved, interval, dest, counters)
        else:
            piece, chain_bytes, acc_entries = _earlier_batch(budget, step_bytes, n_saved, interval, dest, counters)
        count, want0, want1, want_last = _earlier_pieces(n_saved, piece)
        got = (f["piece_saved"], f["chain_bytes"], f["acc_entries"], f["n_pieces"], p0, p1, last)
        assert got == (piece, chain_bytes, acc_entries, count, want0, want1, want_last), line
        # the pieces cover [0, n_saved) once and in order, none of them empty
        assert f["gaps"] == 0 and f["walk_end"] == n_saved, line
        assert n_saved == 0 or (p0[0] == 0 and f["shortest"] >= 1), line
        # no piece exceeds the buffers the plan says to grow
        assert f["longest"] <= f["piece_saved"], line
        if dest == HOST:
            assert f["longest"] * step_bytes <= f["chain_bytes"], line
        else:
            assert f["chain_bytes"] == 0, line
        if counters:
            assert (f["longest"] if mover == "de" else n_saved) * interval <= f["acc_entries"], line
        else:
            assert f["acc_entries"] == 0, line
        # one piece where nothing has to leave through a buffer of the handle's
        if n_saved > 0 and ((mover == "de" and dest == DEVICE and not counters) or (mover == "batch" and dest != HOST)):
            assert f["n_pieces"] == 1, line
    cases = len(STEP_BYTES) * len(N_SAVED) * len(INTERVAL) * 3 * 2
    assert len(out) - 1 == len(seen) == cases * (1 + len(BUDGET)) == 14580


def test_the_grid_reaches_every_bound(driver):
    """The grid is only worth its lines if each rule decides somewhere: both DE bounds, both clamps, the eighth rule and the budget."""
    de = {(s, n, i, d, c): _earlier_de(s, n, i, d, c)[0] for s, n, i, d, c in itertools.product(STEP_BYTES, N_SAVED, INTERVAL, (NONE, HOST, DEVICE), (0, 1))}
    assert de[(16793600, 17, 1, HOST, 0)] == 15          # 256 MiB of chain
    assert de[(16793600, 17, 1, DEVICE, 0)] == 17        # ... which a device destination does not have
    assert de[(16, 10 ** 6, 1000, DEVICE, 1)] == 16777   # 64 MiB of counters
    assert de[(16, 17, (1 << 24) + 1, NONE, 1)] == 1     # clamped: not one stored step's counters fit
    assert de[(300 << 20, 17, 1, HOST, 0)] == 1          # clamped: not one stored step fits
    assert _earlier_batch(32 << 20, 2048, 9, 2, HOST, 0)[0] == 2         # an eighth of the run
    assert _earlier_batch(1 << 20, 100003, 10 ** 6, 1, HOST, 0)[0] == 10  # the budget
    assert _earlier_batch(1 << 20, 32 << 20, 9, 1, HOST, 0)[0] == 1      # at least one


# ---- refusals -------------------------------------------------------------------------------------------------------------------

# What each entry point refused before there was one entry, in the order it checked.  (fact, the value that is refused, code)
_STATE_ARGS = [("have_state", 0, "no_state", E_STATE), ("bad_arguments", 1, "bad_arguments", E_ARG)]
_HALF = [("half_done", 1, "half_done", E_STATE)]
EARLIER = {
    # Sampler::run on a whole handle: check_run(whole_only = true)
    ("stretch", 0, 0): _STATE_ARGS + [("sharded", 1, "sharded", E_UNSUPPORTED)] + _HALF,
    # Sampler::run with a communicator: prepare_split, check_run(whole_only = false); its verdict goes through the all-reduce
    ("stretch", 0, 1): _STATE_ARGS + _HALF,
    # Sampler::run_device: the handles it is not for, then check_run (whose shard check can no longer fire)
    ("stretch", 1, 0): [("sharded", 1, "device_sharded", E_UNSUPPORTED)] + _STATE_ARGS + _HALF,
    ("stretch", 1, 1): [("communicator", 1, "device_with_communicator", E_UNSUPPORTED)],
    # DeSampler::run_steps (run_device checked the same two first)
    ("de", 0): _STATE_ARGS,
    ("de", 1): _STATE_ARGS,
    # BatchSampler::run_to
    ("batch", 0): [("callback_set", 0, "no_callback", E_STATE)] + _STATE_ARGS,
    ("batch", 1): [("callback_set", 0, "no_callback", E_STATE)] + _STATE_ARGS,
}


def test_refusals_for_every_combination_of_the_facts(driver):
    out = driver("refusals")
    seen = set()
    for line in out:
        f = dict(kv.split("=") for kv in line.split())
        mover, got, code = f.pop("mover"), f.pop("refusal"), int(f.pop("code"))
        f = {k: int(v) for k, v in f.items()}
        seen.add((mover,) + tuple(f[k] for k in ("to_device", "have_state", "callback_set", "communicator", "sharded", "half_done", "bad_arguments")))
        key = (mover, f["to_device"], f["communicator"]) if mover == "stretch" else (mover, f["to_device"])
        want = next(((name, c) for fact, bad, name, c in EARLIER[key] if f[fact] == bad), ("none", 0))
        assert (got, code) == want, line
        assert f["text"] == (got != "none"), line
        # only run() on a handle with a communicator must carry its verdict to the other ranks before it returns
        assert f["collective"] == (mover == "stretch" and f["communicator"] == 1 and f["to_device"] == 0), line
    # three movers x two entry points x 2^6 combinations of the facts
    assert len(out) == len(seen) == 3 * 2 * 64 == 384
