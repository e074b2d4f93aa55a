"""The schedule of a tempered run (mcmcpp_amd/csrc/temper_plan.hpp), checked on the CPU, and what the GPU tests of
tests/test_run_tempered.py rest on that needs no device.

tests/cpp/temper_plan_cases.cpp is compiled with the host compiler against the plan header alone (no HIP header: that it
compiles is an assertion) and prints the pieces and rounds the header decides.  The Python side of the comparison is the loop of
HipSampler.run_exchanging / Ladder.run_exchanging, replayed on integers.

Also here: the input conditions of the tempered cases, from tests/replica_restatement.py alone, and the code-object metadata of
replica_cross_kernel in the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import replica_restatement as rr
from tests.test_kernel_metadata import _kernels_of_library
from tests.test_replica_exchange import _restated, _seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

# The tempered cases: K, W, D, calculator, dtype, n_saved, interval, exchange_every, rounds of the run, and the least and the
# most swaps any pair of any round accepts (the restatement's own counts, asserted below).
TEMPERED_CASES = {
    "A": (4, 600, 17, po.CALC_DENSE_GAUSSIAN, po.F64, 7, 1, 1, 7, 264, 471),
    "C": (2, 2054, 32, po.CALC_DENSE_GAUSSIAN, po.F64, 8, 1, 3, 2, 1004, 1004),  # (round 1 has no pair)
    "D": (16, 256, 20, po.CALC_DENSE_GAUSSIAN, po.F64, 4, 2, 2, 4, 132, 217),  # 8 slots, then 7
    "E": (3, 512, 7, po.CALC_ROSENBROCK, po.F64, 6, 2, 3, 4, 218, 346),  # exchange_every no multiple of interval
    "F": (4, 320, 2, po.CALC_SKEWED_GAUSSIAN_2D, po.F64, 6, 1, 1, 6, 183, 272),
    "G": (4, 600, 9, po.CALC_DENSE_GAUSSIAN, po.F32, 6, 1, 2, 3, 358, 443),  # rows of 36 bytes
    "G2": (2, 66, 1, po.CALC_DENSE_GAUSSIAN, po.F32, 6, 1, 2, 3, 42, 44),  # rows of 4 bytes
    "H": (2, 2050, 1024, po.CALC_ROSENBROCK, po.F64, 2, 1, 1, 2, 1040, 1040),
}


def restated_run(name):
    """The restatement's whole tempered run of a case, then its run(2): dict(chain [K][n_saved][W][D], acc [K][n_saved * interval],
    swaps, next: the next round, rounds: [(number, what Ladder.exchange returned)], state: Ladder.get_state() behind the tempered
    run, final_chain, final_acc: the run(2) behind it).  exchange_every counts ensemble steps: the restatement runs with interval
    1 and every interval-th step is taken."""
    K, W, D, calc, dtype, n_saved, interval, every = TEMPERED_CASES[name][:8]
    lad = _restated(K, W, D, calc, dtype, _seed_of(K))[0]
    rounds = []
    exchange = lad.exchange

    def recording(rnd, flip=False):
        r = exchange(rnd, flip)
        rounds.append((rnd, r))
        return r

    lad.exchange = recording
    chain, acc, swaps, nxt = lad.run_exchanging(n_saved * interval, interval=1, exchange_every=every)
    state = lad.get_state()
    final_chain, final_acc = lad.run(2)
    return dict(chain=chain[:, interval - 1::interval], acc=acc, swaps=swaps, next=nxt, rounds=rounds, state=state, final_chain=final_chain, final_acc=final_acc,
                near_ties=sum(o.near_ties for o in lad.orcs), redraws=sum(o.redraws for o in lad.orcs))


_RESTATED = {}


def restated_once(name):
    """restated_run(name), computed once per session and shared: nobody edits it"""
    if name not in _RESTATED:
        _RESTATED[name] = restated_run(name)
    return _RESTATED[name]


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "temper_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: temper_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "temper_plan_cases.cpp"), "-I", CSRC])
    return exe


def _out(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout


def _exchange_points(total, every, first_round):
    """run_exchanging's loop on integers: [(ensemble steps done when the round is made, its number)]"""
    points, rnd, done = [], first_round, 0
    while done < total:
        seg = min(every, total - done)
        done += seg
        if seg == every:
            points.append((done, rnd))
            rnd += 1
    return points


def test_the_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "temper_plan.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<stdint.h>", '"replica_plan.hpp"']
    assert " temper_plan.hpp " in open(os.path.join(CSRC, "Makefile")).read().split("HDRS")[1].split("\n")[0]


@pytest.mark.parametrize("first_round", [0, 5])
def test_pieces_and_rounds_equal_the_loop_of_run_exchanging(driver, first_round):
    lines = _out(driver, "pieces", first_round).strip().split("\n")
    seen = set()
    for line in lines:
        head, _, tail = line.partition(":")
        total, every, c1, c2, c3 = (int(v) for v in head.split())
        calls = [c for c in (c1, c2, c3) if c]
        assert sum(calls) == total
        seen.add((total, every, len(calls)))
        pieces = [tuple(int(v) for v in p.split("/")) for p in tail.split()]
        assert all(steps >= 1 for steps, _, _ in pieces) and sum(steps for steps, _, _ in pieces) == total
        # no piece crosses the end of an enqueue call
        ends, done = set(), 0
        for steps, _, _ in pieces:
            done += steps
            ends.add(done)
        assert set(np.cumsum(calls).tolist()) <= ends, line
        done, points = 0, []
        for steps, follows, rnd in pieces:
            assert done // every == (done + steps - 1) // every, line  # no piece crosses an exchange point
            done += steps
            assert follows == (done % every == 0), line
            if follows:
                points.append((done, rnd))
        assert points == _exchange_points(total, every, first_round), line
    assert seen == {(t, e, c) for t in range(1, 25) for e in range(1, 9) for c in (1, 2, 3) if t >= c}


@pytest.mark.parametrize("K", [2, 3, 16])
def test_rounds_that_pair_each_k(driver, K):
    for total, every, first in [(0, 1, 0), (7, 1, 0), (7, 1, 5), (8, 3, 0), (8, 3, 1), (12, 3, 4), (24, 5, 2**40 - 4), (5, 8, 3)]:
        got = [int(v) for v in _out(driver, "counts", total, every, first, K).split()]
        points = _exchange_points(total, every, first)
        assert got[0] == len(points) == total // every
        want = [sum(1 for _, r in points if (k, k + 1) in rr.pairs_of(K, r)) for k in range(K - 1)]
        assert got[1:] == want, (total, every, first, K)


def test_refusals(driver):
    def refusal(total, every, first, K):
        number, _, text = _out(driver, "refusal", total, every, first, K).strip().partition(" ")
        return int(number), text

    assert refusal(8, 2, 0, 4) == (0, "")
    assert refusal(8, 0, 0, 4)[0] == 1 and "exchange_every" in refusal(8, 0, 0, 4)[1]
    assert refusal(8, -3, 0, 4)[0] == 1
    assert refusal(8, 2, 0, 1)[0] == 2 and "num_chains must be at least 2" in refusal(8, 2, 0, 1)[1]
    assert refusal(8, 0, 0, 1)[0] == 1  # (the order of the checks)
    assert refusal(2, 1, 2**40 - 1, 2)[0] == 3 and "2^40" in refusal(2, 1, 2**40 - 1, 2)[1]
    assert refusal(1, 1, 2**40 - 1, 2)[0] == 0  # (round 2^40 - 1 is the last one)
    assert refusal(2, 2, 2**40 - 1, 2)[0] == 0
    assert refusal(5, 8, 2**40, 2)[0] == 0  # (no round: nothing is numbered)
    assert refusal(8, 8, 2**40, 2)[0] == 3
    assert refusal(0, 1, 2**64 - 1, 2)[0] == 3


def test_the_cases_meet_their_input_conditions():
    """From the restatement alone: in every case every pair of every round accepts between W/8 and W - W/8 swaps (the observed
    least and most are pinned too, so that a changed case cannot silently stop testing), and no round decides anything inside
    the near-tie band of the exchange (so that Python's log against fast_log cannot be a source of disagreement)."""
    for name, (K, W, D, calc, dtype, n_saved, interval, every, n_rounds, least, most) in TEMPERED_CASES.items():
        want = restated_once(name)
        rounds = want["rounds"]
        assert want["chain"].shape == (K, n_saved, W, D) and want["acc"].shape == (K, n_saved * interval)
        assert want["next"] == n_rounds == len(rounds) == n_saved * interval // every, name
        assert want["redraws"] == 0 and (dtype != po.F64 or want["near_ties"] == 0), name
        counts = []
        for rnd, r in rounds:
            assert not r["in_band"] and not r["near_ties"].any(), (name, rnd, r["in_band"])
            for a, _ in rr.pairs_of(K, rnd):
                assert r["proposed"][a] == W
                counts.append(int(r["accepted"][a]))
        assert counts and all(W // 8 <= c <= W - W // 8 for c in counts), (name, counts)
        assert (min(counts), max(counts)) == (least, most), (name, min(counts), max(counts))
        if name == "C":
            assert [len(rr.pairs_of(K, rnd)) for rnd, _ in rounds] == [1, 0]
        if name == "D":
            assert [len(rr.pairs_of(K, rnd)) for rnd, _ in rounds] == [8, 7, 8, 7]


def test_cross_kernels_are_all_there_without_static_lds_or_scratch(tmp_path):
    """replica_cross_kernel in the built library: one instantiation beside every calc_logp_kernel, in both element types, with
    no static LDS and no scratch memory (the rule of the step kernels: tests/test_kernel_metadata.py says why)."""
    kernels = _kernels_of_library(tmp_path)
    cross = sorted(k["name"].split("(")[0] for k in kernels if re.match(r"replica_cross_kernel<", k["name"]))
    calc = sorted(k["name"].split("(")[0] for k in kernels if re.match(r"calc_logp_kernel<", k["name"]))
    # (three calculators at the ten fp64 and nine fp32 lane mappings of build::make, the two-dimensional one at one each)
    assert len(cross) == 3 * (10 + 9) + 2 and cross ==[c.replace("calc_logp_kernel<", "replica_cross_kernel<") for c in calc]
    assert any(c.startswith("replica_cross_kernel<float") for c in cross) and any(c.startswith("replica_cross_kernel<double") for c in cross)
    offenders = [(k["name"][:100], k["lds"], k["scratch"]) for k in kernels if k["name"].startswith("replica_cross_kernel<") and (k["lds"] or k["scratch"])]
    assert not offenders, offenders[:6]
    # one swap kernel serves the rounds between runs and those inside a run
    swap = [k for k in kernels if k["name"].startswith("replica_swap_kernel<")]
    assert sorted(k["name"].split(">")[0] for k in swap) == ["replica_swap_kernel<double", "replica_swap_kernel<float"]
    assert not [k["name"] for k in kernels if "replica_swap_run_kernel" in k["name"]]
    assert all(k["scratch"] == 0 for k in swap)
