"""The replica-exchange rule of mcmcpp_amd/csrc/replica_plan.hpp, checked on the CPU.

tests/cpp/replica_plan_cases.cpp is compiled with the host compiler against the plan header alone (no HIP header: that it
compiles is an assertion) and prints what the header computes: the pairs of a round, the stream position of every draw, the
decision on a table of log-posteriors that includes every combination of finite, -inf, +inf and NaN, and the states its
two-level jump table reaches.  The Python side of every comparison is tests/replica_restatement.py and the oracle's pcg64.

The rule itself (same-index pairing with the stated delta) is checked for invariance on the restatement alone."""
import itertools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import replica_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "replica_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: replica_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replica_plan_cases.cpp"), "-I", CSRC])
    return exe


def _out(exe, *args, stdin=None):
    return subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, text=True, check=True).stdout


def test_the_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "replica_plan.hpp")).read()
    assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == ["<stdint.h>", '"canonical.hpp"', '"fast_log.hpp"', '"tie_eps.h"']
    kernels = open(os.path.join(CSRC, "replica_kernels.hpp")).read()
    assert '#include "replica_plan.hpp"' in kernels and "replica_accept(" in kernels and "replica_draw(" in kernels
    assert "fast_log(" not in kernels and "canonical(" not in kernels  # (the rule is the header's alone)
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " replica_plan.hpp " in makefile.split("HDRS")[1].split("\n")[0] and " replica_kernels.hpp " in makefile.split("HDRS")[1].split("\n")[0]


def test_each_adjacent_pair_lies_in_exactly_one_parity(driver):
    rows = [tuple(int(v) for v in line.split()) for line in _out(driver, "pairs").strip().split("\n")]
    for K in range(2, 17):
        seen = {}
        for r in (0, 1):
            mine = [(j, ka, slot) for (k_, r_, j, ka, slot) in rows if k_ == K and r_ == r]
            assert [(ka, ka + 1) for _, ka, _ in mine] == rr.pairs_of(K, r)
            assert [j for j, _, _ in mine] == list(range(len(mine)))  # slots in order, none skipped
            for j, ka, slot in mine:
                assert j == slot == ka >> 1 and 0 <= j < 8 and ka % 2 == r and ka + 1 < K
                assert ka not in seen
                seen[ka] = r
        assert sorted(seen) == list(range(K - 1))  # every adjacent pair, once
        for r in (2, 3):  # later rounds repeat the two parities
            assert [ka for (k_, r_, j, ka, slot) in rows if k_ == K and r_ == r] == [ka for (k_, r_, j, ka, slot) in rows if k_ == K and r_ == r - 2]


@pytest.mark.parametrize("W", [4, 66, 2054])
def test_draw_positions_are_distinct_and_as_stated(driver, W):
    rows = np.array([[int(v) for v in line.split()] for line in _out(driver, "positions", W).strip().split("\n")], dtype=object)
    assert len(rows) == 3 * 8 * W
    assert sorted(set(rows[:, 0])) == [0, 1, 2**40 - 1]
    for r, j, w, p in rows:
        assert p == (r * 8 + j) * W + w and p < 2**64
    assert len(set(rows[:, 3])) == len(rows)


def _bits(x):
    return "%x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def _decision_table():
    """draw, lp_aa, lp_bb, lp_ab, lp_ba: every combination of {finite, -inf, +inf, NaN} in the four log-posteriors (with two
    draws each), random finite cases, and finite cases built to lie exactly on and right beside the tie"""
    inf, nan = math.inf, math.nan
    rng = np.random.default_rng(7)
    cases = []
    for kinds in itertools.product((0, 1, 2, 3), repeat=4):
        for draw in (int(rng.integers(0, 2**64, dtype=np.uint64)), 2**64 - 1):
            fin = rng.standard_normal(4) * 3.0 - 5.0
            cases.append((draw,) + tuple((fin[i], -inf, inf, nan)[k] for i, k in enumerate(kinds)))
    for _ in range(400):
        cases.append((int(rng.integers(0, 2**64, dtype=np.uint64)),) + tuple(rng.standard_normal(4) * 2.0 - 40.0))
    for draw in (0, 1, 2**63, 2**64 - 1, 2**64 - 1025, 12345678901234567):
        cases.append((draw, -1.0, -2.0, -1.5, -2.5))
    for _ in range(100):  # delta = ln U up to the roundings of Python's log and of the sums: inside the band or a hair outside
        draw = int(rng.integers(0, 2**64, dtype=np.uint64))
        ln_u = math.log(1.0 - rr.canonical(draw))
        aa, bb, ab = rng.standard_normal(3) - 10.0
        ba = ln_u - (ab - aa) + bb
        cases.append((draw, aa, bb, ab, ba * (1.0 + float(rng.integers(-3, 4)) * 1e-12)))
    return cases


def test_replica_accept_equals_the_python_rule(driver):
    cases = _decision_table()
    text = "".join("%d %s %s %s %s\n" % (c[0], _bits(c[1]), _bits(c[2]), _bits(c[3]), _bits(c[4])) for c in cases)
    got = [tuple(int(v) for v in line.split()) for line in _out(driver, "accept", stdin=text).strip().split("\n")]
    assert len(got) == len(cases)
    in_band = ties_nonfinite = 0
    kinds = set()
    for c, (acc, tie) in zip(cases, got):
        want_acc, want_tie, ln_u, delta = rr.decide(*c)
        finite = all(math.isfinite(v) for v in c[1:])
        kinds.add(tuple("f" if math.isfinite(v) else str(v) for v in c[1:]))
        margin = abs(ln_u - delta)
        if not finite:
            # the non-finite rules: the comparison alone decides, and no such decision is a near tie
            assert (acc == 1) == want_acc == (ln_u < delta), c
            assert tie == 0 and not want_tie, c
            ties_nonfinite += tie
            if math.isnan(delta):
                assert acc == 0, c
            elif delta == math.inf:
                assert acc == 1, c
            elif delta == -math.inf:
                assert acc == 0, c
            continue
        # finite: outside the band the two logarithms cannot disagree; inside it both sides say "near tie" or the margin is
        # within a few ulp of the band's edge
        scale = abs(ln_u) + sum(abs(v) for v in c[1:])
        if margin > 2.0 * po.tie_eps(po.F64) * scale:
            assert (acc == 1) == want_acc and tie == 0 and not want_tie, c
        elif margin < 0.5 * po.tie_eps(po.F64) * scale:
            assert tie == 1 and want_tie, c
            in_band += 1
        else:
            assert (acc == 1) == want_acc, c  # (1e-12 relative is still thousands of ulp: the logarithms agree far better)
    assert len(kinds) == 4**4  # every combination was there
    assert in_band >= 20 and ties_nonfinite == 0


@pytest.mark.parametrize("seed,stream,W,rnd,slot", [(5, 0, 4, 0, 0), (40, 3, 66, 1, 7), (2**64 - 1, 2**63 + 5, 2054, 2**40 - 1, 3), (9, 0, 600, 3, 1)])
def test_the_jump_table_lands_where_the_engine_does(driver, seed, stream, W, rnd, slot):
    lines = _out(driver, "table", seed, stream, W, rnd, slot).strip().split("\n")
    entries, inc_hi, inc_lo = (int(v) for v in lines[0].split())
    assert entries == 64 + (W + 63) // 64
    g = po.Pcg64(seed, 2**64 - 1 - stream)
    assert g.inc == (inc_hi << 64) | inc_lo
    step = po.Pcg64(seed, stream)
    assert step.inc != g.inc  # (no step stream of the handle has this increment: theirs is the handle's own stream's)
    g.advance((rnd * 8 + slot) * W)
    for w in range(W):
        hi, lo, draw = (int(v) for v in lines[1 + w].split())
        assert g.next() == draw, w
        assert g.state == (hi << 64) | lo, w


@pytest.mark.parametrize("W,D,elem,vec_ok,want_lanes,want_units", [
    (320, 2, 8, 1, 1, 1), (66, 1, 4, 0, 1, 1), (600, 9, 4, 0, 16, 9), (600, 17, 8, 0, 32, 17), (2054, 32, 8, 1, 16, 16), (2050, 1024, 8, 1, 64, 512),
    (100, 1023, 8, 0, 64, 1023), (256, 20, 8, 1, 16, 10)])
def test_the_launch_shape_covers_every_walker_and_every_piece(driver, W, D, elem, vec_ok, want_lanes, want_units):
    lanes, units, unit_bytes, per_block, gx, gy = (int(v) for v in _out(driver, "shape", W, D, elem, vec_ok, 5).split())
    assert (lanes, units) == (want_lanes, want_units) and gy == 5
    assert units * unit_bytes == D * elem and unit_bytes == (16 if vec_ok else elem)
    assert lanes & (lanes - 1) == 0 and 1 <= lanes <= 64 and per_block * lanes == 256
    assert (gx - 1) * per_block < W <= gx * per_block
    assert lanes >= min(units, 64) and (lanes == 1 or lanes // 2 < units)  # short rows share a wavefront, no idle half


# ---- the rule leaves every rung's target invariant ------------------------------------------------------------------------

def _variance_statistic(seed, mode):
    """max over rungs and parameters of |var_hat / var_true - 1|; mode: 'none' (no exchanges), 'rule', 'flipped'"""
    K, W, D, burn, stored = 3, 128, 3, 100, 400
    betas = (1.0, 0.5, 0.25)
    a = np.random.default_rng(11).standard_normal((D, D))
    P = a @ a.T / D + np.eye(D)
    lad = rr.Ladder(W, D, po.CALC_DENSE_GAUSSIAN, [(b * P).ravel() for b in betas], seed)
    pos = np.stack([po.init_positions(po.F64, W, D, salt=seed * 8 + k) for k in range(K)])
    lad.set_state(pos, np.stack([lad.logp(k, pos[k]) for k in range(K)]))
    chains, rnd = [], 0
    for step in range(burn + stored):
        c, _ = lad.run(1, threads=1)
        if mode != "none":
            lad.exchange(rnd, flip=(mode == "flipped"))
            rnd += 1
        if step >= burn:
            chains.append(c[:, 0])
    x = np.stack(chains, axis=1)  # [K][stored][W][D]
    worst = 0.0
    for k in range(K):
        var_true = np.diag(np.linalg.inv(betas[k] * P))
        var_hat = x[k].reshape(-1, D).var(axis=0)
        worst = max(worst, float(np.max(np.abs(var_hat / var_true - 1.0))))
    return worst


def test_the_exchange_rule_leaves_every_rung_invariant():
    """K = 3 dense D = 3 rungs (beta = 1, .5, .25), W = 128, 100 burn-in + 400 stored steps, a round after every step, seeds 1..5,
    on the restatement alone.  The statistic is max over rungs and parameters of |var_hat / var_true - 1| with
    var_true = diag((beta_k P)^-1); the yardstick is the largest value the same seeds show WITHOUT exchanges (the oracle's
    unmodified behaviour), times 2 because five seeds give a coarse maximum.

    Recorded: without exchanges the five seeds give 0.032, 0.026, 0.035, 0.051, 0.041 (maximum 0.051, bound 0.102); with the
    rule 0.016, 0.034, 0.018, 0.018, 0.014 (maximum 0.034); with the sign of delta flipped 1.94, 1.76, 1.84, 1.79, 1.80: every
    seed breaks the bound at this size, so the run did not have to be enlarged."""
    seeds = (1, 2, 3, 4, 5)
    none = [_variance_statistic(s, "none") for s in seeds]
    rule = [_variance_statistic(s, "rule") for s in seeds]
    flipped = [_variance_statistic(s, "flipped") for s in seeds]
    print("without exchanges", none, "rule", rule, "flipped", flipped)
    bound = 2.0 * max(none)
    assert max(rule) <= bound, (rule, none)
    assert max(flipped) > bound, (flipped, none)
