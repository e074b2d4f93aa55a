"""replica_swap_kernel (mcmcpp_amd/csrc/replica_kernels.hpp) alone, on crafted arrays.

tests/test_replica_exchange.py reaches the kernel through a sampler handle, which fixes W (even, above 2 D), the alignment and the
padding, and makes every log-posterior the calculator's own finite value.  Here tests/cpp/replica_device.hip -- a program of its
own, linked with the production replica.hip -- launches the kernel once per case on inputs this module writes, and everything it
writes back (positions with a guard in front and behind, log-posteriors with their padding, all 15 count records, which lie
by the lower chain of a pair) is compared with
tests/replica_restatement.swap_arrays as integer views, bit for bit.  There is no tolerance anywhere.

How the crafted cases work.  The restatement's stream gives every (slot, walker) its draw and Python's ln U; the stored
log-posteriors and lp_ba are random, and lp_ab is set so that delta lies a chosen margin above ln U (accept) or below it (reject),
the margins spread from 1e-6 (fp32 elements: 1e-3, above the rounding of lp_ab) to 2.  The wanted decisions are random bits with
the last walker and walker 1 accepting and walker 0 rejecting, so accepted and rejected walkers interleave inside a wavefront
and a device draw that is not the stream's flips about half of the decisions of its slot.

The kernel is the one of the rounds between runs and of the rounds inside a tempered run.  The moved cases give it what only
the latter pass: a moved_bit, and every chain's n_accept words behind its log-posteriors at the two offsets of a sampler's buffers
(ChainGeometry: [W | W | W words], the ensemble in the first half or in the second).

  CPU   the driver compiles for gfx950; the row table against replica_shape (tests/cpp/replica_plan_cases.cpp); the conditions
        on the inputs, from the restatement alone; the restatement's split into swap_arrays and exchange_arrays.
  GPU   one child process runs every case (a module-scoped fixture, under a time limit of its own).

What a deliberately wrong kernel does to this module is listed in DESIGN section 4 (replica_swap_kernel)."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import replica_restatement as rr
from tests import test_exchange_kernels as xk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

PATTERN = 0xA5
GUARD = 16384       # bytes in front of and behind the positions: two of the longest rows (1024 x 8 bytes)
BLOCK = 256         # kReplicaBlockThreads
CHILD_LIMIT = 60    # seconds for the child run of all cases; measured on an MI355X: 0.2 to 0.7 s in the program, 0.3 s around it
RECORDS = 15        # kReplicaCountRecords: a count record per lower chain of a pair
MOVED_BIT = 0x80000000  # kRowMovedBit
NACC_GUARD = 64     # bytes of BLOCK_PATTERN behind a chain's n_accept words
BLOCK_PATTERN = 0x5A  # around the log-posteriors and n_accept of a moved case: no word of it has MOVED_BIT, so a stray `|=` shows
UINT = {4: np.uint32, 8: np.uint64}
FLOAT = {4: np.float32, 8: np.float64}
FILL = {4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}

# ---- rows: (D, element bytes) -> (16-byte pieces?, units, lanes per walker pair, trips of the busiest lane) with aligned buffers.
# The table of tests/test_exchange_kernels.py (replica_shape makes the same lanes and trips from it) and two rows that fill a
# 64-lane group only in part.
ROWS = dict(xk.ROWS)
ROWS[(66, 8)] = (True, 33, 64, 1)    # 33 pieces: the smallest row on 64 lanes, 31 of them idle
ROWS[(200, 4)] = (True, 50, 64, 1)   # 50 pieces, 14 lanes idle
MISALIGNED = {(2, 8): (False, 2, 2, 1), (4, 4): (False, 4, 4, 1)}  # a whole number of pieces on a base 8 bytes off: vec_ok = 0


def _t(elem):
    return "f64" if elem == 8 else "f32"


# ---------------------------------------------------------------------------------------------------------------- inputs

def _draws(seed, stream, rnd, pairs, W):
    """[pairs][W] raw outputs: po.Pcg64 advanced with Python integers"""
    out = np.zeros((pairs, W), np.uint64)
    for j in range(pairs):
        g = po.Pcg64(seed, 2**64 - 1 - stream)
        g.advance((rnd * rr.SLOTS + j) * W)
        for w in range(W):
            out[j, w] = g.next()
    return out


def _named_cells(K, W, D, elem):
    """every cell names its chain, walker and column"""
    k, w, c = np.meshgrid(np.arange(K, dtype=np.uint64), np.arange(W, dtype=np.uint64), np.arange(D, dtype=np.uint64), indexing="ij")
    cells = (k << np.uint64(40)) | (w << np.uint64(16)) | c if elem == 8 else (k << np.uint64(27)) | (w << np.uint64(11)) | c
    return cells.astype(UINT[elem])


def _split_f32(x):
    """(ab, ba, aa) in fp32 with (ab - aa) + ba == x in double arithmetic: 24 + 24 + 5 bits of x"""
    ab = np.float32(x)
    r1 = x - float(ab)
    ba = np.float32(r1)
    aa = np.float32(-(r1 - float(ba)))
    return ab, ba, aa


def make_case(name, elem, K, W, D, first_chain=0, pairs=None, vec_ok=None, offset=0, pad=0, seed=1, stream=0, rnd=0, kind="crafted", planted=(), named=None):
    """kind: 'crafted' (above), 'nonfinite' (one combination of {finite, -inf, +inf, NaN} per walker, nothing crafted);
    planted: (slot, walker) made exact ties of Python's own logarithm"""
    pairs = (K - first_chain) // 2 if pairs is None else pairs
    fits = (D * elem) % 16 == 0 and offset % 16 == 0
    vec_ok = int(fits) if vec_ok is None else vec_ok
    assert not vec_ok or fits
    t, u = FLOAT[elem], UINT[elem]
    rng = np.random.default_rng([seed % 2**32, K, W, D, elem])
    units = D * elem // (16 if vec_ok else elem)
    if named is None:
        named = units > 64
    pos = _named_cells(K, W, D, elem) if named else xk.values(rng, (K, W, D), elem)
    logp = np.full((K, W + pad), FILL[elem], u)
    logp[:, :W] = (rng.standard_normal((K, W)) * 2.0 - 5.0).astype(t).view(u)
    lp = logp.view(t)
    cross = (rng.standard_normal((pairs, 2, W)) * 2.0 - 5.0).astype(t)
    draws = _draws(seed, stream, rnd, pairs, W)
    want = None
    if kind == "crafted":
        want = rng.random((pairs, W)) < 0.5
        want[:, W - 1] = True
        if W >= 2:
            want[:, 0] = False
        if W >= 3:
            want[:, 1] = True
        if W == 1:  # (one walker cannot do both: even slots accept it, odd slots reject it)
            want[:, 0] = np.arange(pairs) % 2 == 0
        lo = -6.0 if elem == 8 else -3.0
        margin = 10.0 ** rng.uniform(lo, math.log10(2.0), (pairs, W))
        for j in range(pairs):
            a = first_chain + 2 * j
            for w in range(W):
                ln_u = math.log(1.0 - rr.canonical(int(draws[j, w])))
                delta = ln_u + (margin[j, w] if want[j, w] else -margin[j, w])
                cross[j, 0, w] = t(delta + float(lp[a, w]) - (float(cross[j, 1, w]) - float(lp[a + 1, w])))
        for j, w in planted:
            a = first_chain + 2 * j
            ln_u = math.log(1.0 - rr.canonical(int(draws[j, w])))
            if elem == 8:
                lp[a, w] = lp[a + 1, w] = cross[j, 1, w] = 0.0
                cross[j, 0, w] = ln_u
            else:
                cross[j, 0, w], cross[j, 1, w], lp[a, w] = _split_f32(ln_u)
                lp[a + 1, w] = 0.0
    else:
        assert kind == "nonfinite" and pairs == 1 and W >= 256 and not planted
        nan = np.array([xk.SPECIALS[elem][0]], u).view(t)[0]  # (with a payload)
        for w in range(W):
            digits = [(w >> (2 * i)) & 3 for i in range(4)]
            for i, (arr, at) in enumerate(((lp, (first_chain, w)), (lp, (first_chain + 1, w)), (cross, (0, 0, w)), (cross, (0, 1, w)))):
                if digits[i]:
                    arr[at] = (None, -math.inf, math.inf, nan)[digits[i]]
    c = dict(name=name, elem=elem, K=K, W=W, D=D, first_chain=first_chain, pairs=pairs, vec_ok=vec_ok, offset=offset, stride=(W + pad) * elem, seed=seed,
             stream=stream, rnd=rnd, kind=kind, planted=sorted(planted), pos=pos, logp=logp, cross=cross.view(u), want=want, draws=draws,
             logp_offset=0, nacc_behind=0, moved_bit=0)
    # the restatement, once
    after_pos, after_logp = pos.copy(), logp.copy()
    c["restated"] = rr.swap_arrays(after_pos, after_logp.view(t)[:, :W], cross.copy(), first_chain, pairs, rnd, seed, stream)
    c["after_pos"], c["after_logp"] = after_pos, after_logp
    return c


def in_sampler_layout(c, parity, moved_bit):
    """The case with its log-posteriors inside chain blocks laid out as a sampler's: [W | W] log-posteriors, the ensemble in half
    `parity` and the other half BLOCK_PATTERN, [W] n_accept words pre-filled with distinct low counts, NACC_GUARD bytes of BLOCK_PATTERN.
    c["block"] [K][stride] bytes goes to the driver in place of c["logp"]."""
    assert c["stride"] == c["W"] * c["elem"] and not c["planted"]
    K, W, elem = c["K"], c["W"], c["elem"]
    c = dict(c, name="%s_parity%d_bit%x" % (c["name"], parity, moved_bit), moved_bit=moved_bit, logp_offset=parity * W * elem, nacc_behind=(2 - parity) * W * elem)
    stride = -(-(2 * W * elem + 4 * W + NACC_GUARD) // 8) * 8
    block = np.full((K, stride), BLOCK_PATTERN, np.uint8)
    block[:, c["logp_offset"]:c["logp_offset"] + W * elem] = c["logp"].view(np.uint8)
    c["nacc"] = (np.arange(K * W, dtype=np.uint32) * 7 + 1).reshape(K, W)
    block[:, 2 * W * elem:2 * W * elem + 4 * W] = c["nacc"].view(np.uint8)
    c["block"], c["stride"] = block, stride
    return c


def split_block(c, block):
    """a case's log-posterior buffer [K][stride / elem] -> (log-posteriors in use [K][W], n_accept [K][W], every other byte)"""
    raw = np.ascontiguousarray(block).view(np.uint8).reshape(c["K"], c["stride"])
    W, elem, lo = c["W"], c["elem"], c["logp_offset"]
    logp = raw[:, lo:lo + W * elem].copy().view(UINT[elem])
    nacc = raw[:, 2 * W * elem:2 * W * elem + 4 * W].copy().view(np.uint32)
    rest = np.concatenate([raw[:, :lo], raw[:, lo + W * elem:2 * W * elem], raw[:, 2 * W * elem + 4 * W:]], axis=1)
    return logp, nacc, rest


def shape_of(c):
    """(units, lanes, trips, walkers per workgroup) of a case: replica_shape's rule, stated again"""
    units = c["D"] * c["elem"] // (16 if c["vec_ok"] else c["elem"])
    lanes = 1
    while lanes < units and lanes < 64:
        lanes *= 2
    return units, lanes, -(-units // lanes), BLOCK // lanes


def _row_w(D, elem, vec):
    """one workgroup and three walkers: two workgroups, the second ragged"""
    units = D * elem // (16 if vec else elem)
    lanes = 1
    while lanes < units and lanes < 64:
        lanes *= 2
    return BLOCK // lanes + 3


ROW_CASES = ["row_D%d_%s" % (d, _t(e)) for d, e in ROWS] + ["row_D%d_%s_misaligned" % (d, _t(e)) for d, e in MISALIGNED]
COUNT_ROWS = {1: (2, 8), 4: (6, 8), 64: (128, 8)}  # lanes -> the row that has them
COUNT_CASES = ["count_lanes%d_W%d" % (lanes, BLOCK // lanes + d) for lanes in COUNT_ROWS for d in (-1, 0, 1)] + ["count_W1", "count_W65", "count_W85_ragged_wavefront"]
PAIR_CASES = ["pairs_K16_first0", "pairs_K16_first1", "pairs_K4_first1"]
NONFINITE_CASES = ["nonfinite_f64", "nonfinite_f32"]
TIE_PLANTS = {"ties_f64": [(0, 3), (0, 70), (0, 130), (0, 199), (1, 5), (1, 64), (1, 191)], "ties_f32": [(0, 0), (0, 63), (0, 64), (1, 129), (1, 199)]}
STREAM_CASES = ["stream_last_round_slot7", "stream_3", "stream_2p63_5"]
# (K, first_chain) x element bytes x the half that holds the ensemble: one test each, over every W, D and moved_bit
MOVED_GROUPS = [(K, first, e, parity) for K, first in ((2, 0), (3, 1)) for e in (8, 4) for parity in (0, 1)]
MOVED_W, MOVED_D = (1, 63, 64, 65), (1, 3, 2, 32)  # D: the element path twice, 16-byte pieces twice (fp32: D = 32 alone)


def moved_names(K, first, e, parity):
    return ["moved_K%d_first%d_W%d_D%d_%s_parity%d_bit%x" % (K, first, W, D, _t(e), parity, bit) for W in MOVED_W for D in MOVED_D for bit in (MOVED_BIT, 0)]


MOVED_CASES = [n for g in MOVED_GROUPS for n in moved_names(*g)]
ALL_CASES = ROW_CASES + COUNT_CASES + PAIR_CASES + NONFINITE_CASES + list(TIE_PLANTS) + STREAM_CASES + MOVED_CASES


@functools.lru_cache(maxsize=None)
def suite():
    """every case, its restatement included: made once, shared by all tests, never edited"""
    cases = []
    for (d, e), (vec, _, _, _) in ROWS.items():
        cases.append(make_case("row_D%d_%s" % (d, _t(e)), e, 2, _row_w(d, e, vec), d, seed=100 + d, named=ROWS[(d, e)][3] > 1))
    for (d, e) in MISALIGNED:
        cases.append(make_case("row_D%d_%s_misaligned" % (d, _t(e)), e, 2, _row_w(d, e, False), d, offset=8, seed=200 + d))
    for lanes, (d, e) in COUNT_ROWS.items():
        for delta in (-1, 0, 1):
            W = BLOCK // lanes + delta
            cases.append(make_case("count_lanes%d_W%d" % (lanes, W), e, 2, W, d, seed=300 + W))
    cases.append(make_case("count_W1", 8, 4, 1, 1, seed=7))            # two slots: one accepts its only walker, one rejects it
    cases.append(make_case("count_W65", 4, 2, 65, 4, seed=8))          # one lane per pair: a wavefront and one walker
    cases.append(make_case("count_W85_ragged_wavefront", 8, 2, 85, 6, seed=9))  # 4 lanes: 64 + 16 + 5 pairs, the last wavefront 5 live groups of 16
    cases.append(make_case("pairs_K16_first0", 8, 16, 70, 6, first_chain=0, pad=3, seed=11))
    cases.append(make_case("pairs_K16_first1", 4, 16, 70, 5, first_chain=1, pad=3, seed=12, rnd=1))
    cases.append(make_case("pairs_K4_first1", 8, 4, 70, 3, first_chain=1, pad=3, seed=13, rnd=5))
    cases.append(make_case("nonfinite_f64", 8, 2, 256, 3, seed=21, kind="nonfinite"))
    cases.append(make_case("nonfinite_f32", 4, 2, 256, 5, seed=22, kind="nonfinite"))
    cases.append(make_case("ties_f64", 8, 4, 200, 2, seed=31, planted=tuple(TIE_PLANTS["ties_f64"])))
    cases.append(make_case("ties_f32", 4, 4, 200, 4, seed=32, planted=tuple(TIE_PLANTS["ties_f32"])))
    cases.append(make_case("stream_last_round_slot7", 8, 16, 600, 1, seed=2**64 - 3, rnd=2**40 - 1))
    cases.append(make_case("stream_3", 8, 2, 130, 2, seed=41, stream=3, rnd=6))
    cases.append(make_case("stream_2p63_5", 4, 2, 130, 4, seed=42, stream=2**63 + 5, rnd=7))
    for K, first, e, parity in MOVED_GROUPS:
        for W in MOVED_W:
            for D in MOVED_D:
                plain = make_case("moved_K%d_first%d_W%d_D%d_%s" % (K, first, W, D, _t(e)), e, K, W, D, first_chain=first, seed=500 + 10 * W + D, rnd=first)
                cases += [in_sampler_layout(plain, parity, bit) for bit in (MOVED_BIT, 0)]
    by_name = {c["name"]: c for c in cases}
    assert list(by_name) == ALL_CASES
    return by_name


# ---------------------------------------------------------------------------------------------------------------- builds

def build_driver():
    """tests/cpp/replica_device.hip and the production replica.hip with the flags of mcmcpp_amd/csrc/Makefile -> the program"""
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(CSRC, "replica.hip"), os.path.join(ROOT, "tests", "cpp", "replica_device.hip")]
    exe = os.path.join(BUILD, "replica_device")
    newest = max([os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc", ".h"))] + [os.path.getmtime(s) for s in srcs])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                               "-mllvm", "-amdgpu-kernarg-preload-count=16", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-I" + CSRC] + srcs + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def plan_exe():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "replica_plan_cases")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "replica_plan_cases.cpp"), "-I", CSRC])
    return exe


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.uint64).tobytes())
        for c in cases:
            f.write(np.array([c[k] for k in ("elem", "K", "W", "D", "first_chain", "pairs", "vec_ok", "offset", "stride", "seed", "stream", "rnd", "logp_offset",
                                             "nacc_behind", "moved_bit")], np.uint64).tobytes())
            for a in (c["pos"], c.get("block", c["logp"]), c["cross"]):
                f.write(np.ascontiguousarray(a).tobytes())


def read_results(path, cases):
    """name -> (positions with their guards as bytes, the log-posterior buffer [K][stride / elem], counts [RECORDS][2] by lower chain)"""
    raw = np.fromfile(path, np.uint8)
    out, at = {}, 0
    for c in cases:
        n_pos = 2 * GUARD + c["pos"].nbytes
        n_logp = c["K"] * c["stride"]
        pos = raw[at:at + n_pos]
        logp = raw[at + n_pos:at + n_pos + n_logp].view(UINT[c["elem"]]).reshape(c["K"], -1)
        counts = raw[at + n_pos + n_logp:at + n_pos + n_logp + 16 * RECORDS].view(np.uint64).reshape(RECORDS, 2)
        out[c["name"]] = (pos, logp, counts)
        at += n_pos + n_logp + 16 * RECORDS
    assert at == raw.size
    return out


def run_driver(exe, cases, folder, limit=CHILD_LIMIT):
    """the child process: every case in one run"""
    src, dst = os.path.join(folder, "cases.bin"), os.path.join(folder, "results.bin")
    write_cases(src, cases)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0 and "replica_device OK cases=%d " % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout.strip())
    return read_results(dst, cases)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    cases = list(suite().values())
    return run_driver(build_driver(), cases, str(tmp_path_factory.mktemp("replica_device")))


# ---------------------------------------------------------------------------------------------------------------- checks

def check_case(c, got):
    """what the kernel left against the restatement, and stated again without it"""
    got_pos, got_logp, counts = got
    K, W, D, elem, pairs, first = c["K"], c["W"], c["D"], c["elem"], c["pairs"], c["first_chain"]
    name = c["name"]
    assert np.all(got_pos[:GUARD] == PATTERN), (name, "guard in front", np.flatnonzero(got_pos[:GUARD] != PATTERN)[:8])
    assert np.all(got_pos[-GUARD:] == PATTERN), (name, "guard behind", np.flatnonzero(got_pos[-GUARD:] != PATTERN)[:8])
    pos = got_pos[GUARD:-GUARD].view(UINT[elem]).reshape(K, W, D)
    r = c["restated"]
    planted = {}
    for j, w in c["planted"]:
        planted.setdefault(j, []).append(w)
    want_pos, want_logp, accepted = c["after_pos"].copy(), c["after_logp"].copy(), r["accepted"].astype(np.int64)
    for j, ws in planted.items():
        a = first + 2 * j
        for w in ws:
            # a planted tie: the decision is the device logarithm's.  Wholly swapped or wholly unchanged, rows and log-posteriors alike.
            before = (c["pos"][a, w], c["pos"][a + 1, w], c["logp"][a, w], c["logp"][a + 1, w])
            swapped = (c["pos"][a + 1, w], c["pos"][a, w], c["cross"][j, 0, w], c["cross"][j, 1, w])
            now = (pos[a, w], pos[a + 1, w], got_logp[a, w], got_logp[a + 1, w])
            assert not np.array_equal(before[0], swapped[0])
            is_swapped = all(np.array_equal(x, y) for x, y in zip(now, swapped))
            assert is_swapped or all(np.array_equal(x, y) for x, y in zip(now, before)), (name, "a planted tie moved in part", j, w)
            restated = bool(r["accept"][j, w])
            if is_swapped != restated:
                accepted[j] += 1 if is_swapped else -1
                for k in (a, a + 1):
                    want_pos[k, w], want_logp[k, w] = pos[k, w], got_logp[k, w]
    bad = np.argwhere(pos != want_pos)
    assert bad.size == 0, (name, "positions differ at (chain, walker, column)", bad[:8].tolist())
    bad = np.argwhere(got_logp != want_logp)
    assert bad.size == 0, (name, "log-posteriors differ at (chain, cell)", bad[:8].tolist())
    lower = [first + 2 * j for j in range(pairs)]
    assert counts.shape == (RECORDS, 2)
    assert counts[lower, 0].tolist() == accepted.tolist(), (name, "accepted", counts[:, 0].tolist(), accepted.tolist())
    assert counts[lower, 1].tolist() == [len(planted.get(j, [])) for j in range(pairs)], (name, "near ties", counts[:, 1].tolist())
    assert not np.delete(counts, lower, axis=0).any(), (name, "count records outside the round's pairs", counts.tolist())
    # without the restatement: chains outside the pairs and the padding are the input's, a crafted walker moved as wanted
    outside = [k for k in range(K) if k < first or k >= first + 2 * pairs]
    assert np.array_equal(pos[outside], c["pos"][outside]) and np.array_equal(got_logp[outside], c["logp"][outside]), (name, "chains outside the pairs")
    assert np.all(got_logp[:, W:] == FILL[elem]), (name, "padding of the log-posteriors")
    if c["want"] is not None:
        for j in range(pairs):
            a = first + 2 * j
            for w in range(W):
                if (j, w) in c["planted"]:
                    continue
                src = (a + 1, a) if c["want"][j, w] else (a, a + 1)
                assert np.array_equal(pos[a, w], c["pos"][src[0], w]) and np.array_equal(pos[a + 1, w], c["pos"][src[1], w]), (name, j, w)


# ------------------------------------------------------------------------------------------------------- CPU: the driver

def test_the_driver_compiles_for_gfx950():
    exe = build_driver()
    assert os.path.exists(exe) and os.access(exe, os.X_OK)
    text = open(os.path.join(ROOT, "tests", "cpp", "replica_device.hip")).read()
    for used in ("launch_replica_swap(a, shape, nullptr)", "replica_shape(W, D, (int)sizeof(T), vec_ok, pairs)", "replica_fill_table(inc, W, t.data())",
                 "replica_slot_base(state0, inc, c.round, j, W)", '#include "replica_kernels.hpp"'):
        assert used in text, used
    assert "__global__" not in text and "MCMCPP_DEFINE_REPLICA_KERNEL" not in text  # (the kernel is replica.hip's alone)


# -------------------------------------------------------------------------------------------- CPU: rows and replica_shape

def _shape(exe, W, D, elem, vec_ok, pairs):
    out = subprocess.run([exe, "shape"] + [str(v) for v in (W, D, elem, vec_ok, pairs)], capture_output=True, text=True, check=True).stdout
    return tuple(int(v) for v in out.split())


def test_the_row_table_has_the_lanes_and_trips_it_is_named_for(plan_exe):
    table = [(key, 1, want) for key, want in ROWS.items()] + [(key, 0, want) for key, want in MISALIGNED.items()]
    reached = set()
    for (d, e), aligned, (vec, units, lanes, trips) in table:
        c = suite()["row_D%d_%s%s" % (d, _t(e), "" if aligned else "_misaligned")]
        assert c["vec_ok"] == int(vec) == int(aligned and (d * e) % 16 == 0) and c["offset"] == (0 if aligned else 8)
        got = _shape(plan_exe, c["W"], d, e, c["vec_ok"], c["pairs"])
        per_block = BLOCK // lanes
        assert got == (lanes, units, 16 if vec else e, per_block, -(-c["W"] // per_block), 1), (d, e, got)
        assert shape_of(c) == (units, lanes, trips, per_block)
        assert c["W"] == per_block + 3 and got[4] == 2  # two workgroups, the second ragged
        assert (c["pos"][0, 0, :3].tolist() == [0, 1, 2]) == (trips > 1)  # multi-trip rows name their cells
        reached.add((lanes, trips, bool(vec)))
    assert {lanes for lanes, _, _ in reached} == {1, 2, 4, 8, 32, 64}
    units_on_64 = sorted(u for (vec, u, lanes, trips) in ROWS.values() if lanes == 64)
    assert units_on_64 == [33, 50, 64, 64, 65, 65, 131, 256, 512, 1022, 1023]  # idle lanes, exactly full, one lane's second trip, many trips
    assert {(64, t, False) for t in (3, 16)} <= reached and {(64, t, True) for t in (1, 2, 4, 8)} <= reached
    for (d, e), (vec, units, lanes, trips) in xk.ROWS.items():  # the exchange kernels' table is here unchanged
        assert ROWS[(d, e)] == (vec, units, lanes, trips)


def test_walker_counts_are_what_they_are_named_for(plan_exe):
    s = suite()
    for lanes, (d, e) in COUNT_ROWS.items():
        per_block = BLOCK // lanes
        for W, blocks in ((per_block - 1, 1), (per_block, 1), (per_block + 1, 2)):
            c = s["count_lanes%d_W%d" % (lanes, W)]
            assert shape_of(c)[1] == lanes and _shape(plan_exe, W, d, e, 1, 1)[:1] + _shape(plan_exe, W, d, e, 1, 1)[3:5] == (lanes, per_block, blocks)
    assert s["count_W1"]["W"] == 1 and s["count_W1"]["pairs"] == 2 and shape_of(s["count_W1"])[1] == 1
    assert s["count_W65"]["W"] == 65 and shape_of(s["count_W65"])[1] == 1
    c = s["count_W85_ragged_wavefront"]
    lanes, per_block = shape_of(c)[1], shape_of(c)[3]
    in_last_block = c["W"] - per_block
    assert (lanes, per_block, in_last_block) == (4, 64, 21) and in_last_block % (64 // lanes) == 5  # 5 live groups and 11 dead ones in the last wavefront with any
    assert [s[n]["pairs"] for n in PAIR_CASES] == [8, 7, 1] and [s[n]["first_chain"] for n in PAIR_CASES] == [0, 1, 1]
    for n in PAIR_CASES:
        assert s[n]["stride"] == (s[n]["W"] + 3) * s[n]["elem"]
    assert s["pairs_K16_first1"]["K"] == 16 and s["pairs_K4_first1"]["K"] == 4


# ------------------------------------------------------------------------------ CPU: the inputs have what they are there for

def test_no_decision_outside_the_planted_ones_is_a_near_tie():
    for c in suite().values():
        assert sorted(c["restated"]["in_band"]) == c["planted"], c["name"]
        assert c["restated"]["near_ties"].tolist() == [sum(1 for j, _ in c["planted"] if j == s) for s in range(c["pairs"])]


def test_crafted_decisions_are_the_wanted_ones_and_every_slot_accepts_and_rejects():
    t_margins = []
    for c in suite().values():
        acc = c["restated"]["accept"]
        if c["kind"] == "nonfinite":
            continue
        free = np.ones_like(acc)
        for j, w in c["planted"]:
            free[j, w] = False
        assert np.array_equal(acc[free], c["want"][free]), c["name"]
        if c["W"] == 1:
            continue
        assert acc[:, -1].all() or c["planted"], c["name"]  # the last walker swaps: a `live` guard one short shows
        for j in range(c["pairs"]):
            assert 1 <= int(acc[j][free[j]].sum()) < int(free[j].sum()), (c["name"], j)
            # accepted and rejected walkers side by side inside the first wavefront (64 lanes: a wavefront holds one pair)
            per_wavefront = 64 // shape_of(c)[1]
            assert per_wavefront == 1 or (acc[j, :per_wavefront].any() and not acc[j, :per_wavefront].all()), (c["name"], j)
        a = c["first_chain"]
        lp, cross = c["logp"].view(FLOAT[c["elem"]]), c["cross"].view(FLOAT[c["elem"]])
        for j in range(c["pairs"]):
            for w in range(c["W"]):
                if free[j, w]:
                    _, _, ln_u, delta = rr.decide(int(c["draws"][j, w]), lp[a + 2 * j, w], lp[a + 2 * j + 1, w], cross[j, 0, w], cross[j, 1, w])
                    t_margins.append(abs(ln_u - delta) / (1e-6 if c["elem"] == 8 else 1e-3))
    assert 0.5 < min(t_margins) < 2.0  # the narrowest margins are about the stated ones: a wrong draw flips decisions


def test_the_one_walker_case_decides_both_ways():
    """W = 1 cannot accept and reject in one slot: its two slots are one of each."""
    one = suite()["count_W1"]
    assert one["restated"]["accept"].tolist() == [[True], [False]] and one["restated"]["accepted"].tolist() == [1, 0]
    assert not np.array_equal(one["pos"][0], one["pos"][1]) and not np.array_equal(one["pos"][2], one["pos"][3])


def test_the_non_finite_table_holds_every_combination_once():
    inf = math.inf
    for name in NONFINITE_CASES:
        c = suite()[name]
        t = FLOAT[c["elem"]]
        lp, cross = c["logp"].view(t), c["cross"].view(t)
        kinds = set()
        for w in range(c["W"]):
            four = (lp[0, w], lp[1, w], cross[0, 0, w], cross[0, 1, w])
            kinds.add(tuple("f" if math.isfinite(v) else str(float(v)) for v in four))
        assert len(kinds) == 4**4 and c["W"] == 256
        acc = c["restated"]["accept"][0]
        assert 8 <= acc.sum() <= 248 and not c["restated"]["in_band"]  # (few combinations have delta = +inf)
        for w in np.flatnonzero(acc):  # an accepted walker's delta is no NaN: its cross values are finite or infinite
            assert not math.isnan(cross[0, 0, w]) and not math.isnan(cross[0, 1, w])
        assert any(cross[0, 0, w] == inf for w in np.flatnonzero(acc)) and any(cross[0, 1, w] == inf for w in np.flatnonzero(acc))
        nan_bits = xk.SPECIALS[c["elem"]][0]
        assert (c["logp"] == nan_bits).sum() == 128 and (c["cross"] == nan_bits).sum() == 128  # NaN with its payload, stored and crossed


def test_planted_ties_are_exact_for_python_and_spread_over_wavefronts_and_slots():
    for name, plants in TIE_PLANTS.items():
        c = suite()[name]
        t = FLOAT[c["elem"]]
        lp, cross = c["logp"].view(t), c["cross"].view(t)
        assert c["planted"] == sorted(plants) and shape_of(c)[1] == 1  # one lane per pair: wavefront = walker // 64
        assert len({(j, w // 64) for j, w in plants}) >= 3 and {j for j, _ in plants} == {0, 1} and len({w // 64 for _, w in plants}) >= 3
        for j, w in plants:
            a = 2 * j
            acc, tie, ln_u, delta = rr.decide(int(c["draws"][j, w]), lp[a, w], lp[a + 1, w], cross[j, 0, w], cross[j, 1, w])
            assert delta == ln_u and tie and not acc and ln_u < 0.0, (name, j, w, ln_u)
            if c["elem"] == 8:
                assert (lp[a, w], lp[a + 1, w], cross[j, 1, w]) == (0.0, 0.0, 0.0) and cross[j, 0, w] == math.log(1.0 - rr.canonical(int(c["draws"][j, w])))


def test_stream_cases_reach_the_positions_and_increments_they_are_named_for():
    s = suite()
    c = s["stream_last_round_slot7"]
    assert (c["rnd"], c["pairs"], c["W"]) == (2**40 - 1, 8, 600)
    assert (c["rnd"] * 8 + 7) * c["W"] > 2**52 and (c["rnd"] * 8 + 7) * c["W"] + c["W"] < 2**64
    incs = {}
    for name in STREAM_CASES + ["row_D1_f64"]:
        c = s[name]
        g = po.Pcg64(c["seed"], 2**64 - 1 - c["stream"])
        incs[name] = g.inc >> 64
        g.advance((c["rnd"] * 8 + c["pairs"] - 1) * c["W"] + c["W"] - 1)
        assert g.next() == int(c["draws"][-1, -1]) and int(c["restated"]["draws"][-1, -1]) == int(c["draws"][-1, -1])
    assert (s["stream_3"]["stream"], s["stream_2p63_5"]["stream"]) == (3, 2**63 + 5)
    assert incs == {"stream_last_round_slot7": 1, "stream_3": 1, "stream_2p63_5": 0, "row_D1_f64": 1}  # inc.hi, both values


# ------------------------------------------------------------------------------------------- CPU: the restatement's split

def test_swap_arrays_on_a_case_worked_by_hand():
    """Decided by infinities alone, whatever the draws: delta = +inf accepts, -inf and NaN reject."""
    inf, nan = math.inf, math.nan
    pos = np.arange(3 * 4 * 2, dtype=np.float64).reshape(3, 4, 2)
    logp = np.array([[-1.0, -2.0, -3.0, -4.0], [-5.0, -6.0, -7.0, -8.0], [-9.0, -10.0, -11.0, -12.0]])
    cross = np.array([[[inf, -inf, nan, inf], [-20.0, -21.0, -22.0, inf]]])
    p, lp = pos.copy(), logp.copy()
    r = rr.swap_arrays(p, lp, cross, 1, 1, 4, 9)
    assert r["accept"].tolist() == [[True, False, False, True]] and r["accepted"].tolist() == [2] and r["near_ties"].tolist() == [0] and not r["in_band"]
    assert np.array_equal(p[0], pos[0]) and np.array_equal(lp[0], logp[0])  # chain 0 is no part of first_chain = 1
    assert p[1].tolist() == [[16.0, 17.0], [10.0, 11.0], [12.0, 13.0], [22.0, 23.0]] and p[2].tolist() == [[8.0, 9.0], [18.0, 19.0], [20.0, 21.0], [14.0, 15.0]]
    assert lp[1].tolist() == [inf, -6.0, -7.0, inf] and lp[2].tolist() == [-20.0, -10.0, -11.0, inf]
    g = po.Pcg64(9, 2**64 - 1)
    g.advance(4 * 8 * 4)
    assert [g.next() for _ in range(4)] == r["draws"][0].tolist()


def test_exchange_arrays_is_swap_arrays_on_the_evaluated_cross_values():
    K, W, D = 5, 40, 3
    rng = np.random.default_rng(3)
    betas = [1.0, 0.6, 0.4, 0.2, 0.1]

    def cross_logp(k, rows):
        return -0.5 * betas[k] * (rows * rows).sum(axis=1)

    for rnd in (0, 1, 6, 7):
        pos = rng.standard_normal((K, W, D))
        logp = np.stack([cross_logp(k, pos[k]) for k in range(K)])
        p1, l1, p2, l2 = pos.copy(), logp.copy(), pos.copy(), logp.copy()
        got = rr.exchange_arrays(p1, l1, cross_logp, rnd, 17, stream=2)
        chains = rr.pairs_of(K, rnd)
        cross = np.stack([np.stack([cross_logp(a, pos[b]), cross_logp(b, pos[a])]) for a, b in chains])
        want = rr.swap_arrays(p2, l2, cross, rnd & 1, len(chains), rnd, 17, stream=2)
        assert np.array_equal(p1, p2) and np.array_equal(l1, l2) and not np.array_equal(p1, pos)
        for j, (a, _) in enumerate(chains):
            assert got["proposed"][a] == W and got["accepted"][a] == want["accepted"][j] and 0 < got["accepted"][a] < W
        idle = [k for k in range(K - 1) if k not in [a for a, _ in chains]]
        assert not got["proposed"][idle].any() and not got["accepted"][idle].any()
        # and the rule as it was written before the split: walker by walker, pair by pair
        p3, l3 = pos.copy(), logp.copy()
        for a, b in chains:
            g = po.Pcg64(17, 2**64 - 1 - 2)
            g.advance((rnd * 8 + (a >> 1)) * W)
            ab, ba = cross_logp(a, p3[b]), cross_logp(b, p3[a])
            for w in range(W):
                if rr.decide(g.next(), l3[a, w], l3[b, w], ab[w], ba[w])[0]:
                    p3[[a, b], w] = p3[[b, a], w]
                    l3[a, w], l3[b, w] = ab[w], ba[w]
        assert np.array_equal(p1, p3) and np.array_equal(l1, l3)


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_CASES)
def test_every_row_shape(device, name):
    check_case(suite()[name], device[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNT_CASES)
def test_walker_counts_at_the_edges_of_a_workgroup(device, name):
    check_case(suite()[name], device[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pairs_slots_and_what_lies_outside_them(device, name):
    c = suite()[name]
    check_case(c, device[name])
    _, logp, counts = device[name]
    lower = [c["first_chain"] + 2 * j for j in range(c["pairs"])]
    assert counts[lower, 0].tolist() == c["restated"]["accepted"].tolist() and not np.delete(counts, lower, axis=0).any()
    assert logp.shape == (c["K"], c["W"] + 3) and np.all(logp[:, c["W"]:] == FILL[c["elem"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONFINITE_CASES)
def test_non_finite_stored_and_cross_log_posteriors(device, name):
    c = suite()[name]
    check_case(c, device[name])
    _, logp, counts = device[name]
    assert counts[0].tolist() == [int(c["restated"]["accept"].sum()), 0]
    for w in np.flatnonzero(c["restated"]["accept"][0]):  # the cross values arrive bit for bit
        assert logp[0, w] == c["cross"][0, 0, w] and logp[1, w] == c["cross"][0, 1, w]
    for w in np.flatnonzero(~c["restated"]["accept"][0]):  # and a rejected walker keeps its own, NaN payload included
        assert logp[0, w] == c["logp"][0, w] and logp[1, w] == c["logp"][1, w]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TIE_PLANTS))
def test_planted_near_ties_are_counted(device, name):
    c = suite()[name]
    check_case(c, device[name])
    counts = device[name][2]
    assert counts[:, 1].tolist() == [0 if k % 2 else sum(1 for j, _ in TIE_PLANTS[name] if 2 * j == k) for k in range(RECORDS)]  # (first_chain = 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAM_CASES)
def test_the_stream_on_the_device(device, name):
    check_case(suite()[name], device[name])


def check_moved(c, got):
    """a moved case: rows, log-posteriors in use and counts as without the bit; the bit in n_accept, and nothing else anywhere"""
    name, K, first = c["name"], c["K"], c["first_chain"]
    got_pos, block, counts = got
    logp, nacc, rest = split_block(c, block)
    check_case(c, (got_pos, logp, counts))
    assert np.all(rest == BLOCK_PATTERN), (name, "the other log-posterior half or the guard behind n_accept", np.argwhere(rest != BLOCK_PATTERN)[:8].tolist())
    swapped = np.zeros((K, c["W"]), bool)
    swapped[first] = swapped[first + 1] = c["restated"]["accept"][0]
    assert np.array_equal(nacc & np.uint32(MOVED_BIT - 1), c["nacc"]), (name, "low bits of n_accept")
    if c["moved_bit"]:
        assert np.array_equal((nacc & np.uint32(MOVED_BIT)) != 0, swapped), (name, "moved_bit", np.argwhere(((nacc >> 31) != 0) != swapped)[:8].tolist())
    else:
        assert np.array_equal(nacc, c["nacc"]), (name, "n_accept with moved_bit = 0")


@pytest.mark.gpu
@pytest.mark.parametrize("K,first,e,parity", MOVED_GROUPS, ids=["K%d_first%d_%s_parity%d" % (K, first, _t(e), parity) for K, first, e, parity in MOVED_GROUPS])
def test_moved_bit_in_n_accept_behind_the_log_posteriors(device, K, first, e, parity):
    """What a round inside a run of the full-step kernels adds: the bit in both chains' n_accept for exactly the swapped walkers,
    the counts in the low bits and every byte around the words as they were; with moved_bit = 0 no byte of n_accept changes."""
    for name in moved_names(K, first, e, parity):
        check_moved(suite()[name], device[name])
