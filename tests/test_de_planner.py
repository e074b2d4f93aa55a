"""The stream planner of Mover::DifferentialEvolution (mcmcpp_amd/csrc/diffevo_plan.hpp), role by role and batch by batch.

Whole runs against the oracle (tests/test_diffevo.py, test_lane_mappings.py, test_device_chain.py) see of the planner what a
real stream does at their shapes: pcg's bounded_rand threshold is below 2^30 there, so no draw of theirs ever fell below it,
and no error flag ever rose.  Here the planner runs alone -- tests/cpp/de_planner_device.hip drives the production
de_boundary_kernel through the production DePlanner, one launch at a time -- on streams whose every draw
tests/de_stream_restatement.py knows, with the threshold and the capacities as parameters.

  CPU   the replay's raw stream against numpy.random.PCG64; its thrown-away total against the oracle's at the production
        threshold; that the chosen cases contain what they are there for (from the replay alone); that each flag case
        predicts its flag and no other, at the batch it is meant for.
  GPU   after every launch: the guards around the lists, the batch records, the head and the records; DeHead; the DeBatch
        just resolved (base, extra_base, events, plan[]); the records just made (ind1, ind2, s, neg_exp); the lists just
        scanned, as sets (their order comes from an atomic).  Everything is bit-exact; neg_exp is compared with the host
        build of the type's own logarithm (tests/cpp/de_accept_log_cases.cpp).  What a flagged batch and those behind it
        hold is not specified and not compared.

Seeds were searched with the replay for what a case is there for; each is recorded with its reason."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import de_stream_restatement as dr
from tests.test_de_batch_plan import inline_arithmetic as plan_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

T16, T3 = 2 ** 64 // 16, 2 ** 64 // 3
ROOMY = dict(bad_capacity=1024, resolve_capacity=16000)  # (16000 keys and the widest forced row's tables: 64 328 bytes of LDS)


class Case:
    """n walkers per half, D parameters; batch, scan_run, threshold, bad_capacity, resolve_capacity: None = the plan's own"""

    def __init__(self, name, n, D, batch, scan_run, seed, batches, threshold=None, bad_capacity=None, resolve_capacity=None, why=""):
        self.name, self.n, self.D, self.seed, self.batches, self.why = name, n, D, seed, batches, why
        p = plan_of(n, D, batch if batch is not None and batch <= 64 else None, scan_run)
        self.batch = batch if batch is not None and batch > 64 else p["batch_max"]
        self.scan_run = p["scan_run"]
        self.threshold = dr.production_threshold(n) if threshold is None else threshold
        self.bad_capacity = p["bad_capacity"] if bad_capacity is None else bad_capacity
        self.resolve_capacity = p["resolve_capacity"] if resolve_capacity is None else resolve_capacity
        self.overrides = [-1 if threshold is None else threshold & 0xFFFFFFFF, -1 if threshold is None else threshold >> 32,
                          -1 if bad_capacity is None else bad_capacity, -1 if resolve_capacity is None else resolve_capacity,
                          -1 if scan_run is None else scan_run, -1 if batch is None else batch]
        self.per = D + 3
        self.updates = n * self.batch
        self.positions = self.per * (self.updates - 1) + dr.SHIFT_MAX + 1
        self.scan_positions = self.positions + dr.SHIFT_MAX + 1
        self.seg_len = -(-self.scan_positions // dr.SEGMENTS)

    @functools.lru_cache(maxsize=None)
    def replay(self):
        return dr.replay(self.seed, self.n, self.D, self.threshold, self.updates, self.batches)

    @functools.lru_cache(maxsize=None)
    def flags(self, b):
        st, bs = self.replay()
        return dr.predict_flags(st, bs, b, self.n, self.threshold, self.scan_positions, self.seg_len, self.bad_capacity, self.resolve_capacity)


# ---- production thresholds: four batches each (`behind` and both parities twice); no flag.  Seed 11: these cases are there
# for their shapes, which no seed misses (test_production_cases_hold_what_they_are_there_for) -- but for the first: 128 updates
# have 64 events in the mean, and seed 82 is the first from 1 on with more than 64 in every one of the four batches
PRODUCTION = [
    Case("n2_D1", 2, 1, 64, 8, 82, 4, why="every second position bad: more than 2048 listed (the second trip of the counting sort), more than 64 events (bisection)"),
    Case("n2_D200", 2, 200, None, 8, 11, 4, why="the by_lists cut (5 half-steps); per = 203: four rounds of the residue scan, the last ragged"),
    Case("n3_D1021", 3, 1021, None, 8, 11, 4, why="per = 1024"),
    Case("n3_D1024", 3, 1024, None, 5, 11, 4, why="per = 1027, the widest; positions no multiple of the run"),
    Case("n7_D3", 7, 3, 64, 1, 11, 4, why="modulo path, threshold 2 (never hit), a run of one"),
    Case("n5_D62", 5, 62, 3, 8, 11, 4, why="per = 65: one residue in the second round"),
    Case("n64_D5", 64, 5, 64, 8, 11, 4, why="power-of-two path, 4096 updates: jump_hi past entry 0, 16 record blocks"),
    Case("n300_D4", 300, 4, 1, 8, 11, 4, why="a batch of one half-step: positions dominated by kDeShiftMax + 1; a ragged record block"),
]
BOTH_TYPES = ("n2_D1", "n300_D4")

# ---- forced thresholds, generous capacities: no flag, bit-equal.  Halves that are no power of two (a power-of-two half has
# threshold 0 in production and the scan's fast path is sound only there).  Batch lengths keep the events under kDeMaxEvents
# and the shift under kDeShiftMax.  Seeds: the first from 1 on whose three batches hold a rejected first draw, a rejected second
# draw, events at consecutive updates, an event whose last thrown-away position is bad itself, three wraps of cr and an event
# at the last update of a batch.
FORCED = [
    Case("t16_n5_D2", 5, 2, 64, 8, 2, 3, T16, **ROOMY), Case("t16_n5_D5", 5, 5, 64, 8, 1, 3, T16, **ROOMY),
    Case("t16_n37_D2", 37, 2, 64, 8, 2, 3, T16, **ROOMY), Case("t16_n37_D5", 37, 5, 64, 8, 3, 3, T16, **ROOMY),
    Case("t3_n5_D2", 5, 2, 64, 8, 1, 3, T3, **ROOMY), Case("t3_n5_D5", 5, 5, 64, 8, 1, 3, T3, **ROOMY),
    Case("t3_n37_D2", 37, 2, 32, 8, 1, 3, T3, **ROOMY), Case("t3_n37_D5", 37, 5, 32, 8, 1, 3, T3, **ROOMY),  # (64 half-steps: some 1350 events)
]

# ---- flags: (case, flag, the batch it rises at, "scan" or "resolve").  Two clean batches (one for the events) lie in front.
FLAGS = [
    # 0.7 x 2^64, 851 updates: 4062, 4028, then 4230 draws thrown away; some 780 events and 11 400 listed positions, which hold
    (Case("shift", 37, 2, 23, 8, 12, 4, int(0.7 * 2 ** 64), **ROOMY, why="seed 12: the first whose shifts are <= 4095, <= 4095, > 4095 with no update past the window"),
     dr.ERR_SHIFT, 2, "resolve"),
    # production threshold; the longest lists of batches 0..3 hold 33, 35, 36, 38 positions
    (Case("list", 5, 2, 8, 8, 2, 4, bad_capacity=35, why="seed 2: the first whose batch 2 has a longer list than batches 0 and 1"), dr.ERR_CAND, 2, "scan"),
    # the lists of batches 0..3 hold 1609, 1613, 1617, 1615 positions together
    (Case("total", 5, 2, 8, 8, 1, 4, resolve_capacity=1613, why="seed 1: the first whose batch 2 lists more than batches 0 and 1"), dr.ERR_CAND, 2, "resolve"),
    # 0.225 x 2^64, 2368 updates: 987, then 1028 events
    (Case("events", 37, 5, 64, 8, 18, 3, int(0.225 * 2 ** 64), **ROOMY, why="seed 18: the first with <= 1024 events in batch 0 and more in batch 1"), dr.ERR_CAND, 1, "resolve"),
    # 0.9 x 2^64 with three walkers per half (two are a power of two: no forced threshold there); the updates of batches 0..3
    # throw away at most 20, 20, 92, 27 draws
    (Case("window", 3, 1, 1, 8, 6, 4, int(0.9 * 2 ** 64), resolve_capacity=16000, why="seed 6: the first whose batch 2 is the first with an update past 30 thrown-away draws"),
     dr.ERR_WINDOW, 2, "resolve"),
]
FLAG_IDS = [f[0].name for f in FLAGS]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_the_replays_raw_stream_is_numpys_pcg64():
    for seed, stream in ((0, 0), (21, 0), (2 ** 63 + 5, 7)):
        st = dr.Stream(seed, stream)
        st.need(5000)
        bg = np.random.PCG64(0)
        bg.state = {"bit_generator": "PCG64", "state": {"state": st.state0, "inc": st.inc}, "has_uint32": 0, "uinteger": 0}
        np.testing.assert_array_equal(bg.random_raw(5000), np.array(st.raw[:5000], dtype=np.uint64))


def test_the_replays_thrown_away_total_is_the_oracles():
    from oracle import pyoracle as po
    from tests.goldens import Golden
    g = Golden("de_iso14x3")
    orc = po.Oracle(g.W, g.D, g.calc, g.params, seed=g.seed, dtype=g.dtype, mover=po.MOVER_DIFFERENTIAL_EVOLUTION)
    orc.set_state(g.init_pos, g.init_logp)
    orc.run(g.steps, interval=g.slicing, save_chain=False)
    n = g.W // 2
    _, bs = dr.replay(g.seed, n, g.D, dr.production_threshold(n), 2 * n * g.steps * g.slicing, 1)
    assert bs[0].shift == orc.redraws > 0
    W, D, steps = 4, 1, 500
    pos = po.init_positions(po.F64, W, D, salt=6)
    orc = po.Oracle(W, D, po.CALC_ISO_GAUSSIAN, None, seed=21, mover=po.MOVER_DIFFERENTIAL_EVOLUTION)
    orc.set_state(pos, orc.logp(pos))
    orc.run(steps)
    _, bs = dr.replay(21, 2, D, 0, 2 * 2 * steps, 1)
    assert bs[0].shift == orc.redraws > 1000 and sum(bs[0].E) == bs[0].shift == len(bs[0].thrown)


@pytest.mark.parametrize("case", PRODUCTION + FORCED, ids=lambda c: c.name)
def test_no_flag_is_predicted_where_none_is_expected(case):
    for b in range(case.batches):
        scan, res, _ = case.flags(b)
        assert scan == 0 and res == 0, (case.name, b)
    _, bs = case.replay()
    assert max(len(b.events) for b in bs) < dr.MAX_EVENTS and max(b.shift for b in bs) < dr.SHIFT_MAX


def test_production_cases_hold_what_they_are_there_for():
    by = {c.name: c for c in PRODUCTION}
    c = by["n2_D1"]
    assert c.per == 4 and c.resolve_capacity == 8192
    for b in range(c.batches):
        assert sum(len(l) for l in c.flags(b)[2]) > 8 * 256      # the counting sort's second trip (!once)
        assert len(c.replay()[1][b].events) > 64                 # the records search by bisection
    assert max(max(b.E) for b in c.replay()[1]) >= 5
    # bad positions at either end of a list, at the last position a scan looks at, in front of the batch's true start (scanned
    # from the provisional one: the resolve drops them) and behind the last position an update can start at (dropped too)
    listed = [sorted(p for l in c.flags(b)[2] for p, _ in l) for b in range(c.batches)]
    assert any(p % c.seg_len == 0 for ps in listed for p in ps) and any(p % c.seg_len == c.seg_len - 1 for ps in listed for p in ps)
    assert any(ps[-1] == c.scan_positions - 1 for ps in listed)
    behind = [0] + [b.shift for b in c.replay()[1][:-1]]
    assert any(ps[0] < behind[b] for b, ps in enumerate(listed)) and all(ps[-1] - behind[b] >= c.positions for b, ps in enumerate(listed))
    c = by["n2_D200"]
    assert c.batch == 5 and c.per == 203 and c.per % 64 != 0 and -(-c.per // 64) == 4
    assert by["n3_D1021"].per == 1024 and by["n3_D1024"].per == 1027 and by["n3_D1024"].scan_positions % 5 != 0 and by["n3_D1024"].scan_run == 5
    assert by["n7_D3"].threshold == 2 and by["n7_D3"].scan_run == 1
    assert by["n5_D62"].per == 65
    c = by["n64_D5"]
    assert c.threshold == 0 and c.updates == 4096 and c.updates // 256 == 16
    c = by["n300_D4"]
    assert c.updates == 300 and c.positions < 2 * (dr.SHIFT_MAX + 1) and c.updates % 256 != 0
    # every production case: a batch that throws draws away with a batch behind it (`behind` has something to subtract)
    for c in PRODUCTION:
        _, bs = c.replay()
        assert any(b.shift > 0 for b in bs[:-1]), c.name


def _holds(case):
    st, bs = case.replay()
    n, thr, per = case.n, case.threshold, case.per

    def is_bad(k):
        x, y = st.draw(k), st.draw(k + 1)
        return x < thr or y < thr or x % n == y % n

    return dict(first=any(s == 1 for b in bs for _, s in b.thrown), second=any(s == 2 for b in bs for _, s in b.thrown),
                consecutive=any(b.events[i + 1][0] == b.events[i][0] + 1 for b in bs for i in range(len(b.events) - 1)),
                # with E draws thrown away the update's start moves to where position start + E was: bad itself, it must not become
                # a second event of the same update (the walk's m > m_last)
                inner=any(is_bad(b.start[m] + b.E[m]) for b in bs for m, _ in b.events),
                wraps=max(b.shift // per for b in bs), last=any(b.events and b.events[-1][0] == case.updates - 1 for b in bs))


@pytest.mark.parametrize("case", FORCED, ids=lambda c: c.name)
def test_forced_cases_hold_the_corners(case):
    h = _holds(case)
    assert h["first"] and h["second"] and h["consecutive"] and h["inner"] and h["wraps"] >= 3 and h["last"], h
    assert case.n & (case.n - 1)


@pytest.mark.parametrize("case,flag,at,role", FLAGS, ids=FLAG_IDS)
def test_flag_cases_predict_their_flag_alone(case, flag, at, role):
    for b in range(at + 1):
        scan, res, _ = case.flags(b)
        want = (flag if role == "scan" else 0, flag if role == "resolve" else 0) if b == at else (0, 0)
        assert (scan, res) == want, (case.name, b, scan, res)
    st, bs = case.replay()
    if case.name == "shift":
        assert [b.shift > dr.SHIFT_MAX for b in bs[:3]] == [False, False, True] and max(len(b.events) for b in bs) <= dr.MAX_EVENTS
    if case.name == "events":
        assert len(bs[0].events) <= dr.MAX_EVENTS < len(bs[1].events) and bs[1].shift <= dr.SHIFT_MAX
    if case.name == "window":
        assert [max(b.E) > dr.WINDOW - 2 for b in bs[:3]] == [False, False, True] and case.n == 3


# ---------------------------------------------------------------------------------------------------------------- GPU

def build_shim():
    """tests/cpp/de_planner_device.hip with the flags of mcmcpp_amd/csrc/Makefile"""
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "de_planner_device.hip")
    out = os.path.join(BUILD, "libde_planner_device.so")
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc", ".h")))
    if not os.path.exists(out) or os.path.getmtime(out) < max(newest, os.path.getmtime(src)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-mllvm", "-amdgpu-kernarg-preload-count=16", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-I" + CSRC, src, "-o", out])
    return out


@pytest.fixture(scope="module")
def dev():
    L = C.CDLL(build_shim())
    L.dp_create.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.dp_destroy.argtypes = [C.c_void_p]
    L.dp_destroy.restype = None
    L.dp_info.argtypes = [C.c_void_p, C.c_void_p]
    L.dp_prime.argtypes = [C.c_void_p, C.c_int]
    L.dp_boundary.argtypes = [C.c_void_p, C.c_longlong]
    L.dp_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def accept_log():
    """raw accept draws -> (fp64 bits, fp32 bits) of log(1 - canonical(raw)), by the host build of the device's own headers"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "de_accept_log_cases")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "de_accept_log_cases.cpp"), "-I", CSRC])

    def run(raw, tmp):
        fin, f64, f32 = (os.path.join(str(tmp), f) for f in ("raw.bin", "f64.bin", "f32.bin"))
        np.asarray(raw, dtype=np.uint64).tofile(fin)
        subprocess.check_call([exe, fin, f64, f32])
        return np.fromfile(f64, dtype=np.uint64), np.fromfile(f32, dtype=np.uint32)

    return run


HEAD = np.dtype([("state", "<u8", 2), ("extra_total", "<u8"), ("error", "<u4"), ("last_shift", "<u4"), ("provisional", "<u8", (2, 2))])
BATCH = np.dtype([("base", "<u8", 2), ("extra_base", "<u8"), ("events", "<u4"), ("pad", "<u4", 9), ("plan", "<u4", (dr.MAX_EVENTS, 2))])
REC = {False: np.dtype([("s", "<u8", 2), ("neg_exp", "<u8"), ("ind1", "<u4"), ("ind2", "<u4")]),
       True: np.dtype([("s", "<u8", 2), ("neg_exp", "<u4"), ("ind1", "<u4"), ("ind2", "<u4"), ("pad", "<u4")])}


def u128(pair):
    return int(pair[0]) | (int(pair[1]) << 64)


class Planner:
    def __init__(self, L, case, f32):
        self.L, self.case, self.f32 = L, case, f32
        self.h = C.c_void_p()
        ov = np.array(case.overrides, dtype=np.int64)
        rc = L.dp_create(int(f32), case.seed, case.n, case.D, ov.ctypes.data, C.byref(self.h))
        assert rc == 0, "dp_create: %d" % rc
        info = np.zeros(16, dtype=np.int64)
        assert L.dp_info(self.h, info.ctypes.data) == 0
        # the shim's numbers are the case's: what the replay is asked for is what the kernels are launched with
        assert list(info[:8]) == [case.batch, case.updates, case.positions, case.scan_positions, case.seg_len, case.bad_capacity, case.resolve_capacity, case.scan_run]
        assert int(info[10]) & (2 ** 64 - 1) == case.threshold
        assert (info[12], info[13], info[14]) == (BATCH.itemsize, 32, HEAD.itemsize) and info[15] <= 65536

    def close(self):
        self.L.dp_destroy(self.h)

    def _read(self, what, which, dtype, count):
        out = np.zeros(count, dtype=dtype)
        assert self.L.dp_read(self.h, what, which, out.ctypes.data, out.nbytes) == 0
        return out

    def head(self):
        return self._read(0, 0, HEAD, 1)[0]

    def batch(self, b):
        return self._read(1, b & 1, BATCH, 1)[0]

    def recs(self):
        return self._read(2, 0, REC[self.f32], self.case.updates)

    def lists(self, b):
        """the lists of batch b as scanned last: per list, the set of (p, E)"""
        cap = self.case.bad_capacity
        counts = self._read(4, b & 1, np.uint32, 64 * 32)[::32]
        bad = self._read(3, b & 1, np.uint32, 64 * cap * 2).reshape(64, cap, 2)
        return counts, [set((int(p), int(e)) for p, e in bad[s, :min(int(counts[s]), cap)]) for s in range(64)]


def check_head(pl, batches, resolved, error):
    """behind the resolve of batch `resolved`"""
    h, b = pl.head(), batches[resolved]
    assert int(h["error"]) == error
    assert u128(h["state"]) == b.next_state
    assert int(h["extra_total"]) == b.extra_base + b.shift and int(h["last_shift"]) == b.shift


def check_batch(pl, batches, k):
    got, b = pl.batch(k), batches[k]
    assert u128(got["base"]) == b.base and int(got["extra_base"]) == b.extra_base
    assert int(got["events"]) == len(b.events)
    np.testing.assert_array_equal(got["plan"][:len(b.events)], np.array(b.events, dtype=np.uint32).reshape(-1, 2))


def check_recs(pl, batches, k, accept_log, tmp):
    got, b = pl.recs(), batches[k]
    np.testing.assert_array_equal(got["ind1"], np.array(b.ind1, dtype=np.uint32))
    np.testing.assert_array_equal(got["ind2"], np.array(b.ind2, dtype=np.uint32))
    np.testing.assert_array_equal(got["s"][:, 0], np.array([s & (2 ** 64 - 1) for s in b.s], dtype=np.uint64))
    np.testing.assert_array_equal(got["s"][:, 1], np.array([s >> 64 for s in b.s], dtype=np.uint64))
    want64, want32 = accept_log(b.accept_raw, tmp)
    np.testing.assert_array_equal(got["neg_exp"], want32 if pl.f32 else want64)


def check_lists(pl, case, b):
    counts, got = pl.lists(b)
    want = case.flags(b)[2]
    assert [int(c) for c in counts] == [len(l) for l in want]
    assert got == want


def launches(case):
    """the launch sequence: (what to call, the batch it scans or None, the batch it resolves or None, the batch whose records it
    makes or None) -- rewind, the two priming launches, then a boundary per batch while the replay covers what it resolves"""
    seq = [(("prime", 0), None, None, None), (("prime", 1), 0, None, None), (("prime", 2), 1, 0, None)]
    for b in range(case.batches - 1):
        seq.append((("boundary", b), b + 2, b + 1, b))
    return seq


def call(pl, what):
    rc = pl.L.dp_prime(pl.h, what[1]) if what[0] == "prime" else pl.L.dp_boundary(pl.h, what[1])
    assert rc == 0, "%s: %d (-2: a guard was written)" % (what, rc)


def run_clean(dev, case, f32, accept_log, tmp):
    _, batches = case.replay()
    pl = Planner(dev, case, f32)
    try:
        for what, scanned, resolved, recorded in launches(case):
            call(pl, what)
            if resolved is not None:
                check_head(pl, batches, resolved, 0)
                check_batch(pl, batches, resolved)
            else:
                assert int(pl.head()["error"]) == 0
            if recorded is not None:
                check_recs(pl, batches, recorded, accept_log, tmp)
            if scanned is not None and scanned < case.batches:
                check_lists(pl, case, scanned)
    finally:
        pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,f32", [(c, t) for c in PRODUCTION for t in ((False, True) if c.name in BOTH_TYPES else (False,))],
                         ids=lambda v: v.name if isinstance(v, Case) else ("f32" if v else "f64"))
def test_planner_at_production_thresholds(dev, accept_log, tmp_path, case, f32):
    run_clean(dev, case, f32, accept_log, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORCED, ids=lambda c: c.name)
def test_planner_at_forced_thresholds(dev, accept_log, tmp_path, case):
    run_clean(dev, case, False, accept_log, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("case,flag,at,role", FLAGS, ids=FLAG_IDS)
def test_planner_raises_each_flag_alone(dev, accept_log, tmp_path, case, flag, at, role):
    """Up to the launch at which the flag rises every batch is bit-equal to the replay and head.error is the replay's
    prediction; the flag is still set behind the next launch; every guard holds throughout (dp_* return -2 otherwise)."""
    _, batches = case.replay()
    pl = Planner(dev, case, False)
    try:
        risen = False
        seq = launches(case)
        for i, (what, scanned, resolved, recorded) in enumerate(seq):
            call(pl, what)
            rises = (role == "scan" and scanned == at) or (role == "resolve" and resolved == at)
            if rises:
                assert int(pl.head()["error"]) == flag
                risen = True
                # the batches in front of the flagged one: the records made by this very launch are theirs
                if recorded is not None and recorded < at:
                    check_recs(pl, batches, recorded, accept_log, tmp_path)
                if role == "scan" and resolved is not None:
                    check_head(pl, batches, resolved, flag)
                    check_batch(pl, batches, resolved)
                assert i + 1 < len(seq)
                call(pl, seq[i + 1][0])
                assert int(pl.head()["error"]) & flag == flag  # sticky
                break
            if resolved is not None:
                check_head(pl, batches, resolved, 0)
                check_batch(pl, batches, resolved)
            else:
                assert int(pl.head()["error"]) == 0
            if recorded is not None:
                check_recs(pl, batches, recorded, accept_log, tmp_path)
            if scanned is not None and scanned < at:
                check_lists(pl, case, scanned)
        assert risen
    finally:
        pl.close()
