"""Every lane mapping of every kernel family, stepped against the oracle at the edges of its range of D.

A step kernel is built once per lane mapping: LPW lanes x EPL elements hold one walker (lane_map in step_plan.hpp chooses it
from D and the element size), and build::make (launch_build.hpp) fills one launch-table slot per mapping with a half-step
kernel (with and without its draw wavefront, for one and for several chains), a full-step kernel, a calc_logp kernel and a
differential-evolution update kernel; the batch mover has a propose / accept pair per mapping.  The mapping decides whether a
walker's tail sits in a half-filled lane, whether rows are read as 16-byte vectors, how many lanes idle, and whether
Rosenbrock's x[i+1] and the tree sum reach the right neighbour across lanes.  The oracle is sequential CPU code that knows
nothing of lanes.

CPU: SLOT_TABLE below is written down as data; tests/cpp/lane_map_cases.cpp (host compiler, step_plan.hpp alone) prints
lane_map for D = 1..1024 in both element types and must agree with it; the table's slots must be the ones build::make fills;
and the oracle alone is run over the whole case matrix to show that every case meets its input conditions (no near tie, no
redraw for the stretch move, proposals accepted and rejected in each run), so that bit-equality is the right bar.

GPU: each slot [lo, hi] is run at D = lo (most idle lanes), hi - 1 (last lane partly filled, scalar rows) and hi (full lanes,
vector rows); fp32 adds hi - 2 (rows 8-byte but not 16-byte aligned); the first slot runs every D it holds.  The ensemble has
W = 2 n walkers, n the smallest odd integer >= max(D + 1, 2 wpb + 3) with wpb = 4 (64 / LPW) walkers per workgroup: two full
workgroups and a ragged one, a ragged last wavefront wherever a wavefront holds several walkers, a partner bound that is no
power of two.  run(3, interval=2) then run(1, interval=1): seven ensemble steps, an odd count, so the full-step kernels end
in their second buffer.  Chains, accepted counts, final state and the redraw / near-tie counters are compared bit for bit;
there is no tolerance anywhere."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po
from tests.test_batch_calc import CTarget, cb_lib  # noqa: F401  (the callback library's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

ISO, DENSE, ROSENBROCK = po.CALC_ISO_GAUSSIAN, po.CALC_DENSE_GAUSSIAN, po.CALC_ROSENBROCK
CALC_NAME = {ISO: "iso", DENSE: "dense", ROSENBROCK: "rosenbrock"}
DTYPE_NAME = {po.F64: "f64", po.F32: "f32"}
ELEM_SIZE = {po.F64: 8, po.F32: 4}
STRETCH, DE = po.MOVER_STRETCH, po.MOVER_DIFFERENTIAL_EVOLUTION
MOVER_NAME = {STRETCH: "stretch", DE: "de"}

# ---- the slots, as data: (LPW, EPL, lowest D, highest D) ----------------------------------------------------------------------
SLOT_TABLE = {
    po.F64: [(1, 2, 1, 2), (2, 2, 3, 4), (4, 2, 5, 8), (8, 2, 9, 16), (16, 2, 17, 32), (32, 2, 33, 64),
             (64, 2, 65, 128), (64, 4, 129, 256), (64, 8, 257, 512), (64, 16, 513, 1024)],
    po.F32: [(1, 4, 1, 4), (2, 4, 5, 8), (4, 4, 9, 16), (8, 4, 17, 32), (16, 4, 33, 64), (32, 4, 65, 128),
             (64, 4, 129, 256), (64, 8, 257, 512), (64, 16, 513, 1024)],
}
# the (log2 LPW, EPL shift) pairs build::make fills (EPL = (16 bytes / element size) << shift): ten in fp64, nine in fp32
BUILD_MAKE_SLOTS = {
    po.F64: {(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (6, 1), (6, 2), (6, 3)},
    po.F32: {(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (6, 1), (6, 2)},
}


def slot_pair(dtype, lpw, epl):
    return (lpw.bit_length() - 1, (epl * ELEM_SIZE[dtype] // 16).bit_length() - 1)


def slot_dims(dtype, lo, hi):
    """The dimensions a slot is run at."""
    if lo == 1:
        return list(range(lo, hi + 1))
    return sorted({lo, hi - 1, hi} | ({hi - 2} if dtype == po.F32 else set()))


def walkers_for(D, lpw):
    wpb = 4 * (64 // lpw)
    n = max(D + 1, 2 * wpb + 3)
    return 2 * (n | 1)


# ---- the case matrix ----------------------------------------------------------------------------------------------------------
SEED, SALT = 12345, 3
# The seed column of the case table: SEED but for the cases listed here by (mover, calculator, dtype, D), each with the input
# condition the default seed missed (test_oracle_runs_meet_their_input_conditions).  Chain k of a handle of several chains is
# seeded with the case's seed + k, by the library and here.
SEEDS = {
    # fp32, isotropic Gaussian, wide walkers: with SEED the oracle counts one near tie in its seven steps (the fp32 band is
    # 6e-7 of magnitudes that grow with D); the seeds below are the first after SEED without one
    (STRETCH, ISO, po.F32, 1023): 12346,
    (STRETCH, ISO, po.F32, 1024): 12346,
    (DE, ISO, po.F32, 256): 12346,
    (DE, ISO, po.F32, 512): 12348,  # (12346 and 12347: one near tie each)
    (DE, ISO, po.F32, 1022): 12346,
    (DE, ISO, po.F32, 1024): 12346,
}

# Two cuts, both for the oracle's cost (sequential CPU code; seven steps of the dense Gaussian take about 40 s at 2050 x 1023
# and 6 s at 1030 x 513, under 1 s at 514 x 255; the isotropic Gaussian and Rosenbrock under 0.5 s at 2050 x 1024):
#   1. the dense Gaussian above D = 256 runs one dimension per slot, hi - 1, for three steps: run(1, 2) then run(1, 1);
#   2. differential evolution has no counter-addressed (multi-threaded) oracle mode, so it leaves the dense Gaussian out of the
#      slot 513..1024 altogether; the isotropic Gaussian and Rosenbrock still step the update kernel of that slot.
DENSE_FULL_MATRIX_MAX_D = 256
DE_DENSE_MAX_D = 512
RUNS, SHORT_RUNS = ((3, 2), (1, 1)), ((1, 2), (1, 1))

Case = collections.namedtuple("Case", "mover calc dtype D lpw epl lo hi W runs")


def _cases(mover):
    out = []
    for dtype in (po.F64, po.F32):
        for lpw, epl, lo, hi in SLOT_TABLE[dtype]:
            for calc in (ISO, DENSE, ROSENBROCK):
                dims = slot_dims(dtype, lo, hi)
                if calc == DENSE and (lo, hi) == (17, 32):
                    dims = sorted(set(dims) | {18})  # an even D just above the slot's foot, for the matrix-core kernels
                for D in dims:
                    if calc == ROSENBROCK and D < 2:
                        continue  # (no neighbour to couple to: the target is constant, every proposal is accepted)
                    runs = RUNS
                    if calc == DENSE and D > DENSE_FULL_MATRIX_MAX_D:
                        if D != hi - 1 or (mover == DE and D > DE_DENSE_MAX_D):
                            continue
                        runs = SHORT_RUNS
                    out.append(Case(mover, calc, dtype, D, lpw, epl, lo, hi, walkers_for(D, lpw), runs))
    return out


STRETCH_CASES, DE_CASES = _cases(STRETCH), _cases(DE)


def case_id(c):
    return "%s-lpw%dx%d-D%d-%s" % (DTYPE_NAME[c.dtype], c.lpw, c.epl, c.D, CALC_NAME[c.calc])


def is_matrix_core_shape(c):
    """Where the dense Gaussian's step kernels are the matrix-core ones by default."""
    return c.calc == DENSE and 18 <= c.D <= 32 and c.D % 2 == 0


# ---- CPU: the table, lane_map, build::make ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lane_maps():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "lane_map_cases")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lane_map_cases.cpp"), "-I", CSRC])
    out = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n"):
        if line:
            elem_size, D, lpw, epl, vec_ok = map(int, line.split())
            out[(elem_size, D)] = (lpw, epl, vec_ok)
    return out


def test_lane_map_returns_the_slot_table(lane_maps):
    assert len(lane_maps) == 2 * 1024
    for dtype, slots in SLOT_TABLE.items():
        elem_size = ELEM_SIZE[dtype]
        covered = []
        for lpw, epl, lo, hi in slots:
            for D in range(lo, hi + 1):
                assert lane_maps[(elem_size, D)] == (lpw, epl, int(D % (16 // elem_size) == 0)), (DTYPE_NAME[dtype], D)
            covered += range(lo, hi + 1)
        assert covered == list(range(1, 1025))  # the ranges tile 1..1024 in order, without a gap


def _slots_put_by_build_make():
    """The put<T, Calc, log2 LPW, EPL shift>(t) lines of build::make, per element type."""
    text = open(os.path.join(CSRC, "launch_build.hpp")).read()
    body = text[text.index("LaunchTable<T> make()"):]
    body = body[:body.index("return t;")]
    found = {po.F64: set(), po.F32: set()}
    for line in body.split("\n"):
        m = re.search(r"put<T, Calc, (\d+), (\d+)>\(t\)", line)
        if not m:
            assert "put<" not in line, line
            continue
        pair = (int(m.group(1)), int(m.group(2)))
        if "sizeof(T) == 8" in line:
            found[po.F64].add(pair)
        else:
            assert "sizeof(T)" not in line, line
            found[po.F64].add(pair)
            found[po.F32].add(pair)
    return found


def test_slot_table_holds_the_slots_build_make_fills():
    """A slot added to build::make fails here until SLOT_TABLE, and with it the case matrix, covers it."""
    for dtype, slots in SLOT_TABLE.items():
        assert {slot_pair(dtype, lpw, epl) for lpw, epl, _, _ in slots} == BUILD_MAKE_SLOTS[dtype]
        assert len(slots) == len(BUILD_MAKE_SLOTS[dtype])
    assert (len(BUILD_MAKE_SLOTS[po.F64]), len(BUILD_MAKE_SLOTS[po.F32])) == (10, 9)
    assert _slots_put_by_build_make() == BUILD_MAKE_SLOTS


def test_case_matrix_hits_every_slot_at_its_edges(lane_maps):
    """Every slot, for each calculator and each family, at lo, hi - 1 and hi (fp32: hi - 2 too; the first slot: every D),
    but for the two stated cuts; the slot of a case is the one lane_map gives its D."""
    for cases, mover in ((STRETCH_CASES, STRETCH), (DE_CASES, DE)):
        for c in cases:
            assert lane_maps[(ELEM_SIZE[c.dtype], c.D)][:2] == (c.lpw, c.epl)
            assert c.W > 2 * c.D and (c.W // 2) % 2 == 1 and c.W // 2 >= 2 * 4 * (64 // c.lpw) + 3
        for dtype, slots in SLOT_TABLE.items():
            for lpw, epl, lo, hi in slots:
                for calc in (ISO, DENSE, ROSENBROCK):
                    have = sorted(c.D for c in cases if (c.dtype, c.lpw, c.epl, c.calc) == (dtype, lpw, epl, calc))
                    want = slot_dims(dtype, lo, hi)
                    if calc == ROSENBROCK:
                        want = [D for D in want if D >= 2]
                    if calc == DENSE and lo == 17:
                        want = sorted(set(want) | {18})
                    if calc == DENSE and lo > DENSE_FULL_MATRIX_MAX_D:
                        want = [] if (mover == DE and lo > DE_DENSE_MAX_D) else [hi - 1]
                    assert have == want, (MOVER_NAME[mover], DTYPE_NAME[dtype], lpw, epl, CALC_NAME[calc])
    # the only slot a family leaves out: differential evolution, dense Gaussian, 513..1024
    missing = {(c.dtype, c.lpw, c.epl, c.calc) for c in STRETCH_CASES} - {(c.dtype, c.lpw, c.epl, c.calc) for c in DE_CASES}
    assert missing == {(po.F64, 64, 16, DENSE), (po.F32, 64, 16, DENSE)}
    assert max(c.W for c in STRETCH_CASES) == 2050
    assert {c.W for c in STRETCH_CASES if c.lpw == 1} == {1030}


# ---- the oracle's side of every case, computed once ---------------------------------------------------------------------------

def params_for(calc, D, dtype, W):
    t = po.np_dtype(dtype)
    if calc == DENSE:
        a = np.random.default_rng(W + D).standard_normal((D, D))
        return (a @ a.T / D + np.eye(D)).astype(t).ravel()
    if calc == ROSENBROCK:
        return np.array([1.0, 100.0, 0.05], dtype=t)
    return None


OracleRun = collections.namedtuple("OracleRun", "seed params pos logp chains accepted state redraws near_ties nbytes")
_ORACLE_RUNS = collections.OrderedDict()
_ORACLE_CACHE_BYTES = 1 << 30  # the least recently used results beyond this are computed again when asked for


def oracle_run(c, chain=0):
    """What the oracle makes of case c (chain k of a handle of several chains: seed + k, a start of its own)."""
    key = (c.mover, c.calc, c.dtype, c.D, chain)
    if key in _ORACLE_RUNS:
        _ORACLE_RUNS.move_to_end(key)
        return _ORACLE_RUNS[key]
    seed = SEEDS.get(key[:4], SEED) + chain
    params = params_for(c.calc, c.D, c.dtype, c.W)
    orc = po.Oracle(c.W, c.D, c.calc, params, seed=seed, dtype=c.dtype, mover=c.mover)
    pos = po.init_positions(c.dtype, c.W, c.D, salt=SALT + chain)
    logp = orc.logp(pos)
    orc.set_state(pos, logp)
    chains, accepted = [], []
    for n_saved, interval in c.runs:
        if c.mover == STRETCH:
            ch, acc = orc.run(n_saved, interval=interval, mode=po.MODE_COUNTER, threads=8)
        else:
            ch, acc = orc.run(n_saved, interval=interval)
        chains.append(ch)
        accepted.append(acc)
    r = OracleRun(seed, params, pos, logp, chains, accepted, orc.get_state(), orc.redraws, orc.near_ties,
                  sum(a.nbytes for a in chains) + 2 * pos.nbytes + (0 if params is None else params.nbytes))
    for a in [pos, logp] + chains + accepted + list(r.state) + ([] if params is None else [params]):
        a.setflags(write=False)
    _ORACLE_RUNS[key] = r
    total = sum(v.nbytes for v in _ORACLE_RUNS.values())
    while total > _ORACLE_CACHE_BYTES and len(_ORACLE_RUNS) > 1:
        total -= _ORACLE_RUNS.popitem(last=False)[1].nbytes
    return r


def assert_input_conditions(c, r):
    """What makes bit-equality the right bar for this case, and the case a test of the accept as well as of the proposal."""
    assert r.near_ties == 0, "near ties: this case needs another seed"
    if c.mover == STRETCH:
        assert r.redraws == 0, "redraws: this case needs another seed"
    for (n_saved, interval), acc in zip(c.runs, r.accepted):
        assert acc.shape == (n_saved * interval,)
        assert 0 < int(acc.sum()) < c.W * n_saved * interval, "every proposal of a run accepted, or none: this case needs another seed"


def hi_minus_1(cases):
    """The case at D = hi - 1 of each slot and calculator (Rosenbrock in the slot 1..2 of fp64, where that is D = 1: hi)."""
    return [c for c in cases if c.D == (c.hi if c.calc == ROSENBROCK and c.hi - 1 < 2 else c.hi - 1)]


CONDITION_CASES = ([(c, 0) for c in STRETCH_CASES] + [(c, 1) for c in hi_minus_1(STRETCH_CASES)] + [(c, 0) for c in DE_CASES])


@pytest.mark.parametrize("c,chain", CONDITION_CASES, ids=["%s-%s-chain%d" % (MOVER_NAME[c.mover], case_id(c), k) for c, k in CONDITION_CASES])
def test_oracle_runs_meet_their_input_conditions(c, chain):
    assert_input_conditions(c, oracle_run(c, chain))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

KNOBS = ("MCMCPP_HIP_FULL_STEP", "MCMCPP_HIP_NO_DRAW_WAVE", "MCMCPP_HIP_PASSES", "MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS")
FULL, HALF = {"MCMCPP_HIP_FULL_STEP": "1"}, {"MCMCPP_HIP_FULL_STEP": "0"}
NO_DRAW_WAVE, PASSES_4, PLAIN = {"MCMCPP_HIP_NO_DRAW_WAVE": "1"}, {"MCMCPP_HIP_PASSES": "4"}, {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "-1"}
# path name -> (knobs, chains per handle)
STEP_PATHS = {"full_step": (FULL, 1), "half_step": (HALF, 1)}
# at D = hi - 1 of each slot: the instantiations without a draw wavefront, four passes, several chains per launch
EDGE_PATHS = {"full_step_no_draw_wave": ({**FULL, **NO_DRAW_WAVE}, 1), "half_step_no_draw_wave": ({**HALF, **NO_DRAW_WAVE}, 1),
              "half_step_passes_4": ({**HALF, **PASSES_4}, 1), "full_step_2_chains": (FULL, 2), "half_step_2_chains": (HALF, 2)}
# even D in 18..32, dense: the matrix-core kernels (the default) and the slot's plain kernels
DENSE_PATHS = {"full_step_matrix_core": (FULL, 1), "half_step_matrix_core": (HALF, 1),
               "full_step_plain": ({**FULL, **PLAIN}, 1), "half_step_plain": ({**HALF, **PLAIN}, 1)}


def set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def compare_with_oracle(hip, c, runs):
    """hip: a handle in its start state; runs: the oracle's result for each of its chains."""
    K = len(runs)
    one = (lambda a, k: a) if K == 1 else (lambda a, k: a[k])
    for i, (n_saved, interval) in enumerate(c.runs):
        chain, acc = hip.run(n_saved, interval=interval)
        for k, r in enumerate(runs):
            np.testing.assert_array_equal(one(acc, k), r.accepted[i], err_msg="accepted per step, run %d, chain %d" % (i, k))
            np.testing.assert_array_equal(one(chain, k), r.chains[i], err_msg="stored steps, run %d, chain %d" % (i, k))
    state = hip.get_state()
    for k, r in enumerate(runs):
        for got, want, what in zip(state, r.state, ("positions", "log-posteriors", "accepted per walker")):
            np.testing.assert_array_equal(one(got, k), want, err_msg="%s, chain %d" % (what, k))
    counters = hip.counters()
    assert counters["redraws"] == sum(r.redraws for r in runs)
    assert counters["near_ties"] == sum(r.near_ties for r in runs)


def step_and_compare(monkeypatch, c, knobs, chains=1, **kw):
    runs = [oracle_run(c, k) for k in range(chains)]
    for r in runs:
        assert_input_conditions(c, r)
    set_knobs(monkeypatch, knobs)
    hip = capi.HipSampler(c.W, c.D, c.calc, runs[0].params, seed=runs[0].seed, dtype=c.dtype, mover=c.mover, **kw)
    if chains == 1:
        hip.set_state(runs[0].pos, runs[0].logp)
    else:
        assert [r.seed for r in runs] == [runs[0].seed + k for k in range(chains)]  # (what the library seeds chain k with)
        hip.set_state(np.stack([r.pos for r in runs]), np.stack([r.logp for r in runs]))
    compare_with_oracle(hip, c, runs)


def _with_paths(cases, paths):
    return [pytest.param(c, path, id="%s-%s" % (case_id(c), path)) for c in cases for path in paths]


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("c,path", _with_paths(STRETCH_CASES, STEP_PATHS))
def test_stretch_step_kernels(monkeypatch, c, path):
    """The slot's full-step and half-step kernels (for the dense Gaussian at even D in 18..32 the matrix-core ones)."""
    knobs, chains = STEP_PATHS[path]
    step_and_compare(monkeypatch, c, knobs, chains)


@gpu
@pytest.mark.parametrize("c,path", _with_paths(hi_minus_1(STRETCH_CASES), EDGE_PATHS))
def test_stretch_step_kernel_variants_with_a_partly_filled_last_lane(monkeypatch, c, path):
    """The other instantiations of a slot, at D = hi - 1: without the draw wavefront (what the updating wavefronts do where
    the default carries one -- the half-step kernels while 3 * 4 * (64 / LPW) * passes <= 128), four passes, and two chains
    per launch, chain k against an oracle seeded seed + k."""
    knobs, chains = EDGE_PATHS[path]
    step_and_compare(monkeypatch, c, knobs, chains, **({"num_chains": chains} if chains > 1 else {}))


@gpu
@pytest.mark.parametrize("c,path", _with_paths([c for c in STRETCH_CASES if is_matrix_core_shape(c)], DENSE_PATHS))
def test_dense_plain_kernels_where_the_matrix_cores_take_over(monkeypatch, c, path):
    """Even D in 18..32: by default the dense Gaussian is stepped by the matrix-core kernels, which leaves the slot's own
    dense kernels (16 lanes x 2 in fp64, 8 lanes x 4 in fp32) to odd D; both are run here."""
    knobs, chains = DENSE_PATHS[path]
    step_and_compare(monkeypatch, c, knobs, chains)


DE_PATHS = {"default": {}}
DE_DENSE_PATHS = {"matrix_core": {}, "plain": PLAIN}


@gpu
@pytest.mark.parametrize("c,path", _with_paths([c for c in DE_CASES if not is_matrix_core_shape(c)], DE_PATHS)
                         + _with_paths([c for c in DE_CASES if is_matrix_core_shape(c)], DE_DENSE_PATHS))
def test_differential_evolution_update_kernels(monkeypatch, c, path):
    """de_update_kernel of every slot; redraws are expected here and must be the oracle's."""
    step_and_compare(monkeypatch, c, {**DE_PATHS, **DE_DENSE_PATHS}[path])


@gpu
@pytest.mark.parametrize("c", [c for c in STRETCH_CASES if c.calc == ISO], ids=case_id)
def test_batch_propose_and_accept_kernels(monkeypatch, cb_lib, c):  # noqa: F811
    """The batch mover's propose / accept pair of every slot (the calculator is outside these kernels: the isotropic Gaussian
    as a C callback), against the stretch move's own oracle result."""
    r = oracle_run(c)
    assert_input_conditions(c, r)
    set_knobs(monkeypatch, {})
    target = CTarget(cb_lib, c.calc, c.D, None, c.dtype)
    hip = capi.HipSampler(c.W, c.D, capi.CALC_BATCH, seed=r.seed, dtype=c.dtype, batch_callback=target.callback())
    hip.set_state(r.pos, r.logp)
    compare_with_oracle(hip, c, [r])
    del hip


def _calc_cases():
    out = []
    for dtype in (po.F64, po.F32):
        for lpw, epl, lo, hi in SLOT_TABLE[dtype]:
            for calc in (ISO, DENSE, ROSENBROCK):
                dims = set(slot_dims(dtype, lo, hi)) | ({18} if calc == DENSE and lo == 17 else set())
                out += [Case(None, calc, dtype, D, lpw, epl, lo, hi, walkers_for(D, lpw), None) for D in sorted(dims) if not (calc == ROSENBROCK and D < 2)]
    return out


@gpu
@pytest.mark.parametrize("c", _calc_cases(), ids=case_id)
def test_calc_logp_kernels(c):
    """calc_logp_kernel of every slot on 301 rows (no cut here: an evaluation costs the oracle nothing to speak of)."""
    t = po.np_dtype(c.dtype)
    params = params_for(c.calc, c.D, c.dtype, c.W)
    pos = (np.random.default_rng(c.D * 7 + c.calc).standard_normal((301, c.D)) * 1.5).astype(t)
    want = po.Oracle(c.W, c.D, c.calc, params, dtype=c.dtype).logp(pos)
    got = capi.HipSampler(c.W, c.D, c.calc, params, dtype=c.dtype).calc_logp(pos)
    np.testing.assert_array_equal(got, want)
