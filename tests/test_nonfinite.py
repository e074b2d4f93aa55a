"""Non-finite log-posteriors on every step path.

A target with a bounded prior returns -inf outside its support; a target can also return NaN or +inf.  The reference decides
such proposals by plain IEEE comparison (StretchMove.h:112-113 accepts iff lnU < probScaling + newProb - oldProb,
DifferentialEvolution.h:134 iff newProb - oldProb > -exp): an -inf proposal is rejected, a walker that starts at -inf takes
the first finite proposal, -inf against -inf is NaN and the walker stays, a NaN never wins, a +inf proposal always wins and
the walker then never moves again.  The oracle is pinned to the compiled reference on exactly these inputs by the boxed
fixtures (tests/golden/boxed64x4*.npz, de_boxed64x4*.npz; tests/test_oracle_golden.py, tests/test_diffevo.py); here every
device path is compared with the oracle, bit for bit: chain, positions, log-posteriors, accepted per step, per-walker
counters (np.testing.assert_array_equal: a NaN equals a NaN whatever its sign and payload, which differ between x86 and
gfx950; everything else is compared exactly), near_ties == 0 on both sides, redraws equal.

Every run first checks, on the ORACLE's side, that its inputs exercise what it is there for (oracle_boxed_run,
oracle_overflow_run): the CPU tests below run those checks alone, the GPU tests run them again in front of the comparison.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi, workloads
from oracle import pyoracle as po
from tests.goldens import BOXED, DE_BOXED, Golden, boxed_start, in_box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
BOXED_ISO = 1002  # the plug-in's calculator id (ids from 1000 are the user's; tests/test_plugin.py registers 1000 and 1001)
OUTSIDES = [-np.inf, np.nan, np.inf]
ROSEN = [1.0, 100.0, 0.05]


def _name(v):
    return {"-inf": "minus_inf", "nan": "nan", "inf": "plus_inf"}[str(float(v))]


# ---- the oracle's side of every run, with the conditions its inputs must meet ------------------------------------------

class Run:
    pass


def _check_boxed_conditions(r):
    """The conditions a boxed run must meet to test anything, asserted on what the ORACLE did."""
    W, hw, outside = r.W, r.half_width, r.outside
    proposals = W * r.acc.size
    # at least 10 % of all proposals left the box (with -inf and NaN outside every one of them is a rejection: that no walker
    # ever took one is the monotonicity check below); at least 10 % of all proposals were accepted
    assert r.left_box >= 0.10 * proposals, "only %d of %d proposals left the box" % (r.left_box, proposals)
    assert int(r.acc.sum()) >= 0.10 * proposals, "only %d of %d proposals were accepted" % (int(r.acc.sum()), proposals)
    assert np.all(np.isfinite(r.chain)) and r.near_ties == 0
    start_in = in_box(r.pos, hw)
    assert not start_in[r.started_outside].any() and start_in.sum() == W - r.started_outside.size and r.started_outside.size >= 1
    inb = np.concatenate([start_in[None], in_box(r.chain, hw)])  # [1 + stored steps][W]
    end_pos, end_lp, nacc = r.state
    if np.isneginf(outside):
        assert in_box(end_pos, hw)[r.started_outside].any(), "no walker that started outside the support joined"
    if not np.isposinf(outside):
        # a walker that was ever inside never holds a position outside
        assert np.all(inb[1:] >= inb[:-1])
        assert np.all(np.isfinite(end_lp[in_box(end_pos, hw)]))
    if np.isnan(outside):
        # the walkers that started at NaN never moved
        assert np.all(nacc[r.started_outside] == 0) and np.all(r.chain[:, r.started_outside] == r.pos[r.started_outside])
        assert np.all(np.isnan(end_lp[r.started_outside]))
    if np.isposinf(outside):
        # +inf wins every comparison and then loses every one: the walkers that started outside never moved, and a walker that
        # left the box sits where it landed ever after
        assert np.all(nacc[r.started_outside] == 0) and np.all(r.chain[:, r.started_outside] == r.pos[r.started_outside])
        full = np.concatenate([r.pos[None], r.chain])
        out = ~inb
        assert np.all(out[1:] >= out[:-1])
        stays = out[:-1]  # outside at step k: the same row at step k + 1
        assert np.all(full[1:][stays] == full[:-1][stays])
        assert np.all(np.isposinf(end_lp[~in_box(end_pos, hw)]))
        assert (~in_box(end_pos, hw)).sum() > r.started_outside.size, "no walker escaped to +inf"


def oracle_boxed_run(W, D, dtype, mover, half_width, outside, steps, seed, interval=1, salt=0, start=None, spread=0.9, push=1.5):
    """The oracle's run of the boxed target from tests/goldens.boxed_start (or start = (pos, logp) of a fixture)."""
    r = Run()
    t = po.np_dtype(dtype)
    r.W, r.D, r.dtype, r.mover, r.half_width, r.outside, r.steps, r.interval, r.seed = W, D, dtype, mover, half_width, outside, steps, interval, seed
    r.params = np.array([half_width, outside], dtype=t)
    orc = po.Oracle(W, D, po.CALC_BOXED_ISO_GAUSSIAN, r.params, seed=seed, dtype=dtype, mover=mover)
    if start is None:
        r.pos, r.started_outside = boxed_start(dtype, W, D, half_width, salt=salt, spread=spread, push=push)
        r.lp = orc.logp(r.pos)
    else:
        r.pos, r.lp = start
        r.started_outside = np.flatnonzero(~in_box(r.pos, half_width))
    orc.set_state(r.pos, r.lp)
    before = po.boxed_outside_evals()
    if mover == po.MOVER_STRETCH:
        r.chain, r.acc = orc.run(steps, interval=interval, mode=po.MODE_COUNTER, threads=4)
    else:
        r.chain, r.acc = orc.run(steps, interval=interval)
    r.left_box = po.boxed_outside_evals() - before
    r.state = orc.get_state()
    r.near_ties, r.redraws = orc.near_ties, orc.redraws
    if interval == 1:
        _check_boxed_conditions(r)
    return r


# Fresh shapes: W, D, stored steps, and per mover (stretch, differential evolution) the half width and the start
# (tests/goldens.boxed_start: spread, push), chosen with the oracle so that every run meets _check_boxed_conditions.  A proposal
# leaves the box when ANY coordinate does, so the box grows with D under the stretch move; the differential-evolution step is
# gamma (w1 - w2) with gamma = 2.38 / sqrt(2 D), so there the ensemble starts closer together and the outside walkers closer
# to the box.  +inf runs are short: every walker leaves the box within a few steps and freezes, after which nothing is accepted.
FRESH = {
    "34x3": dict(W=34, D=3, steps=150, start=(dict(half_width=1.25), dict(half_width=1.25))),
    "6x2": dict(W=6, D=2, steps=300, start=(dict(half_width=1.25), dict(half_width=1.25))),
    "4098x32": dict(W=4098, D=32, steps=20, start=(dict(half_width=4.0), dict(half_width=1.0, spread=0.6, push=1.05))),
    # (seed 5 meets an fp32 near tie between finite operands under differential evolution here: another seed)
    "1026x130": dict(W=1026, D=130, steps=12, start=(dict(half_width=4.0), dict(half_width=1.0, spread=0.6, push=1.05, seed=6))),
}
PINF_STEPS = 8


@functools.lru_cache(maxsize=48)  # (the step paths share one oracle run; nothing writes to it)
def fresh_run(shape, dtype, mover, outside):
    c = FRESH[shape]
    steps = PINF_STEPS if np.isposinf(outside) else c["steps"]
    return oracle_boxed_run(c["W"], c["D"], dtype, mover, outside=outside, steps=steps, salt=7, **dict(dict(seed=5), **c["start"][mover]))


@functools.lru_cache(maxsize=48)  # (the step paths share one oracle run; nothing writes to it)
def fixture_run(name):
    g = Golden(name)
    assert g.calc == po.CALC_BOXED_ISO_GAUSSIAN and g.slicing == 1
    r = oracle_boxed_run(g.W, g.D, g.dtype, g.mover, float(g.params[0]), float(g.params[1]), g.steps, g.seed, start=(g.init_pos, g.init_logp))
    for k in g.checked_steps:
        g.check_chain_step(k, r.chain[k - 1])
    np.testing.assert_array_equal(r.acc, g.accepted_per_call)
    return g, r


def overflow_start(dtype, W, D, calc, params, salt=3, stated=True):
    """Initial state with walkers outside what the element type can square: every eighth walker sits at 1e200 * x (fp64) or
    1e30 * x (fp32), so that its log-posterior is not finite; with stated=True two more walkers in sixteen keep their finite
    position but are GIVEN a log-posterior of NaN (w % 16 == 2) or -inf (w % 16 == 10), which set_state takes as stated."""
    t = po.np_dtype(dtype)
    pos = po.init_positions(dtype, W, D, salt=salt)
    far = np.arange(5, W, 8)
    pos[far] *= t(1e200 if dtype == po.F64 else 1e30)
    assert np.all(np.isfinite(pos))
    lp = po.Oracle(W, D, calc, params, dtype=dtype).logp(pos)
    assert not np.isfinite(lp[far]).any() and np.all(np.isfinite(np.delete(lp, far)))
    nan_w, ninf_w = np.arange(2, W, 16), np.arange(10, W, 16)
    if stated:
        lp[nan_w] = np.nan
        lp[ninf_w] = -np.inf
    return pos, lp, far, (nan_w if stated else nan_w[:0]), (ninf_w if stated else ninf_w[:0])


def oracle_overflow_run(W, D, dtype, calc, params, steps, seed, interval=1, mover=po.MOVER_STRETCH, salt=3, stated=True):
    r = Run()
    r.W, r.D, r.dtype, r.params, r.steps, r.interval, r.seed = W, D, dtype, params, steps, interval, seed
    r.pos, r.lp, far, nan_w, ninf_w = overflow_start(dtype, W, D, calc, params, salt=salt, stated=stated)
    orc = po.Oracle(W, D, calc, params, seed=seed, dtype=dtype, mover=mover)
    orc.set_state(r.pos, r.lp)
    if mover == po.MOVER_STRETCH:
        r.chain, r.acc = orc.run(steps, interval=interval, mode=po.MODE_COUNTER, threads=4)
    else:
        r.chain, r.acc = orc.run(steps, interval=interval)
    r.state = orc.get_state()
    r.near_ties, r.redraws = orc.near_ties, orc.redraws
    end_pos, end_lp, nacc = r.state
    # the walkers that overflow and those stated NaN never move; those stated -inf join; nothing becomes non-finite; the rest of
    # the ensemble samples on; and none of these decisions is a near tie
    frozen = np.concatenate([far, nan_w])
    assert np.all(nacc[frozen] == 0) and np.all(end_pos[frozen] == r.pos[frozen]) and np.all(r.chain[:, frozen] == r.pos[frozen])
    assert np.all(np.isfinite(r.chain)) and np.all(np.isfinite(end_pos))
    if ninf_w.size:
        assert np.all(nacc[ninf_w] >= 1) and np.all(np.isfinite(end_lp[ninf_w]))
    moving = np.setdiff1d(np.arange(W), frozen)
    assert np.all(np.isfinite(end_lp[moving]))
    assert int(r.acc.sum()) >= 0.10 * moving.size * r.acc.size
    assert r.near_ties == 0, "%d near ties: pick another seed" % r.near_ties
    r.frozen = frozen
    return r


# ---- CPU: the near-tie rule and the input conditions ------------------------------------------------------------------

@pytest.mark.parametrize("mover", [po.MOVER_STRETCH, po.MOVER_DIFFERENTIAL_EVOLUTION])
@pytest.mark.parametrize("dtype", [po.F64, po.F32])
@pytest.mark.parametrize("calc,params", [(po.CALC_ISO_GAUSSIAN, None), (po.CALC_ROSENBROCK, ROSEN)])
def test_a_proposal_outside_the_support_is_no_near_tie(calc, params, dtype, mover):
    """64 x 4, eight walkers started where their log-posterior is -inf, 200 steps.  Before the rule counted finite decisions
    only, the oracle reported 1298 (stretch) and 2694 (differential evolution) near ties here, and none without those walkers."""
    W, D = 64, 4
    r = oracle_overflow_run(W, D, dtype, calc, params, 200, seed=0, mover=mover, salt=0, stated=False)
    assert r.near_ties == 0 and r.frozen.size == 8
    assert np.all(np.isneginf(r.state[1][r.frozen]))
    assert int(r.acc.sum()) > (3000 if mover == po.MOVER_STRETCH else 1000)  # (the other 56 walkers sample on)


def test_near_tie_count_of_finite_runs_is_unchanged():
    """Decisions between finite operands are flagged as before: an fp32 run long enough to meet some, whose number was the same
    before the finite-margin rule."""
    W, D = 4102, 32
    P = workloads.ar1_precision(D, 0.5).ravel()
    orc = po.Oracle(W, D, po.CALC_DENSE_GAUSSIAN, P, seed=77, dtype=po.F32)
    pos = po.init_positions(po.F32, W, D, salt=3)
    orc.set_state(pos, orc.logp(pos))
    orc.run(60, save_chain=False, mode=po.MODE_COUNTER, threads=4)
    assert orc.near_ties == 2  # (measured with the oracle of the parent commit, and with this one)
    hs, w, accepted, ln_u, delta = orc.last_near_tie()
    assert np.isfinite(ln_u) and np.isfinite(delta)


@pytest.mark.parametrize("name", BOXED + DE_BOXED)
def test_fixture_runs_meet_their_input_conditions(name):
    g, r = fixture_run(name)
    assert r.near_ties == 0
    assert r.redraws == 0 or g.mover == po.MOVER_DIFFERENTIAL_EVOLUTION


@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("mover", [po.MOVER_STRETCH, po.MOVER_DIFFERENTIAL_EVOLUTION], ids=["stretch", "de"])
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(FRESH))
def test_fresh_runs_meet_their_input_conditions(shape, dtype, mover, outside):
    fresh_run(shape, dtype, mover, outside)


CHAIN_HALF_WIDTHS = (1.0, 1.25, 1.6)


@functools.lru_cache(maxsize=48)  # (the step paths share one oracle run; nothing writes to it)
def chains_runs(dtype, outside):
    """Three chains of 1024 x 7 with a half width each (chain k: seed + k, as the handle seeds its chains)."""
    steps = PINF_STEPS if np.isposinf(outside) else 30
    return [oracle_boxed_run(1024, 7, dtype, po.MOVER_STRETCH, hw, outside, steps, 40 + k, salt=50 + k) for k, hw in enumerate(CHAIN_HALF_WIDTHS)]


@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
def test_chain_runs_meet_their_input_conditions(dtype, outside):
    chains_runs(dtype, outside)


# ---- GPU (a): the calculators at the edges ------------------------------------------------------------------------------

def _edge_rows(D, t, rng):
    """Rows for a calculator: all +0, all -0, denormals, the largest finite value, a value whose square overflows, +inf, -inf
    and NaN -- each as a whole row and in one coordinate of an ordinary row at a time: the first, the last, and either side
    of every 16-element boundary."""
    fi = np.finfo(t)
    specials = [t(0.0), t(-0.0), fi.smallest_subnormal, -fi.smallest_subnormal * 3, fi.tiny / 4, fi.max, -fi.max,
                t(1e200 if t == np.float64 else 1e30), t(np.inf), t(-np.inf), t(np.nan)]
    where = sorted({0, D - 1} | {p for b in range(16, D, 16) for p in (b - 1, b)})
    rows = []
    for v in specials:
        rows.append(np.full(D, v, dtype=t))
        for p in where:
            x = (rng.standard_normal(D) * 1.5).astype(t)
            x[p] = v
            rows.append(x)
    return np.stack(rows), len(where) + 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("calc,D", [(po.CALC_ISO_GAUSSIAN, 1), (po.CALC_ISO_GAUSSIAN, 2), (po.CALC_ISO_GAUSSIAN, 7), (po.CALC_ISO_GAUSSIAN, 32),
                                    (po.CALC_ISO_GAUSSIAN, 100), (po.CALC_ISO_GAUSSIAN, 513), (po.CALC_ISO_GAUSSIAN, 1024),
                                    (po.CALC_DENSE_GAUSSIAN, 3), (po.CALC_DENSE_GAUSSIAN, 26), (po.CALC_DENSE_GAUSSIAN, 32),
                                    (po.CALC_DENSE_GAUSSIAN, 64), (po.CALC_DENSE_GAUSSIAN, 130),
                                    (po.CALC_ROSENBROCK, 2), (po.CALC_ROSENBROCK, 5), (po.CALC_ROSENBROCK, 32), (po.CALC_ROSENBROCK, 33),
                                    (po.CALC_ROSENBROCK, 300), (po.CALC_SKEWED_GAUSSIAN_2D, 2)])
def test_device_calculators_bit_exact_at_the_edges(calc, D, dtype):
    """calc_logp of every built-in target on the rows of _edge_rows against the oracle's.  The dense Gaussian's precision
    matrix is the AR(1) one, which is tridiagonal: its exact zeros meet the infinities (0 * inf) in the row dot products.

    What the oracle makes of these rows is the bar, NaN included (its calculators are the reference-pinned host twins).  It
    turns into NaN, not -inf: every row with a NaN, under every target; under the dense Gaussian from D = 3 on, every row with
    an infinite coordinate (0 * inf in the fma chain of a matrix row that does not touch that coordinate; inf - inf in the
    tree for the rows that are infinite throughout).  The isotropic Gaussian gives -inf for every row with an infinite or
    overflowing coordinate.  Rows of zeros and denormals are finite under every target.  All of that is asserted below on the
    oracle's values before the device is asked."""
    t = po.np_dtype(dtype)
    rng = np.random.default_rng(1000 * calc + D)
    W = 2 * D + 2
    params = {po.CALC_DENSE_GAUSSIAN: workloads.ar1_precision(D, 0.5).astype(t).ravel() if calc == po.CALC_DENSE_GAUSSIAN else None,
              po.CALC_ROSENBROCK: np.array(ROSEN, dtype=t), po.CALC_SKEWED_GAUSSIAN_2D: np.array([0.13], dtype=t)}.get(calc)
    rows, per_special = _edge_rows(D, t, rng)
    with np.errstate(all="ignore"):
        want = po.Oracle(W, D, calc, params, dtype=dtype).logp(rows)
    # the inputs do reach every kind of result
    by_special = want.reshape(-1, per_special)
    assert np.all(np.isnan(by_special[10]))                      # NaN rows
    assert np.all(np.isfinite(by_special[:5]))                   # zeros and denormals
    if calc == po.CALC_ISO_GAUSSIAN:
        assert np.all(np.isneginf(by_special[5:10]))
    if calc == po.CALC_DENSE_GAUSSIAN and D >= 3:
        assert np.all(np.isnan(by_special[8:10]))                # 0 * inf
    got = capi.HipSampler(W, D, calc, params, dtype=dtype).calc_logp(rows)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(np.signbit(got[np.isfinite(want)]), np.signbit(want[np.isfinite(want)]))  # (-0 against +0)


# ---- GPU (b): the bounded target through the plug-in functor, the C callback and the torch target ---------------------

@pytest.fixture(params=["full_step", "half_step"])
def step_path(request, monkeypatch):
    """Small ensembles step with one launch per ensemble step, large ones with one per half-step: both."""
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "1" if request.param == "full_step" else "0")
    return request.param


@pytest.fixture(scope="module")
def plugin():
    from tests.test_plugin import OUT, SRC
    capi.build_library()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    hdr_dir = os.path.join(ROOT, "mcmcpp_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(hdr_dir, f)) for f in os.listdir(hdr_dir) if f.endswith((".hpp", ".inc")))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(newest, os.path.getmtime(SRC)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-fno-fast-math", "-fPIC", "-shared", "-mllvm", "-amdgpu-kernarg-preload-count=16",
                               "-I" + hdr_dir, SRC, "-o", OUT])
    lib = C.CDLL(OUT)
    tables = []
    for t in ("f64", "f32"):
        f = getattr(lib, "mcmcpp_hip_plugin_boxed_iso_%s" % t)
        f.restype = C.c_void_p
        tables.append(f())
        assert tables[-1]
    L = capi.lib()
    L.mcmcpp_hip_register_calculator.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    assert L.mcmcpp_hip_register_calculator(BOXED_ISO, tables[0], tables[1], 2) == 0
    return L


@pytest.fixture(scope="module")
def cb_lib():
    from tests.test_batch_calc import HIPCC
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "batch_calc.hip")
    out = os.path.join(BUILD, "libbatch_calc.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.check_call(HIPCC + [src, "-o", out])
    L = C.CDLL(out)
    L.batch_calc_create.restype = C.c_void_p
    L.batch_calc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.batch_calc_destroy.argtypes = [C.c_void_p]
    L.batch_calc_outside.argtypes = [C.c_void_p]
    L.batch_calc_outside.restype = C.c_int64
    L.batch_calc_calls.argtypes = [C.c_void_p]
    L.batch_calc_calls.restype = C.c_int64
    return L


def _torch_boxed(half_width, outside):
    """The boxed target in torch: the in-box value by the built-in's host twin (tests/test_batch_calc._torch_iso: its bits)."""
    import torch
    from tests.test_batch_calc import _torch_iso

    def fn(x):
        lp = _torch_iso(x)
        inside = (x.abs() <= half_width).all(dim=1)
        return torch.where(inside, lp, torch.full_like(lp, outside))
    return fn


def _compare(s, r, chain=None):
    """Run the handle from the oracle run's start and compare everything with what the oracle got."""
    s.set_state(r.pos, r.lp)
    hc, ha = s.run(r.steps, interval=r.interval)
    np.testing.assert_array_equal(ha, r.acc, err_msg="accepted per step")
    np.testing.assert_array_equal(hc, r.chain, err_msg="chain")
    for a, b, what in zip(s.get_state(), r.state, ("positions", "logp", "n_accept")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    c = s.counters()
    assert c["accepted"] == int(r.acc.sum()) and c["ensemble_steps"] == r.steps * r.interval
    assert c["near_ties"] == 0 == r.near_ties
    assert c["redraws"] == r.redraws


def _plugin_sampler(r, **kw):
    return capi.HipSampler(r.W, r.D, BOXED_ISO, r.params, seed=r.seed, dtype=r.dtype, mover=r.mover, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOXED + DE_BOXED)
def test_plugin_functor_reproduces_the_boxed_fixtures(plugin, name, step_path):
    g, r = fixture_run(name)
    s = _plugin_sampler(r)
    np.testing.assert_array_equal(s.calc_logp(g.init_pos), g.init_logp)
    _compare(s, r)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOXED + DE_BOXED)
def test_plugin_functor_reproduces_the_boxed_fixtures_without_graphs(plugin, name):
    g, r = fixture_run(name)
    _compare(_plugin_sampler(r, graph_steps=-1), r)


@pytest.mark.gpu
@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(FRESH))
def test_plugin_functor_equals_the_oracle_under_the_stretch_move(plugin, shape, dtype, outside, step_path):
    r = fresh_run(shape, dtype, po.MOVER_STRETCH, outside)
    s = _plugin_sampler(r)
    np.testing.assert_array_equal(s.calc_logp(r.pos), r.lp)
    _compare(s, r)


@pytest.mark.gpu
@pytest.mark.parametrize("graph_steps", [0, -1])
@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(FRESH))
def test_plugin_functor_equals_the_oracle_under_differential_evolution(plugin, shape, dtype, outside, graph_steps):
    r = fresh_run(shape, dtype, po.MOVER_DIFFERENTIAL_EVOLUTION, outside)
    _compare(_plugin_sampler(r, graph_steps=graph_steps), r)


@pytest.mark.gpu
@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", ["34x3", "4098x32"])
def test_plugin_functor_equals_the_oracle_without_graphs(plugin, shape, dtype, outside, step_path):
    r = fresh_run(shape, dtype, po.MOVER_STRETCH, outside)
    _compare(_plugin_sampler(r, graph_steps=-1), r)


@pytest.mark.gpu
@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
def test_plugin_functor_with_a_half_width_per_chain(plugin, dtype, outside, step_path):
    """Three chains of 1024 x 7 in one launch, each with its own half width (mcmcpp_hip_set_chain_params)."""
    runs = chains_runs(dtype, outside)
    K, r0 = len(runs), runs[0]
    s = capi.HipSampler(r0.W, r0.D, BOXED_ISO, np.stack([r.params for r in runs]), seed=r0.seed, dtype=dtype, num_chains=K)
    for k, r in enumerate(runs):
        np.testing.assert_array_equal(s.calc_logp(r.pos, chain=k), r.lp, err_msg="chain %d" % k)
    s.set_state(np.stack([r.pos for r in runs]), np.stack([r.lp for r in runs]))
    hc, ha = s.run(r0.steps)
    pos, lp, nacc = s.get_state()
    for k, r in enumerate(runs):
        np.testing.assert_array_equal(ha[k], r.acc, err_msg="chain %d" % k)
        np.testing.assert_array_equal(hc[k], r.chain, err_msg="chain %d" % k)
        for a, b, what in zip((pos[k], lp[k], nacc[k]), r.state, ("positions", "logp", "n_accept")):
            np.testing.assert_array_equal(a, b, err_msg="chain %d %s" % (k, what))
    c = s.counters()
    assert c["near_ties"] == 0 and c["redraws"] == sum(r.redraws for r in runs)
    assert c["accepted"] == sum(int(r.acc.sum()) for r in runs)


def _c_callback_sampler(L, r, **kw):
    user = L.batch_calc_create(4, r.dtype, r.D, r.params.ctypes.data, 2)
    assert user
    s = capi.HipSampler(r.W, r.D, capi.CALC_BATCH, seed=r.seed, dtype=r.dtype, batch_callback=(C.cast(L.batch_calc_logp, C.c_void_p).value, user), **kw)
    return s, user


def _c_callback_case(L, r):
    s, user = _c_callback_sampler(L, r)
    try:
        _compare(s, r)
        # every proposal went through the callback, those outside the box included, and its -inf / NaN / +inf came back verbatim
        assert L.batch_calc_calls(user) == 2 * r.steps * r.interval
        assert L.batch_calc_outside(user) == r.left_box
    finally:
        s.close()
        L.batch_calc_destroy(user)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOXED)
def test_c_callback_reproduces_the_boxed_fixtures(cb_lib, name):
    _c_callback_case(cb_lib, fixture_run(name)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(FRESH))
def test_c_callback_equals_the_oracle(cb_lib, shape, dtype, outside):
    _c_callback_case(cb_lib, fresh_run(shape, dtype, po.MOVER_STRETCH, outside))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOXED)
def test_torch_target_reproduces_the_boxed_fixtures(name):
    g, r = fixture_run(name)
    s = capi.HipSampler(r.W, r.D, capi.CALC_BATCH, seed=r.seed, dtype=r.dtype, log_prob=_torch_boxed(r.half_width, r.outside))
    np.testing.assert_array_equal(s.calc_logp(g.init_pos), g.init_logp)
    _compare(s, r)


@pytest.mark.gpu
@pytest.mark.parametrize("outside", OUTSIDES, ids=_name)
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(FRESH))
def test_torch_target_equals_the_oracle(shape, dtype, outside):
    r = fresh_run(shape, dtype, po.MOVER_STRETCH, outside)
    s = capi.HipSampler(r.W, r.D, capi.CALC_BATCH, seed=r.seed, dtype=r.dtype, log_prob=_torch_boxed(r.half_width, r.outside))
    _compare(s, r)


# ---- GPU (c): built-in targets with walkers that overflow (these reach the matrix-core kernels) ----------------------

OVERFLOW_SEEDS = {}  # (calc, W, D, dtype): a seed with which the oracle meets no near tie (fp32 runs of this size meet a few otherwise)


def _builtin_params(calc, D, t):
    if calc == po.CALC_DENSE_GAUSSIAN:
        return workloads.ar1_precision(D, 0.5).astype(t).ravel()
    return np.array(ROSEN, dtype=t)


@functools.lru_cache(maxsize=48)  # (the step paths share one oracle run; nothing writes to it)
def builtin_overflow_run(calc, W, D, dtype, steps, interval, mover=po.MOVER_STRETCH, seed=None, salt=3):
    seed = OVERFLOW_SEEDS.get((calc, W, D, dtype, mover), 77) if seed is None else seed
    r = oracle_overflow_run(W, D, dtype, calc, _builtin_params(calc, D, po.np_dtype(dtype)), steps, seed, interval=interval, mover=mover, salt=salt)
    r.calc, r.mover = calc, mover
    return r


def _builtin_sampler(r, **kw):
    return capi.HipSampler(r.W, r.D, r.calc, r.params, seed=r.seed, dtype=r.dtype, mover=r.mover, **kw)


MATRIX_CORE_SHAPES = [(4096 + 6, 32), (600, 18), (2048, 26)]           # test_matrix_core_kernel_is_bit_exact
LATE_DRAW_SHAPES = [(8192 + 74, 32), (2048 + 6, 26)]                   # test_matrix_core_kernel_with_late_draws_...


@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("calc", [po.CALC_DENSE_GAUSSIAN, po.CALC_ROSENBROCK], ids=["dense", "rosenbrock"])
@pytest.mark.parametrize("W,D", MATRIX_CORE_SHAPES)
def test_overflow_runs_meet_their_input_conditions(W, D, calc, dtype):
    builtin_overflow_run(calc, W, D, dtype, 15, 2)


@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("W,D", LATE_DRAW_SHAPES + [(8192 + 10, 32)])
def test_large_overflow_runs_meet_their_input_conditions(W, D, dtype):
    builtin_overflow_run(po.CALC_DENSE_GAUSSIAN, W, D, dtype, 7, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("calc", [po.CALC_DENSE_GAUSSIAN, po.CALC_ROSENBROCK], ids=["dense", "rosenbrock"])
@pytest.mark.parametrize("W,D", MATRIX_CORE_SHAPES)
def test_matrix_core_kernels_with_walkers_that_overflow(monkeypatch, W, D, calc, dtype, step_path):
    """The shapes and switches of test_matrix_core_kernel_is_bit_exact: padded rows and columns of the tiles are multiplied by
    whatever the walker holds (0 * 1e200 is 0; 0 * inf would be NaN), ragged last wavefronts."""
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS", "0")
    r = builtin_overflow_run(calc, W, D, dtype, 15, 2)
    s = _builtin_sampler(r)
    np.testing.assert_array_equal(s.calc_logp(r.pos[r.frozen[:8]]), po.Oracle(W, D, calc, r.params, dtype=dtype).logp(r.pos[r.frozen[:8]]))
    _compare(s, r)


@pytest.mark.gpu
def test_sixteen_walkers_per_wavefront_fp32_with_walkers_that_overflow(monkeypatch):
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "0")
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS", "1")
    r = builtin_overflow_run(po.CALC_DENSE_GAUSSIAN, 8192 + 10, 32, po.F32, 7, 2)
    _compare(_builtin_sampler(r), r)


@pytest.mark.gpu
@pytest.mark.parametrize("late", ["0", "-1"])
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("W,D", LATE_DRAW_SHAPES)
def test_late_draw_kernels_with_walkers_that_overflow(monkeypatch, W, D, dtype, late):
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "0")
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS", "0")
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS", "1")
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS", late)
    r = builtin_overflow_run(po.CALC_DENSE_GAUSSIAN, W, D, dtype, 7, 2)
    _compare(_builtin_sampler(r), r)


@pytest.mark.gpu
@pytest.mark.parametrize("late", ["0", "-1"])
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
def test_late_draw_kernels_with_three_chains_of_walkers_that_overflow(monkeypatch, dtype, late):
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "0")
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS", "0")
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS", "1")
    monkeypatch.setenv("MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS", late)
    W, D, K = 1024 + 38, 32, 3
    runs = [builtin_overflow_run(po.CALC_DENSE_GAUSSIAN, W, D, dtype, 5, 2, seed=11 + k, salt=20 + k) for k in range(K)]
    s = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, runs[0].params, seed=11, dtype=dtype, num_chains=K)
    s.set_state(np.stack([r.pos for r in runs]), np.stack([r.lp for r in runs]))
    hc, ha = s.run(5, interval=2)
    pos, lp, nacc = s.get_state()
    for k, r in enumerate(runs):
        np.testing.assert_array_equal(ha[k], r.acc, err_msg="chain %d" % k)
        np.testing.assert_array_equal(hc[k], r.chain, err_msg="chain %d" % k)
        for a, b, what in zip((pos[k], lp[k], nacc[k]), r.state, ("positions", "logp", "n_accept")):
            np.testing.assert_array_equal(a, b, err_msg="chain %d %s" % (k, what))
    assert s.counters()["near_ties"] == 0


@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
def test_differential_evolution_overflow_run_meets_its_input_conditions(dtype):
    builtin_overflow_run(po.CALC_DENSE_GAUSSIAN, 1030, 32 if dtype == po.F64 else 26, dtype, 20, 1, mover=po.MOVER_DIFFERENTIAL_EVOLUTION)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
def test_differential_evolution_on_the_matrix_cores_with_walkers_that_overflow(dtype):
    r = builtin_overflow_run(po.CALC_DENSE_GAUSSIAN, 1030, 32 if dtype == po.F64 else 26, dtype, 20, 1, mover=po.MOVER_DIFFERENTIAL_EVOLUTION)
    _compare(_builtin_sampler(r), r)
