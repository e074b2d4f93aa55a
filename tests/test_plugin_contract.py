"""The plug-in calculator contract (mcmcpp_amd/csrc/mcmcpp_hip_plugin.hpp) at every lane mapping of every kernel family.

tests/cpp/plugin_contract.hip is one functor the library does not ship, built as a plug-in, that uses every facility the
header names: the wave-private stage (kNeedsStage, g.publish, g.element -- one read in the neighbouring lane, one anywhere in
the group), a block-shared table in LDS (block_scratch_elems = 2 D, block_commit, g.block_scratch), registers of its own (Regs,
preload) and the parameter block, which for a handle of several chains is the chain's own.  Its target, "coupled table", is a
Gaussian with nearest-neighbour and mirror coupling, params = {mu[D], w[D], c[D], r}; with d_j = x_j - mu_j and every operation
rounded on its own,

    a_j = w_j (d_j d_j),  b_j = c_j (d_j d_{j+1}) for j + 1 < D,  m_j = r (d_j d_{D-1-j}),
    t_j = (a_j + b_j) + m_j  (a_j + m_j at j = D - 1),  logp = -1/2 tree_sum(t).

mu and w are read from the table only, c from Regs only, r from the parameter block in eval: a kernel family that hands a hook
the wrong block, skips the table's barrier, lays the table over the stage or indexes the stage wrongly computes another number.
The oracle twin (oracle/stretch_oracle.h: SO_CALC_COUPLED_TABLE) is a plain loop over j that knows nothing of lanes.

CPU: the twin against np.longdouble under a bar derived from the operation count; the oracle alone over the whole case matrix
(no near tie, no redraw for the stretch move, proposals accepted and rejected in each run), so that bit-equality is the right
bar; the plug-in cross-compiles, and its kernels carry no static LDS and no scratch but where listed; the largest table fits
kMaxBlockScratchBytes.

GPU: the case matrix of tests/test_lane_mappings.py with this one calculator, bit for bit against the twin, no tolerance."""
import collections
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po
from tests import replica_restatement as rr
from tests import test_kernel_metadata as km
from tests.test_lane_mappings import (DE, DTYPE_NAME, EDGE_PATHS, RUNS, SALT, SEED, SLOT_TABLE, STEP_PATHS, STRETCH, Case, OracleRun,
                                      assert_input_conditions, compare_with_oracle, hi_minus_1, set_knobs, slot_dims, walkers_for)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "plugin_contract.hip")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libplugin_contract.so")
COUPLED_TABLE = 1003  # the plug-in's calculator id (1000..1002 are taken by tests/test_plugin.py and tests/test_nonfinite.py)
TWIN = po.CALC_COUPLED_TABLE
MOVER_NAME = {STRETCH: "stretch", DE: "de"}


def params_of(D, dtype, k=0):
    """Chain k's block {mu[D], w[D], c[D], r}, rounded to the element type.  The form stays positive definite:
    |off-diagonal row sum| <= 0.2 + 0.0625 < 0.5 <= w_j."""
    rng = np.random.default_rng((D, k))
    mu = rng.uniform(-0.5, 0.5, D)
    w = rng.uniform(0.5, 2.0, D)
    c = rng.uniform(-0.2, 0.2, D)
    return np.concatenate([mu, w, c, [0.0625]]).astype(po.np_dtype(dtype))


# ---- the case matrix: that of tests/test_lane_mappings.py with one calculator ---------------------------------------------------

def _cases(mover):
    return [Case(mover, TWIN, dtype, D, lpw, epl, lo, hi, walkers_for(D, lpw), RUNS)
            for dtype in (po.F64, po.F32) for lpw, epl, lo, hi in SLOT_TABLE[dtype] for D in slot_dims(dtype, lo, hi)]


STRETCH_CASES, DE_CASES = _cases(STRETCH), _cases(DE)
EDGE_CASES = hi_minus_1(STRETCH_CASES)
MATRIX_DIMS = sorted({c.D for c in STRETCH_CASES})

# The seed column of the case table: SEED but for the cases listed here by (mover, dtype, D), each with the input condition the
# default seed missed (test_oracle_runs_meet_their_input_conditions).  Chain k of a handle is seeded with the case's seed + k.
SEEDS = {
    # fp32, wide walkers: with SEED the oracle counts near ties in its seven steps (the fp32 band is 6e-7 of magnitudes that grow
    # with D); each seed below is the first after SEED without one (the number of seeds passed over: every one of them missed
    # "no near tie" and nothing else)
    (STRETCH, po.F32, 1023): 12346,
    (DE, po.F32, 129): 12346,
    (DE, po.F32, 254): 12346,
    (DE, po.F32, 510): 12347,
    (DE, po.F32, 511): 12348,
    (DE, po.F32, 512): 12346,
    (DE, po.F32, 1022): 12355,  # (ten seeds with one to six near ties each)
    (DE, po.F32, 1023): 12346,
    (DE, po.F32, 1024): 12347,
}


def case_id(c):
    return "%s-lpw%dx%d-D%d" % (DTYPE_NAME[c.dtype], c.lpw, c.epl, c.D)


def test_case_matrix_is_the_lane_mapping_matrix():
    for cases in (STRETCH_CASES, DE_CASES):
        for dtype, slots in SLOT_TABLE.items():
            for lpw, epl, lo, hi in slots:
                have = [c.D for c in cases if (c.dtype, c.lpw, c.epl) == (dtype, lpw, epl)]
                assert have == slot_dims(dtype, lo, hi) and len(have) >= 2
        assert {c.runs for c in cases} == {((3, 2), (1, 1))}
    assert [(c.dtype, c.lpw, c.epl) for c in EDGE_CASES] == [(dtype, lpw, epl) for dtype in (po.F64, po.F32) for lpw, epl, _, _ in SLOT_TABLE[dtype]]
    assert all(c.D == c.hi - 1 for c in EDGE_CASES)
    assert max(c.W for c in STRETCH_CASES) == 2050 and MATRIX_DIMS[0] == 1 and MATRIX_DIMS[-1] == 1024


# ---- CPU 1: the oracle twin against a high-precision reference --------------------------------------------------------------------

def reference(params, x):
    """(log-posterior, 1/2 sum_j |a_j| + |b_j| + |m_j|) of the rows of x, every operation in np.longdouble."""
    L = np.longdouble
    D = x.shape[1]
    p = params.astype(L)
    mu, w, c, r = p[:D], p[D:2 * D], p[2 * D:3 * D], p[3 * D]
    d = x.astype(L) - mu
    a = w * (d * d)
    b = np.zeros_like(a)
    b[:, :D - 1] = c[:D - 1] * (d[:, :D - 1] * d[:, 1:])
    m = r * (d * d[:, ::-1])
    return L(-0.5) * (a + b + m).sum(axis=1), L(0.5) * (np.abs(a) + np.abs(b) + np.abs(m)).sum(axis=1)


def test_oracle_twin_against_the_long_double_reference():
    """|oracle - reference| <= (8 + ceil(log2 D)) u 1/2 sum_j (|a_j| + |b_j| + |m_j|), u = 2^-53 or 2^-24, on 40 rows of
    1.5 N(0, 1) for every D of the GPU matrix in both element types.  To first order a term carries at most 6 roundings (d_j,
    d_j d_j, w_j ., the two sums, and one of d_{j+1} / d_{D-1-j} entering a product) and the tree adds its depth; the remaining 2
    is slack for second order.  The bar is not a measured number.  Largest |error| / bar met: 0.359 in fp64 and 0.341 in fp32,
    both at D = 1 (printed by the test)."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than fp64 here: it would not be a reference"
    worst = {}
    for dtype, u in ((po.F64, 2.0 ** -53), (po.F32, 2.0 ** -24)):
        t = po.np_dtype(dtype)
        worst[dtype] = (0.0, None)
        for D in MATRIX_DIMS:
            params = params_of(D, dtype)
            x = (np.random.default_rng(D * 7 + TWIN).standard_normal((40, D)) * 1.5).astype(t)
            got = po.Oracle(walkers_for(D, 1), D, TWIN, params, dtype=dtype).logp(x)
            want, scale = reference(params, x)
            bar = (8 + math.ceil(math.log2(D))) * u * scale
            err = np.abs(got.astype(np.longdouble) - want)
            ratio = float((err / bar).max())
            if ratio > worst[dtype][0]:
                worst[dtype] = (ratio, D)
            assert (err <= bar).all(), (DTYPE_NAME[dtype], D, ratio)
    for dtype, (ratio, D) in worst.items():
        print("oracle twin vs long double, %s: largest |error| / bar = %.3f at D = %d" % (DTYPE_NAME[dtype], ratio, D))
        assert 0.0 < ratio  # (a twin that returned the reference's own bits would not be a restatement in the element type)


def test_oracle_twin_checks_its_parameter_count():
    D = 5
    p = params_of(D, po.F64)
    po.Oracle(12, D, TWIN, p)
    for bad in (p[:-1], np.concatenate([p, [0.0]]), None):
        with pytest.raises(ValueError):
            po.Oracle(12, D, TWIN, bad)


# ---- the oracle's side of every case, computed once -------------------------------------------------------------------------------

_ORACLE_RUNS = collections.OrderedDict()
_ORACLE_CACHE_BYTES = 1 << 30  # the least recently used results beyond this are computed again when asked for


def oracle_run(c, chain=0, params_chain=None):
    """What the twin makes of case c: chain k of a handle of several chains has seed + k, a start of its own and the block
    params_of(D, dtype, params_chain), which is chain k's own unless stated otherwise."""
    params_chain = chain if params_chain is None else params_chain
    key = (c.mover, c.dtype, c.D, chain, params_chain)
    if key in _ORACLE_RUNS:
        _ORACLE_RUNS.move_to_end(key)
        return _ORACLE_RUNS[key]
    seed = SEEDS.get(key[:3], SEED) + chain
    params = params_of(c.D, c.dtype, params_chain)
    orc = po.Oracle(c.W, c.D, TWIN, params, seed=seed, dtype=c.dtype, mover=c.mover)
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
                  sum(a.nbytes for a in chains) + 2 * pos.nbytes + params.nbytes)
    for a in [pos, logp, params] + chains + accepted + list(r.state):
        a.setflags(write=False)
    _ORACLE_RUNS[key] = r
    total = sum(v.nbytes for v in _ORACLE_RUNS.values())
    while total > _ORACLE_CACHE_BYTES and len(_ORACLE_RUNS) > 1:
        total -= _ORACLE_RUNS.popitem(last=False)[1].nbytes
    return r


# ---- CPU 2: input conditions ------------------------------------------------------------------------------------------------------

CONDITION_CASES = [(c, 0) for c in STRETCH_CASES] + [(c, 1) for c in EDGE_CASES] + [(c, 0) for c in DE_CASES]


@pytest.mark.parametrize("c,chain", CONDITION_CASES, ids=["%s-%s-chain%d" % (MOVER_NAME[c.mover], case_id(c), k) for c, k in CONDITION_CASES])
def test_oracle_runs_meet_their_input_conditions(c, chain):
    """No near tie, no redraw for the stretch move, and in every run some proposals accepted and some rejected."""
    assert_input_conditions(c, oracle_run(c, chain))


@pytest.mark.parametrize("c", EDGE_CASES, ids=case_id)
def test_each_chains_block_decides_its_chain(c):
    """The two blocks of a two-chain case differ, and a chain stepped under the other chain's block is another chain: a hook
    that read chain 0's block for chain 1 (or the reverse) could not pass the two-chain cases."""
    p0, p1 = params_of(c.D, c.dtype, 0), params_of(c.D, c.dtype, 1)
    D = c.D
    for part in (slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D)):  # mu (table), w (table), c (Regs)
        assert not np.array_equal(p0[part], p1[part])
    for chain in (0, 1):
        own, other = oracle_run(c, chain), oracle_run(c, chain, params_chain=1 - chain)
        assert own.seed == other.seed and np.array_equal(own.pos, other.pos)
        assert not np.array_equal(own.logp, other.logp)
        assert not np.array_equal(own.chains[0], other.chains[0]) and not np.array_equal(own.state[0], other.state[0])


# ---- CPU 3: the plug-in builds, and what the compiler made of it ------------------------------------------------------------------

def build_plugin():
    """tests/cpp/plugin_contract.hip -> its shared library (hipcc cross-compiles without a GPU), with the flags of tests/test_plugin.py
    (it needs the library's headers only; the library itself, which build() makes, is asked for at registration)"""
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc")))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(newest, os.path.getmtime(SRC)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                               "-fPIC", "-shared", "-mllvm", "-amdgpu-kernarg-preload-count=16", "-I" + CSRC, SRC, "-o", OUT])
    return OUT


@pytest.fixture(scope="module")
def plugin():
    lib = C.CDLL(build_plugin())
    tables = []
    for t in ("f64", "f32"):
        f = getattr(lib, "mcmcpp_hip_plugin_coupled_table_%s" % t)
        f.restype = C.c_void_p
        tables.append(f())
        assert tables[-1]
    L = capi.lib()
    L.mcmcpp_hip_register_calculator.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    assert L.mcmcpp_hip_register_calculator(COUPLED_TABLE, tables[0], tables[1], -1) == 0
    return L


def test_plugin_builds_and_registers(plugin):
    """CPU: the functor compiles against the plug-in header outside the library's own translation units and its launch
    tables register under an id of the user's."""
    assert os.path.exists(OUT)


# The instantiations with scratch memory, as data: one family, the plain full-step kernel of fp64 walkers of 513..1024
# dimensions (64 lanes x 16 elements; three proposals of 16 registers each beside Regs), 108 bytes of spills with and without
# several chains per launch -- the slot where the dense built-in has its tests/test_kernel_metadata.py KNOWN_SCRATCH entry.
KNOWN_SCRATCH = {"stretch_full_step_kernel<double, CoupledTable<double>, 16, 64"}
KERNELS_PER_SLOT = 8  # half step (with / without the draw wavefront, one / several chains), full step (one / several chains), calc, de


def test_plugin_kernels_carry_no_static_lds_and_no_scratch(tmp_path, monkeypatch):
    """The metadata reader of tests/test_kernel_metadata.py (the notes of the code object only) on the plug-in's library."""
    out = build_plugin()
    with monkeypatch.context() as m:
        m.setattr(km.capi, "build_library", lambda: out)  # (the reader asks this for the library whose code objects it reads)
        kernels = km._kernels_of_library(tmp_path)
    step = [k for k in kernels if re.match(r"(void )?(mcmcpp::)?(stretch_(half|full)_step|de_update|calc_logp)", k["name"]) and "CoupledTable<" in k["name"]]
    assert len(step) == KERNELS_PER_SLOT * sum(len(s) for s in SLOT_TABLE.values()) == 152, len(step)
    assert not [k["name"] for k in step if "mfma" in k["name"]]  # (MatrixCore::kUse is false in every slot)
    assert [(k["name"][:110], k["lds"]) for k in step if k["lds"] != 0] == []
    with_scratch = {}
    for k in step:
        if k["scratch"] != 0:
            family = re.sub(r", (true|false)>.*$", "", k["name"].split("(")[0])
            with_scratch.setdefault(family, []).append(k["scratch"])
    print("scratch in the plug-in's step kernels (bytes per instantiation):", with_scratch)
    assert set(with_scratch) == KNOWN_SCRATCH


# ---- CPU 4: the LDS claim ---------------------------------------------------------------------------------------------------------

def test_largest_table_fits_the_block_scratch_cap():
    """block_scratch_elems(1024) = 2048 fp64 elements against kMaxBlockScratchBytes, the author's obligation (nothing enforces it)."""
    text = open(os.path.join(CSRC, "calculators.hpp")).read()
    m = re.search(r"constexpr size_t kMaxBlockScratchBytes = (\d+) \* 1024;", text)
    assert m, "kMaxBlockScratchBytes not found in calculators.hpp"
    assert 2 * 1024 * 8 <= int(m.group(1)) * 1024
    assert "block_scratch_elems(int D) { return 2 * (size_t)D; }" in open(SRC).read()


# ---- the exchange case, restated on the CPU ---------------------------------------------------------------------------------------

EX_K, EX_D, EX_SEED, EX_ROUNDS, EX_STEPS = 3, 33, 43, 4, 3
EX_W = walkers_for(EX_D, 32)
EX_BETAS = (1.0, 0.5, 0.25)


def exchange_ladder():
    """Rows {mu, beta w, beta c, beta r}: chain 0's target flattened by beta (exact scalings: powers of two)."""
    base = params_of(EX_D, po.F64)
    rows = []
    for beta in EX_BETAS:
        row = base.copy()
        row[EX_D:] *= beta
        rows.append(row)
    return rows


def restated_exchange():
    params = exchange_ladder()
    lad = rr.Ladder(EX_W, EX_D, TWIN, params, EX_SEED)
    pos = np.stack([po.init_positions(po.F64, EX_W, EX_D, salt=90 + k) for k in range(EX_K)])
    logp = np.stack([lad.logp(k, pos[k]) for k in range(EX_K)])
    lad.set_state(pos, logp)
    return lad, pos, logp, params


def assert_exchange_conditions(want, rnd):
    """On the restatement's own counts: no decision inside the near-tie band, and every pair of the round both accepts and
    rejects swaps."""
    assert not want["in_band"] and not want["near_ties"].any(), (rnd, want["in_band"])
    for a, _ in rr.pairs_of(EX_K, rnd):
        assert want["proposed"][a] == EX_W and 0 < want["accepted"][a] < EX_W, (rnd, a, want["accepted"][a])


def test_exchange_case_meets_its_input_conditions():
    assert EX_W == 70 and [len(rr.pairs_of(EX_K, r)) for r in range(EX_ROUNDS)] == [1, 1, 1, 1]
    rows = exchange_ladder()
    assert all(np.array_equal(rows[k][:EX_D], rows[0][:EX_D]) and np.array_equal(rows[k][EX_D:], EX_BETAS[k] * rows[0][EX_D:]) for k in range(EX_K))
    lad = restated_exchange()[0]
    for r in range(EX_ROUNDS):
        _, acc = lad.run(EX_STEPS)
        assert (acc > 0).all() and (acc < EX_W).all()
        assert_exchange_conditions(lad.exchange(r), r)
    assert all(o.near_ties == 0 and o.redraws == 0 for o in lad.orcs)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

gpu = pytest.mark.gpu


def step_and_compare(monkeypatch, c, knobs, chains=1):
    runs = [oracle_run(c, k) for k in range(chains)]
    for r in runs:
        assert_input_conditions(c, r)
    set_knobs(monkeypatch, knobs)
    if chains == 1:
        hip = capi.HipSampler(c.W, c.D, COUPLED_TABLE, runs[0].params, seed=runs[0].seed, dtype=c.dtype, mover=c.mover)
        hip.set_state(runs[0].pos, runs[0].logp)
    else:
        assert [r.seed for r in runs] == [runs[0].seed + k for k in range(chains)]  # (what the library seeds chain k with)
        assert not any(np.array_equal(runs[0].params, r.params) for r in runs[1:])
        # (the stacked params of num_chains: row 0 goes to create, rows 1.. to set_chain_params)
        hip = capi.HipSampler(c.W, c.D, COUPLED_TABLE, np.stack([r.params for r in runs]), seed=runs[0].seed, dtype=c.dtype, mover=c.mover, num_chains=chains)
        hip.set_state(np.stack([r.pos for r in runs]), np.stack([r.logp for r in runs]))
    compare_with_oracle(hip, c, runs)


def _with_paths(cases, paths):
    return [pytest.param(c, path, id="%s-%s" % (case_id(c), path)) for c in cases for path in paths]


@gpu
@pytest.mark.parametrize("c,path", _with_paths(STRETCH_CASES, STEP_PATHS))
def test_stretch_step_kernels(monkeypatch, plugin, c, path):
    """The slot's full-step and half-step kernels around the plug-in functor.  From D = 129 on these are the first launches in
    which a block table meets the 64-lane slots' barriers and a stage of 8, 16 or 32 KiB lies in front of it."""
    knobs, chains = STEP_PATHS[path]
    step_and_compare(monkeypatch, c, knobs, chains)


@gpu
@pytest.mark.parametrize("c,path", _with_paths(EDGE_CASES, EDGE_PATHS))
def test_stretch_step_kernel_variants_with_a_partly_filled_last_lane(monkeypatch, plugin, c, path):
    """The other instantiations of a slot, at D = hi - 1: without the draw wavefront, four passes, and two chains per launch --
    chain k with a block of its own against a twin with chain k's block and seed + k
    (test_each_chains_block_decides_its_chain: under the other chain's block it would be another chain)."""
    knobs, chains = EDGE_PATHS[path]
    step_and_compare(monkeypatch, c, knobs, chains)


@gpu
@pytest.mark.parametrize("c", DE_CASES, ids=case_id)
def test_differential_evolution_update_kernels(monkeypatch, plugin, c):
    """de_update_kernel of every slot; redraws are expected here and must be the oracle's."""
    step_and_compare(monkeypatch, c, {})


@gpu
@pytest.mark.parametrize("c", STRETCH_CASES, ids=case_id)
def test_calc_logp_kernels(plugin, c):
    """calc_logp_kernel of every slot on 301 rows: a handle of one chain, and chain 1 of a handle of two, whose block comes
    through set_chain_params, against chain 1's twin."""
    t = po.np_dtype(c.dtype)
    p0, p1 = params_of(c.D, c.dtype, 0), params_of(c.D, c.dtype, 1)
    pos = (np.random.default_rng(c.D * 7 + TWIN).standard_normal((301, c.D)) * 1.5).astype(t)
    want0 = po.Oracle(c.W, c.D, TWIN, p0, dtype=c.dtype).logp(pos)
    want1 = po.Oracle(c.W, c.D, TWIN, p1, dtype=c.dtype).logp(pos)
    assert not np.array_equal(want0, want1)
    np.testing.assert_array_equal(capi.HipSampler(c.W, c.D, COUPLED_TABLE, p0, dtype=c.dtype).calc_logp(pos), want0)
    two = capi.HipSampler(c.W, c.D, COUPLED_TABLE, p0, dtype=c.dtype, num_chains=2)
    two.set_chain_params(1, p1)
    np.testing.assert_array_equal(two.calc_logp(pos, chain=1), want1)
    np.testing.assert_array_equal(two.calc_logp(pos, chain=0), want0)
    np.testing.assert_array_equal(two.calc_logp(pos), want0)


@gpu
def test_exchange_rounds_equal_the_restatement(monkeypatch, plugin):
    """K = 3 chains of 70 walkers x 33 dims on the ladder {mu, beta w, beta c, beta r}, beta = 1, 1/2, 1/4: four times run(3) and
    exchange_chains(r), every array and counter against tests/replica_restatement.py, as tests/test_replica_exchange.py does
    for the built-ins.  The exchange is the only path that evaluates a chain's rows under its neighbour's block."""
    set_knobs(monkeypatch, {})
    lad, pos, logp, params = restated_exchange()
    hip = capi.HipSampler(EX_W, EX_D, COUPLED_TABLE, np.stack(params), seed=EX_SEED, num_chains=EX_K)
    for k in range(EX_K):
        np.testing.assert_array_equal(hip.calc_logp(pos[k], chain=k), logp[k], err_msg="chain %d" % k)
    hip.set_state(pos, logp)

    def same_state(what):
        for got, want, name in zip(hip.get_state(), lad.get_state(), ("positions", "log-posteriors", "n_accept")):
            np.testing.assert_array_equal(got, want, err_msg="%s: %s" % (what, name))

    for r in range(EX_ROUNDS):
        hc, ha = hip.run(EX_STEPS)
        oc, oa = lad.run(EX_STEPS)
        np.testing.assert_array_equal(hc, oc, err_msg="run before round %d" % r)
        np.testing.assert_array_equal(ha, oa, err_msg="run before round %d" % r)
        want = lad.exchange(r)
        got = hip.exchange_chains(r)
        assert_exchange_conditions(want, r)
        assert not got["near_ties"].any()
        np.testing.assert_array_equal(got["proposed"], want["proposed"])
        np.testing.assert_array_equal(got["accepted"], want["accepted"])
        same_state("after round %d" % r)
    hc, ha = hip.run(2)
    oc, oa = lad.run(2)
    np.testing.assert_array_equal(hc, oc, err_msg="final run")
    np.testing.assert_array_equal(ha, oa, err_msg="final run")
    counters = hip.counters()
    assert counters["redraws"] == 0 and counters["near_ties"] == 0
