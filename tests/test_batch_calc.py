"""Batch targets (calc_id MCMCPP_HIP_CALC_BATCH): the proposals of a half-step are formed on the device, evaluated in one
batch by a host callback, and accepted.  A callback that computes a built-in Calculator's bits must reproduce that
Calculator's chains bit for bit -- the reference's fixtures, the oracle, and the fused path."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po
from tests.goldens import GOLDEN_DIR, Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
HIPCC = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"]
KIND = {po.CALC_ISO_GAUSSIAN: 0, po.CALC_DENSE_GAUSSIAN: 1, po.CALC_ROSENBROCK: 2, po.CALC_SKEWED_GAUSSIAN_2D: 3}


def _noop(user, proposals, logp_out, count, num_params, hip_stream):
    return 0


NOOP = capi.BATCH_LOGP_FN(_noop)


# ---- CPU: interface and refusals ------------------------------------------------------------------------

def test_header_declares_the_batch_interface(tmp_path):
    header = open(os.path.join(ROOT, "include", "mcmcpp_hip.h")).read()
    assert re.search(r"\bint mcmcpp_hip_set_batch_calculator\s*\(", header)
    assert re.search(r"MCMCPP_HIP_CALC_BATCH\s*=\s*4\b", header)
    assert re.search(r"MCMCPP_HIP_E_CALLBACK\s*=\s*8\b", header)
    assert "mcmcpp_hip_set_batch_calculator" in capi.EXPORTS
    src = tmp_path / "use.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'static int cb(void* u, const void* p, void* l, int64_t n, int32_t d, void* s)\n'
                   '{ (void)u; (void)p; (void)l; (void)n; (void)d; (void)s; return 0; }\n'
                   'int use(mcmcpp_hip_sampler* h) { mcmcpp_hip_batch_logp_fn f = cb;\n'
                   '  return mcmcpp_hip_set_batch_calculator(h, f, 0, 0, 0) + MCMCPP_HIP_CALC_BATCH + MCMCPP_HIP_E_CALLBACK; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "use.o")])


@pytest.mark.parametrize("kw,msg", [
    (dict(mover=capi.MOVER_DIFFERENTIAL_EVOLUTION), "StretchMove only"),
    (dict(num_chains=2), "one ensemble per handle"),
    (dict(shard_count=16), "no shards"),
    (dict(shard_begin=4, shard_count=8), "no shards"),
    (dict(comm_world=1, comm_id=b"\0" * 128), "no communicator"),
    (dict(params=[1.0]), "takes no parameters"),
])
def test_create_refuses_unsupported_batch_configurations(kw, msg):
    capi.build_library()
    with pytest.raises(capi.HipError) as e:
        capi.HipSampler(64, 4, capi.CALC_BATCH, batch_callback=(NOOP, None), **kw)
    assert e.value.code == 1 and msg in str(e.value)


def test_wrapper_pairs_log_prob_with_the_batch_calc_id():
    with pytest.raises(ValueError):
        capi.HipSampler(64, 4, capi.CALC_ISO_GAUSSIAN, log_prob=lambda x: x.sum(1))
    with pytest.raises(ValueError):
        capi.HipSampler(64, 4, capi.CALC_ISO_GAUSSIAN, batch_callback=(NOOP, None))
    with pytest.raises(ValueError):
        capi.HipSampler(64, 4, capi.CALC_BATCH)
    with pytest.raises(ValueError):
        capi.HipSampler(64, 4, capi.CALC_BATCH, log_prob=lambda x: x.sum(1), batch_callback=(NOOP, None))


def test_existing_calc_id_rules_hold():
    capi.build_library()
    for bad in (9, 1234):
        with pytest.raises(capi.HipError) as e:
            capi.HipSampler(64, 4, bad)
        assert "unknown calc_id" in str(e.value)
    assert capi.lib().mcmcpp_hip_register_calculator(capi.CALC_BATCH, None, None, 0) == 1


def _build_facade_example():
    """examples/batch_calculator_device.hip -> libbatch_calculator.so (hipcc), examples/batch_calculator.cpp -> the program (g++)."""
    capi.build_library()
    os.makedirs(BUILD, exist_ok=True)
    dev_so = os.path.join(BUILD, "libbatch_calculator.so")
    exe = os.path.join(BUILD, "batch_calculator")
    subprocess.check_call(HIPCC + [os.path.join(ROOT, "examples", "batch_calculator_device.hip"), "-o", dev_so])
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include", "MCMCpp"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "batch_calculator.cpp"), "-o", exe,
                           "-L" + BUILD, "-lbatch_calculator", "-Wl,-rpath," + BUILD, "-L" + os.path.join(ROOT, "mcmcpp_amd"),
                           "-lmcmcpp_hip", "-Wl,-rpath," + os.path.join(ROOT, "mcmcpp_amd")])
    return exe


def test_facade_batch_example_compiles_and_links():
    assert os.path.exists(_build_facade_example())


# ---- GPU ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cb_lib():
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "batch_calc.hip")
    out = os.path.join(BUILD, "libbatch_calc.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.check_call(HIPCC + [src, "-o", out])
    L = C.CDLL(out)
    L.batch_calc_create.restype = C.c_void_p
    L.batch_calc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.batch_calc_destroy.argtypes = [C.c_void_p]
    L.batch_calc_fail_at.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    L.batch_calc_calls.argtypes = [C.c_void_p]
    L.batch_calc_calls.restype = C.c_int64
    return L


class CTarget:
    """A restated built-in Calculator in tests/cpp/batch_calc.hip, as (function pointer, user pointer)."""

    def __init__(self, L, calc, D, params, dtype):
        self.L = L
        p = None if params is None else np.ascontiguousarray(params, dtype=po.np_dtype(dtype))
        self.user = L.batch_calc_create(KIND[calc], dtype, D, None if p is None else p.ctypes.data, 0 if p is None else p.size)
        assert self.user
        self.fn = C.cast(L.batch_calc_logp, C.c_void_p).value

    def callback(self):
        return (self.fn, self.user)

    def fail_at(self, call, code):
        self.L.batch_calc_fail_at(self.user, call, code)

    def __del__(self):
        if getattr(self, "user", None):
            self.L.batch_calc_destroy(self.user)


def _params_for(calc, D, t, rng):
    if calc == po.CALC_DENSE_GAUSSIAN:
        a = rng.standard_normal((D, D))
        return (a @ a.T / D + np.eye(D)).astype(t).ravel()
    if calc == po.CALC_ROSENBROCK:
        return np.array([1.0, 100.0, 0.05], dtype=t)
    if calc == po.CALC_SKEWED_GAUSSIAN_2D:
        return np.array([0.13], dtype=t)
    return None


def _batch_sampler(L, W, D, calc, params, dtype=po.F64, **kw):
    tgt = CTarget(L, calc, D, params, dtype)
    s = capi.HipSampler(W, D, capi.CALC_BATCH, dtype=dtype, batch_callback=tgt.callback(), **kw)
    s._target = tgt  # (the callback's context lives as long as the handle)
    return s


def _run_against_golden(s, g):
    s.set_state(g.init_pos, g.init_logp)
    done, acc_calls = 0, []
    for k in sorted(set(g.checked_steps + [g.steps])):
        chain, acc = s.run(k - done, interval=g.slicing)
        acc_calls.append(acc.reshape(k - done, g.slicing).sum(axis=1))
        done = k
        if k in g.checked_steps:
            g.check_chain_step(k, chain[-1])
    np.testing.assert_array_equal(np.concatenate(acc_calls), g.accepted_per_call)
    c = s.counters()
    assert c["accepted"] + g.W == g.accepted_total
    assert g.W * (1 + c["ensemble_steps"]) == g.total_steps
    assert c["near_ties"] == 0 and c["redraws"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iso64x4", "iso64x4_f32", "iso100x7", "dense96x16", "dense80x5_f32", "rosen80x8", "skewed320x2"])
def test_c_callback_reproduces_reference_golden(cb_lib, name):
    g = Golden(name)
    s = _batch_sampler(cb_lib, g.W, g.D, g.calc, g.params, dtype=g.dtype, seed=g.seed, alpha=g.alpha)
    _run_against_golden(s, g)


def _oracle_pair(L, W, D, calc, dtype, seed, salt=3, **kw):
    t = po.np_dtype(dtype)
    params = _params_for(calc, D, t, np.random.default_rng(W + D))
    orc = po.Oracle(W, D, calc, params, seed=seed, dtype=dtype)
    pos = po.init_positions(dtype, W, D, salt=salt)
    logp = orc.logp(pos)
    orc.set_state(pos, logp)
    s = _batch_sampler(L, W, D, calc, params, dtype=dtype, seed=seed, **kw)
    s.set_state(pos, logp)
    return orc, s, pos, logp, params


def _assert_same_state(orc, s):
    for a, b, what in zip(s.get_state(), orc.get_state(), ("positions", "logp", "n_accept")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    c = s.counters()
    assert c["near_ties"] == 0 == orc.near_ties and c["redraws"] == orc.redraws == 0


@pytest.mark.gpu
@pytest.mark.parametrize("W,D,calc,dtype,steps,interval", [
    (6, 2, po.CALC_ISO_GAUSSIAN, po.F64, 500, 1),        # n = 3: non power of two partner bound
    (4, 1, po.CALC_ISO_GAUSSIAN, po.F32, 500, 3),        # D = 1
    (1026, 512, po.CALC_ISO_GAUSSIAN, po.F64, 12, 1),    # EPL > base (D > 128)
    (4098, 32, po.CALC_ROSENBROCK, po.F32, 30, 1),       # ragged last wavefront
    (300, 64, po.CALC_DENSE_GAUSSIAN, po.F64, 40, 2),
    (1000, 9, po.CALC_ROSENBROCK, po.F64, 60, 4),
])
def test_c_callback_equals_oracle(cb_lib, W, D, calc, dtype, steps, interval):
    orc, s, _, _, _ = _oracle_pair(cb_lib, W, D, calc, dtype, seed=12345)
    oc, oa = orc.run(steps, interval=interval, mode=po.MODE_COUNTER, threads=4)
    hc, ha = s.run(steps, interval=interval)
    np.testing.assert_array_equal(ha, oa)
    np.testing.assert_array_equal(hc, oc)
    _assert_same_state(orc, s)


@pytest.mark.gpu
def test_calc_logp_equals_oracle(cb_lib):
    W, D = 40, 7
    orc, s, _, _, params = _oracle_pair(cb_lib, W, D, po.CALC_DENSE_GAUSSIAN, po.F64, seed=1)
    x = np.random.default_rng(3).standard_normal((W * 3 + 5, D))  # several chunks of W/2 rows
    np.testing.assert_array_equal(s.calc_logp(x), orc.logp(x))


@pytest.mark.gpu
def test_reference_own_skewed_test_through_the_callback(cb_lib):
    """The reference's SkewedGaussian/StretchMove test (320 x 2, slicing 30, 40 019 stored steps: 2.4 M callbacks)."""
    want = json.load(open(os.path.join(GOLDEN_DIR, "reference_skewed_test.json")))
    g = Golden("skewed320x2")
    s = _batch_sampler(cb_lib, g.W, g.D, g.calc, g.params, seed=0)
    s.set_state(g.init_pos, g.init_logp)
    s.run(want["stored_steps"], interval=want["slicing"], save_chain=False, want_accepted=False)
    c = s.counters()
    print("%d / %d" % (c["accepted"] + g.W, g.W * (1 + c["ensemble_steps"])))
    assert c["near_ties"] == 0
    assert c["accepted"] + g.W == want["accepted_total"]
    assert g.W * (1 + c["ensemble_steps"]) == want["total_steps"]


def _fused(W, D, calc, params, dtype, seed, monkeypatch):
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "0")
    return capi.HipSampler(W, D, calc, params, seed=seed, dtype=dtype)


@pytest.mark.gpu
def test_bookkeeping_equals_the_fused_path(cb_lib, monkeypatch):
    W, D, calc, seed = 512, 6, po.CALC_ROSENBROCK, 77
    orc, s, pos, logp, params = _oracle_pair(cb_lib, W, D, calc, po.F64, seed)
    f = _fused(W, D, calc, params, po.F64, seed, monkeypatch)
    f.set_state(pos, logp)
    # split runs with an interval
    for n_saved, interval in ((5, 3), (7, 1), (2, 4)):
        a, b = s.run(n_saved, interval=interval), f.run(n_saved, interval=interval)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    # run_async + wait_stored into pinned memory
    out_s, out_f = capi.pinned_empty((9, W, D)), capi.pinned_empty((9, W, D))
    s.run_async(9, interval=2, out=out_s)
    s.wait_stored(3)
    s.run_wait()
    f.run(9, interval=2, out=out_f)
    np.testing.assert_array_equal(out_s, out_f)
    # counters and reset
    assert s.counters() == f.counters()
    s.reset_counters()
    f.reset_counters()
    s.run(3)
    f.run(3)
    assert s.counters() == f.counters()
    for a, b in zip(s.get_state(), f.get_state()):
        np.testing.assert_array_equal(a, b)
    # checkpoint: get_state + seek into a new handle, resumed
    p, lp, _ = s.get_state()
    steps_done = 5 * 3 + 7 + 2 * 4 + 9 * 2 + 3
    s2 = _batch_sampler(cb_lib, W, D, calc, params, seed=seed)
    s2.set_state(p, lp)
    s2.seek(steps_done)
    a, b = s2.run(6, interval=2), f.run(6, interval=2)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    # calc_logp equals the oracle's logp
    x = np.random.default_rng(0).standard_normal((W + 3, D))
    np.testing.assert_array_equal(s.calc_logp(x), orc.logp(x))
    with pytest.raises(capi.HipError) as e:
        s.half_step_async(0)
    assert e.value.code == 4


@pytest.mark.gpu
def test_calls_before_the_callback_is_set_are_refused():
    h = C.c_void_p()
    cfg = capi.Config(C.sizeof(capi.Config), 0, 64, 4, capi.CALC_BATCH, 0, None, 0, 0, -1, 0, 0, 0, 0, 0, None, None, 0, 0, 0, 0,
                      None, None, 0, 0)
    L = capi.lib()
    assert L.mcmcpp_hip_create(C.byref(cfg), C.byref(h)) == 0
    try:
        pos, lp = np.zeros((64, 4)), np.zeros(64)
        assert L.mcmcpp_hip_set_state(h, pos.ctypes.data, lp.ctypes.data) == 5
        assert L.mcmcpp_hip_run(h, 1, 1, None, None) == 5
        assert L.mcmcpp_hip_calc_logp(h, pos.ctypes.data, 4, lp.ctypes.data) == 5
    finally:
        L.mcmcpp_hip_destroy(h)


@pytest.mark.gpu
def test_failing_callback_ends_the_run(cb_lib, monkeypatch):
    W, D, calc, seed = 128, 5, po.CALC_ISO_GAUSSIAN, 9
    orc, s, pos, logp, params = _oracle_pair(cb_lib, W, D, calc, po.F64, seed)
    s._target.fail_at(7, 42)
    with pytest.raises(capi.HipError) as e:
        s.run(10)
    assert e.value.code == capi.E_CALLBACK and "returned 42" in str(e.value)
    with pytest.raises(capi.HipError) as e:
        s.run(1)
    assert e.value.code == 5
    s.set_state(pos, logp)
    f = _fused(W, D, calc, params, po.F64, seed, monkeypatch)
    f.set_state(pos, logp)
    a, b = s.run(10), f.run(10)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


# ---- torch targets ----------------------------------------------------------------------------------------

def _torch():
    import torch
    return torch


def _torch_iso(x):
    """IsoGaussian's host twin in torch: squares, +0 padding to a power of two, pairwise halving, * -1/2."""
    torch = _torch()
    v = x * x
    p2 = 1
    while p2 < v.shape[1]:
        p2 *= 2
    if p2 > v.shape[1]:
        v = torch.cat([v, torch.zeros((v.shape[0], p2 - v.shape[1]), dtype=v.dtype, device=v.device)], dim=1)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0] * -0.5


def _torch_skewed(eps):
    """SkewedGaussian2D's host twin in torch, one op at a time, dividing by a device tensor (not a Python scalar)."""
    def fn(x):
        half = x[:, 0] / 2.0
        lo = half - x[:, 1]
        hi = half + x[:, 1]
        a = (lo * lo) / eps
        b = hi * hi
        return (a + b) / -2.0
    return fn


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iso64x4", "skewed320x2"])
def test_torch_target_reproduces_reference_golden(name):
    torch = _torch()
    g = Golden(name)
    if g.calc == po.CALC_ISO_GAUSSIAN:
        fn = _torch_iso
    else:
        fn = _torch_skewed(torch.tensor(float(g.params[0]), dtype=torch.float64, device="cuda"))
    s = capi.HipSampler(g.W, g.D, capi.CALC_BATCH, seed=g.seed, dtype=g.dtype, alpha=g.alpha, log_prob=fn)
    _run_against_golden(s, g)


@pytest.mark.gpu
@pytest.mark.parametrize("calc", [po.CALC_ISO_GAUSSIAN, po.CALC_SKEWED_GAUSSIAN_2D])
def test_torch_target_equals_the_fused_path(calc, monkeypatch):
    torch = _torch()
    W, D = 4096, (8 if calc == po.CALC_ISO_GAUSSIAN else 2)
    params = _params_for(calc, D, np.float64, None)
    fn = _torch_iso if calc == po.CALC_ISO_GAUSSIAN else _torch_skewed(torch.tensor(0.13, dtype=torch.float64, device="cuda"))
    pos = po.init_positions(po.F64, W, D, salt=5)
    logp = po.Oracle(W, D, calc, params).logp(pos)
    s = capi.HipSampler(W, D, capi.CALC_BATCH, seed=11, log_prob=fn)
    np.testing.assert_array_equal(s.calc_logp(pos), logp)
    f = _fused(W, D, calc, params, po.F64, 11, monkeypatch)
    s.set_state(pos, logp)
    f.set_state(pos, logp)
    a, b = s.run(20, interval=2), f.run(20, interval=2)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    # the same through run_async (the callback then runs on the handle's worker thread)
    ca, _ = s.run_async(5)
    s.run_wait()
    cb, _ = f.run(5)
    np.testing.assert_array_equal(ca, cb)
    assert s.counters() == f.counters()


@pytest.mark.gpu
def test_torch_matmul_target_samples_the_right_covariance():
    """A correlated Gaussian written with torch.matmul (no bit parity claimed): the sample covariance must match."""
    torch = _torch()
    D, W = 4, 256
    rho = 0.6
    cov = np.array([[rho ** abs(i - j) for j in range(D)] for i in range(D)])
    prec = torch.tensor(np.linalg.inv(cov), dtype=torch.float64, device="cuda")

    def fn(x):
        return -0.5 * (torch.matmul(x, prec) * x).sum(dim=1)

    s = capi.HipSampler(W, D, capi.CALC_BATCH, seed=3, log_prob=fn)
    pos = np.random.default_rng(1).standard_normal((W, D))
    s.set_state(pos, s.calc_logp(pos))
    chain, _ = s.run(400, interval=5)
    x = chain[100:].reshape(-1, D)
    got = np.cov(x.T)
    assert np.max(np.abs(got - cov)) < 0.08, got
    assert np.max(np.abs(x.mean(axis=0))) < 0.06


@pytest.mark.gpu
def test_torch_exception_becomes_the_cause(monkeypatch):
    torch = _torch()
    calls = {"n": 0}

    def fn(x):
        calls["n"] += 1
        if calls["n"] == 5:
            raise RuntimeError("boom in log_prob")
        return _torch_iso(x)

    W, D = 64, 4
    pos = po.init_positions(po.F64, W, D, salt=2)
    logp = po.Oracle(W, D, po.CALC_ISO_GAUSSIAN, None).logp(pos)
    s = capi.HipSampler(W, D, capi.CALC_BATCH, seed=4, log_prob=fn)
    s.set_state(pos, logp)
    with pytest.raises(capi.HipError) as e:
        s.run(10)
    assert e.value.code == capi.E_CALLBACK
    assert isinstance(e.value.__cause__, RuntimeError) and "boom" in str(e.value.__cause__)
    with pytest.raises(capi.HipError):
        s.run(1)
    s.set_state(pos, logp)
    f = _fused(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64, 4, monkeypatch)
    f.set_state(pos, logp)
    a, b = s.run(6), f.run(6)
    np.testing.assert_array_equal(a[0], b[0])
    # a wrong result shape is an error of the same kind
    s2 = capi.HipSampler(W, D, capi.CALC_BATCH, seed=4, log_prob=lambda x: x)
    s2.set_state(pos, logp)
    with pytest.raises(capi.HipError) as e:
        s2.run(1)
    assert isinstance(e.value.__cause__, TypeError)
    del torch


# ---- C++ facade ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iso64x4", "iso100x7"])
def test_facade_batch_example_equals_builtin_and_golden(name, tmp_path):
    exe = _build_facade_example()
    g = Golden(name)
    init = tmp_path / "init.bin"
    init.write_bytes(np.asarray(g.init_pos, dtype=np.float64).tobytes())
    out_bin = tmp_path / "chain.bin"
    r = subprocess.run([exe, str(g.W), str(g.D), str(g.steps), str(g.slicing), str(g.seed), str(init), str(out_bin)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "identical chains" in r.stdout, r.stdout + r.stderr
    chain = np.fromfile(str(out_bin), dtype=np.float64).reshape(-1, g.W, g.D)
    for k in g.checked_steps:
        g.check_chain_step(k, chain[k])
    assert "accepted %d/%d" % (g.accepted_total, g.total_steps) in r.stdout, r.stdout
