"""Per-chain calculator parameters (mcmcpp_hip_set_chain_params / mcmcpp_hip_calc_logp_chain): the K chains of one handle
stepped by the same launches, each with a parameter block of its own -- one model fitted to K data sets.  Chain k must be,
bit for bit, what a sampler of its own with parameters params_k and seed seed + k computes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E_ARG, E_UNSUPPORTED, E_STATE = 1, 4, 5


def _params(calc, D, k, rng, t=np.float64):
    """chain k's block: a different target for every k"""
    if calc == po.CALC_DENSE_GAUSSIAN:
        a = rng.standard_normal((D, D))
        return (a @ a.T / D + (1.0 + 0.25 * k) * np.eye(D)).astype(t).ravel()
    if calc == po.CALC_ROSENBROCK:
        return np.array([1.0 + 0.125 * k, 100.0 - 6.0 * k, 0.05 + 0.01 * k], dtype=t)
    if calc == po.CALC_SKEWED_GAUSSIAN_2D:
        return np.array([0.13 + 0.02 * k], dtype=t)
    raise ValueError(calc)


def _chains(K, W, D, calc, dtype, seed, rng):
    """K oracles (params_k, seed + k) with their initial states"""
    t = po.np_dtype(dtype)
    out = []
    for k in range(K):
        p = _params(calc, D, k, rng, t)
        orc = po.Oracle(W, D, calc, p, seed=seed + k, dtype=dtype)
        pos = po.init_positions(dtype, W, D, salt=30 + k)
        logp = orc.logp(pos)
        orc.set_state(pos, logp)
        out.append((orc, p, pos, logp))
    return out


def _check_against_oracles(hip, orcs, n_saved, interval, dtype, threads=4):
    hc, ha = hip.run(n_saved, interval=interval)
    for k, (orc, _, _, _) in enumerate(orcs):
        oc, oa = orc.run(n_saved, interval=interval, mode=po.MODE_COUNTER, threads=threads)
        np.testing.assert_array_equal(ha[k], oa, err_msg="chain %d: accepted per step" % k)
        np.testing.assert_array_equal(hc[k], oc, err_msg="chain %d: stored steps" % k)
    pos, logp, nacc = hip.get_state()
    for k, (orc, _, _, _) in enumerate(orcs):
        opos, ologp, onacc = orc.get_state()
        np.testing.assert_array_equal(pos[k], opos, err_msg="chain %d" % k)
        np.testing.assert_array_equal(logp[k], ologp, err_msg="chain %d" % k)
        np.testing.assert_array_equal(nacc[k], onacc, err_msg="chain %d" % k)
    c = hip.counters()
    assert c["redraws"] == 0
    if dtype == po.F64:
        assert c["near_ties"] == 0
    else:  # (fp32 meets decisions inside the guard band; both sides flag the same ones)
        assert c["near_ties"] == sum(o[0].near_ties for o in orcs)


_MC_ON = {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "0"}
_MC_LATE = {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "0", "MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS": "1", "MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS": "0"}
_MC_16 = {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "0", "MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS": "1", "MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS": "-1"}
_MC_OFF = {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "-1"}


@pytest.mark.gpu
@pytest.mark.parametrize("K,W,D,calc,dtype,env", [
    # dense, matrix-core kernels (even D in 18..32): one launch per step, one per half-step (8 walkers per wavefront), and the
    # 16-walker forms with the next draws behind the accept / in the gather's shadow
    (4, 2048 + 6, 32, po.CALC_DENSE_GAUSSIAN, po.F64, dict(_MC_ON, MCMCPP_HIP_FULL_STEP="1")),
    (4, 2048 + 6, 32, po.CALC_DENSE_GAUSSIAN, po.F64, dict(_MC_ON, MCMCPP_HIP_FULL_STEP="0")),
    (2, 1024 + 38, 26, po.CALC_DENSE_GAUSSIAN, po.F64, dict(_MC_LATE, MCMCPP_HIP_FULL_STEP="0")),
    (4, 1024 + 38, 18, po.CALC_DENSE_GAUSSIAN, po.F64, dict(_MC_16, MCMCPP_HIP_FULL_STEP="0")),
    (2, 2048, 24, po.CALC_DENSE_GAUSSIAN, po.F32, dict(_MC_ON, MCMCPP_HIP_FULL_STEP="1")),
    (4, 1024 + 38, 32, po.CALC_DENSE_GAUSSIAN, po.F32, dict(_MC_LATE, MCMCPP_HIP_FULL_STEP="0")),
    # dense, generic kernels: odd D, and even D with the matrix cores switched off
    (2, 600, 17, po.CALC_DENSE_GAUSSIAN, po.F64, {"MCMCPP_HIP_FULL_STEP": "1"}),
    (4, 600, 17, po.CALC_DENSE_GAUSSIAN, po.F64, {"MCMCPP_HIP_FULL_STEP": "0"}),
    (16, 256, 20, po.CALC_DENSE_GAUSSIAN, po.F64, dict(_MC_OFF, MCMCPP_HIP_FULL_STEP="1")),
    (2, 600, 9, po.CALC_DENSE_GAUSSIAN, po.F32, {"MCMCPP_HIP_FULL_STEP": "0"}),
    # more than 32 768 walkers together: the half-step kernels without forcing
    (4, 16384, 20, po.CALC_DENSE_GAUSSIAN, po.F64, {}),
    # Rosenbrock and the skewed 2-D Gaussian
    (16, 512, 7, po.CALC_ROSENBROCK, po.F64, {"MCMCPP_HIP_FULL_STEP": "1"}),
    (4, 1024 + 2, 33, po.CALC_ROSENBROCK, po.F64, {"MCMCPP_HIP_FULL_STEP": "0"}),
    (2, 2048, 9, po.CALC_ROSENBROCK, po.F32, {"MCMCPP_HIP_FULL_STEP": "1"}),
    (4, 640, 2, po.CALC_SKEWED_GAUSSIAN_2D, po.F64, {"MCMCPP_HIP_FULL_STEP": "1"}),
    (16, 640, 2, po.CALC_SKEWED_GAUSSIAN_2D, po.F64, {"MCMCPP_HIP_FULL_STEP": "0"}),
    (2, 320, 2, po.CALC_SKEWED_GAUSSIAN_2D, po.F32, {"MCMCPP_HIP_FULL_STEP": "0"}),
])
def test_each_chain_follows_its_own_parameters(monkeypatch, K, W, D, calc, dtype, env):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    seed = 40 + K
    orcs = _chains(K, W, D, calc, dtype, seed, np.random.default_rng(W + D + K))
    hip = capi.HipSampler(W, D, calc, np.stack([o[1] for o in orcs]), seed=seed, dtype=dtype, num_chains=K)
    for k, (orc, p, pos, logp) in enumerate(orcs):
        np.testing.assert_array_equal(hip.calc_logp(pos, chain=k), logp, err_msg="chain %d" % k)
    hip.set_state(np.stack([o[2] for o in orcs]), np.stack([o[3] for o in orcs]))
    _check_against_oracles(hip, orcs, 6, 2, dtype)
    _check_against_oracles(hip, orcs, 3, 1, dtype)  # (a second run: the graphs of the first are replayed)


@pytest.mark.gpu
def test_config4_shape_with_a_precision_matrix_per_chain():
    """BASELINE config 4's shape -- 8 chains of 16 384 walkers x 32 dims, dense -- with a precision matrix of its own per chain."""
    K, W, D = 8, 16384, 32
    orcs = _chains(K, W, D, po.CALC_DENSE_GAUSSIAN, po.F64, 0, np.random.default_rng(4))
    hip = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, np.stack([o[1] for o in orcs]), seed=0, num_chains=K)
    hip.set_state(np.stack([o[2] for o in orcs]), np.stack([o[3] for o in orcs]))
    _check_against_oracles(hip, orcs, 5, 1, po.F64, threads=8)


@pytest.fixture(params=["full_step", "half_step"])
def step_path(request, monkeypatch):
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "1" if request.param == "full_step" else "0")
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 12])
def test_chains_left_alone_are_unaffected(step_path, D):
    """Giving chain 1 a block of its own changes chain 1 only: the others stay bit-identical to a shared-parameter handle."""
    K, W, seed = 4, 1024, 3
    rng = np.random.default_rng(D)
    shared = _params(po.CALC_DENSE_GAUSSIAN, D, 0, rng)
    own = _params(po.CALC_DENSE_GAUSSIAN, D, 1, rng)
    pos = np.stack([po.init_positions(po.F64, W, D, salt=50 + k) for k in range(K)])
    orc = po.Oracle(W, D, po.CALC_DENSE_GAUSSIAN, shared, seed=seed)
    logp = np.stack([orc.logp(pos[k]) for k in range(K)])
    orc1 = po.Oracle(W, D, po.CALC_DENSE_GAUSSIAN, own, seed=seed + 1)
    logp_own = logp.copy()
    logp_own[1] = orc1.logp(pos[1])
    a = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, shared, seed=seed, num_chains=K)
    b = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, shared, seed=seed, num_chains=K)
    b.set_chain_params(1, own)
    np.testing.assert_array_equal(b.calc_logp(pos[1], chain=1), logp_own[1])
    for k in (0, 2, 3):
        np.testing.assert_array_equal(b.calc_logp(pos[k], chain=k), logp[k])
    a.set_state(pos, logp)
    b.set_state(pos, logp_own)
    ca, aa = a.run(8)
    cb, ab = b.run(8)
    for k in (0, 2, 3):
        np.testing.assert_array_equal(cb[k], ca[k], err_msg="chain %d" % k)
        np.testing.assert_array_equal(ab[k], aa[k], err_msg="chain %d" % k)
    orc1.set_state(pos[1], logp_own[1])
    oc, oa = orc1.run(8, mode=po.MODE_COUNTER, threads=4)
    np.testing.assert_array_equal(cb[1], oc)
    np.testing.assert_array_equal(ab[1], oa)
    assert not np.array_equal(cb[1], ca[1])


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,calc", [(3, 16, po.CALC_DENSE_GAUSSIAN), (2, 32, po.CALC_DENSE_GAUSSIAN), (1, 24, po.CALC_DENSE_GAUSSIAN),
                                      (4, 5, po.CALC_ROSENBROCK)])
def test_new_parameters_between_runs(step_path, K, D, calc):
    """Run N steps, give every chain new parameters, recompute the log-posteriors with calc_logp_chain, set_state + seek(N), run M
    more: each chain equals a fresh single-chain handle with the new block and seed + k resumed from the same state.  K = 1: a
    handle's target changed without a new handle."""
    W, seed, N, M = 1024, 13, 10, 12
    rng = np.random.default_rng(K * 100 + D)
    first = [_params(calc, D, k, rng) for k in range(K)]
    hip = capi.HipSampler(W, D, calc, np.stack(first) if K > 1 else first[0], seed=seed, num_chains=K)
    lead = (lambda a: a) if K > 1 else (lambda a: a[None])
    pos0 = np.stack([po.init_positions(po.F64, W, D, salt=60 + k) for k in range(K)])
    logp0 = np.stack([hip.calc_logp(pos0[k], chain=k) for k in range(K)])
    hip.set_state(pos0 if K > 1 else pos0[0], logp0 if K > 1 else logp0[0])
    hip.run(N, save_chain=False, want_accepted=False)  # (graphs captured with the create-time parameters)
    pos, _, _ = hip.get_state()
    pos = lead(pos)
    second = [_params(calc, D, k + 7, rng) for k in range(K)]
    for k in range(K):
        hip.set_chain_params(k, second[k])
    logp = np.stack([hip.calc_logp(pos[k], chain=k) for k in range(K)])
    hip.set_state(pos if K > 1 else pos[0], logp if K > 1 else logp[0])
    hip.seek(N)
    chain, acc = hip.run(M)
    chain, acc = lead(chain), lead(acc)
    for k in range(K):
        fresh = capi.HipSampler(W, D, calc, second[k], seed=seed + k)
        np.testing.assert_array_equal(fresh.calc_logp(pos[k]), logp[k])
        fresh.set_state(pos[k], logp[k])
        fresh.seek(N)
        fc, fa = fresh.run(M)
        np.testing.assert_array_equal(chain[k], fc, err_msg="chain %d" % k)
        np.testing.assert_array_equal(acc[k], fa, err_msg="chain %d" % k)
    assert hip.counters()["near_ties"] == 0
    if K == 1:  # (and the handle's own calc_logp now evaluates the new target)
        np.testing.assert_array_equal(hip.calc_logp(pos[0]), logp[0])


@pytest.mark.gpu
@pytest.mark.parametrize("calc,D", [(po.CALC_DENSE_GAUSSIAN, 32), (po.CALC_DENSE_GAUSSIAN, 130), (po.CALC_ROSENBROCK, 11),
                                    (po.CALC_SKEWED_GAUSSIAN_2D, 2)])
@pytest.mark.parametrize("dtype", [po.F64, po.F32])
def test_calc_logp_chain_is_the_oracles_log_posterior(calc, D, dtype):
    K, W = 3, 300
    t = po.np_dtype(dtype)
    rng = np.random.default_rng(D)
    blocks = [_params(calc, D, k, rng, t) for k in range(K)]
    hip = capi.HipSampler(W, D, calc, np.stack(blocks), seed=1, dtype=dtype, num_chains=K)
    pos = po.init_positions(dtype, W, D, salt=70)
    for k in range(K):
        want = po.Oracle(W, D, calc, blocks[k], seed=1, dtype=dtype).logp(pos)
        np.testing.assert_array_equal(hip.calc_logp(pos, chain=k), want, err_msg="chain %d" % k)
    np.testing.assert_array_equal(hip.calc_logp(pos), hip.calc_logp(pos, chain=0))


@pytest.mark.gpu
def test_plugin_functor_gets_its_chains_block(step_path):
    """DiagShifted (tests/cpp/plugin_calc.hip, params = {mu[D], w[D]}, any length) with a block per chain: each chain follows a
    single-chain plug-in handle with that block, and chains whose block is mu = 0, w = 1 follow the built-in IsoGaussian twin."""
    from tests.test_plugin import DIAG_SHIFTED, OUT, SRC
    _build_plugin(OUT, SRC, DIAG_SHIFTED)
    K, W, D, seed = 4, 1024, 10, 5
    rng = np.random.default_rng(9)
    iso = np.concatenate([np.zeros(D), np.ones(D)])
    blocks = [iso, np.concatenate([rng.uniform(-2, 2, D), rng.uniform(0.5, 3, D)]), iso.copy(),
              np.concatenate([rng.uniform(-2, 2, D), rng.uniform(0.5, 3, D)])]
    hip = capi.HipSampler(W, D, DIAG_SHIFTED, np.stack(blocks), seed=seed, num_chains=K)
    pos = np.stack([po.init_positions(po.F64, W, D, salt=80 + k) for k in range(K)])
    logp = np.stack([hip.calc_logp(pos[k], chain=k) for k in range(K)])
    hip.set_state(pos, logp)
    chain, acc = hip.run(10)
    for k in range(K):
        twin = capi.HipSampler(W, D, DIAG_SHIFTED, blocks[k], seed=seed + k)
        np.testing.assert_array_equal(twin.calc_logp(pos[k]), logp[k])
        twin.set_state(pos[k], logp[k])
        tc, ta = twin.run(10)
        np.testing.assert_array_equal(chain[k], tc, err_msg="chain %d" % k)
        np.testing.assert_array_equal(acc[k], ta, err_msg="chain %d" % k)
        if k in (0, 2):
            builtin = capi.HipSampler(W, D, capi.CALC_ISO_GAUSSIAN, None, seed=seed + k)
            np.testing.assert_array_equal(builtin.calc_logp(pos[k]), logp[k])
            builtin.set_state(pos[k], logp[k])
            bc, ba = builtin.run(10)
            np.testing.assert_array_equal(chain[k], bc, err_msg="chain %d" % k)
            np.testing.assert_array_equal(acc[k], ba, err_msg="chain %d" % k)
    assert not np.array_equal(chain[1], chain[3])


def _build_plugin(out, src, calc_id):
    """tests/cpp/plugin_calc.hip -> its shared library (hipcc), DiagShifted registered under calc_id (any parameter count)"""
    capi.build_library()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hdr_dir = os.path.join(ROOT, "mcmcpp_amd", "csrc")
    newest = max(os.path.getmtime(os.path.join(hdr_dir, f)) for f in os.listdir(hdr_dir) if f.endswith((".hpp", ".inc")))
    if not os.path.exists(out) or os.path.getmtime(out) < max(newest, os.path.getmtime(src)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                               "-fPIC", "-shared", "-mllvm", "-amdgpu-kernarg-preload-count=16", "-I" + hdr_dir, src, "-o", out])
    lib = C.CDLL(out)
    tables = []
    for t in ("f64", "f32"):
        f = getattr(lib, "mcmcpp_hip_plugin_diag_shifted_%s" % t)
        f.restype = C.c_void_p
        tables.append(f())
    assert capi.lib().mcmcpp_hip_register_calculator(calc_id, tables[0], tables[1], -1) == 0


def _refused(fn, code, text):
    with pytest.raises(capi.HipError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_refusals():
    W, D, K = 512, 8, 3
    P = _params(po.CALC_DENSE_GAUSSIAN, D, 0, np.random.default_rng(0))
    h = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, num_chains=K)
    L = capi.lib()
    # E_ARG: chain out of range, wrong len, NULL block, a calculator without parameters, the batch target
    _refused(lambda: h.set_chain_params(K, P), E_ARG, "chain 3 outside 0..2")
    _refused(lambda: h.set_chain_params(-1, P), E_ARG, "outside")
    _refused(lambda: h.calc_logp(np.zeros((4, D)), chain=K), E_ARG, "outside")
    _refused(lambda: h.set_chain_params(1, P[:-1]), E_ARG, "len 63")
    assert L.mcmcpp_hip_set_chain_params(h.h, 1, None, D * D) == E_ARG
    assert b"NULL" in L.mcmcpp_hip_last_error(h.h)
    iso = capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, num_chains=K)
    _refused(lambda: iso.set_chain_params(0, np.zeros(1)), E_ARG, "takes no parameters")
    x = np.zeros((4, D))
    np.testing.assert_array_equal(iso.calc_logp(x, chain=2), iso.calc_logp(x))  # (no parameters: every chain is the same)
    batch = capi.HipSampler(W, D, capi.CALC_BATCH, None, batch_callback=(capi.BATCH_LOGP_FN(lambda *a: 0), None))
    _refused(lambda: batch.set_chain_params(0, np.zeros(1)), E_ARG, "batch target takes no parameters")
    # E_UNSUPPORTED: differential evolution, shards, a communicator, caller-owned positions
    de = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    _refused(lambda: de.set_chain_params(0, P), E_UNSUPPORTED, "stretch-move handles only")
    _refused(lambda: de.calc_logp(x, chain=0), E_UNSUPPORTED, "stretch-move handles only")
    shard = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, shard_begin=0, shard_count=W // 4)
    _refused(lambda: shard.set_chain_params(0, P), E_UNSUPPORTED, "sharded")
    comm = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, comm_world=1, comm_rank=0, comm_id=capi.comm_unique_id())
    _refused(lambda: comm.set_chain_params(0, P), E_UNSUPPORTED, "communicator")
    import torch
    buf = torch.zeros((W, D), dtype=torch.float64, device="cuda")
    owned = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, device_positions=buf.data_ptr())
    _refused(lambda: owned.set_chain_params(0, P), E_UNSUPPORTED, "caller-owned positions")
    # while an asynchronous run is live: the code every other entry point returns then
    pos = po.init_positions(po.F64, W, D, salt=1)
    h1 = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P)
    h1.set_state(pos, h1.calc_logp(pos))
    h1.run_async(200)
    _refused(lambda: h1.set_chain_params(0, P), E_STATE, "asynchronous run is in progress")
    _refused(lambda: h1.calc_logp(pos, chain=0), E_STATE, "asynchronous run is in progress")
    h1.run_wait()
    h1.set_chain_params(0, P)  # (and accepted once it has ended)


def test_entry_points_need_a_handle():
    """CPU: the two entry points exist and refuse a NULL handle."""
    capi.build_library()
    L = capi.lib()
    assert L.mcmcpp_hip_set_chain_params(None, 0, None, 0) == E_ARG
    assert L.mcmcpp_hip_calc_logp_chain(None, 0, None, 0, None) == E_ARG


def test_header_declares_the_entry_points_as_c99(tmp_path):
    """CPU: a C99 translation unit that calls both functions compiles warning-free."""
    src = tmp_path / "chain_params.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int set_and_eval(mcmcpp_hip_sampler* h, const double* p, int32_t len, const double* pos, double* out)\n'
                   '{\n'
                   '    int rc = mcmcpp_hip_set_chain_params(h, 1, p, len);\n'
                   '    if (rc != MCMCPP_HIP_OK) return rc;\n'
                   '    return mcmcpp_hip_calc_logp_chain(h, 1, pos, (int64_t)4, out);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "chain_params.o")])
    assert "mcmcpp_hip_set_chain_params" in capi.EXPORTS and "mcmcpp_hip_calc_logp_chain" in capi.EXPORTS
