"""Stored steps that stay in device memory: mcmcpp_hip_run_device, run_device_async, calc_logp_device and
moments_add_device_steps_strided.

run_device computes the run mcmcpp_hip_run computes and leaves the stored steps in the caller's device array.  The reference of
every GPU case is therefore a twin handle with the same seed driven through mcmcpp_hip_run into host memory (and the golden
fixture where the shape has one): the device chain copied back, positions, log-posteriors, per-walker counters, per-step
accepted counts, near_ties and redraws are bit-identical.  Every destination lies between two guards of at least one stored
step each, filled -- like the destination itself -- with a NaN pattern: both guards must be untouched afterwards, and no cell
of the destination may still hold the pattern.  No case provokes a fault: a host pointer is refused by the runtime's pointer
attributes before anything is launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po
from tests.goldens import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcmcpp_hip_run_device", "mcmcpp_hip_run_device_async", "mcmcpp_hip_calc_logp_device", "mcmcpp_hip_moments_add_device_steps_strided"]
E_ARG, E_UNSUPPORTED, E_STATE = 1, 4, 5


# ---- CPU: the interface -----------------------------------------------------------------------------------------------------

def test_header_declares_the_device_chain_interface(tmp_path):
    header = open(os.path.join(ROOT, "include", "mcmcpp_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in capi.EXPORTS
    assert re.search(r"#define\s+MCMCPP_HIP_ABI_VERSION\s+2\b", header)
    src = tmp_path / "use.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int use(mcmcpp_hip_sampler* h, mcmcpp_hip_moments* m, void* dev, uint32_t* acc)\n'
                   '{\n'
                   '  int rc = mcmcpp_hip_run_device(h, 20, 100, dev, acc);\n'
                   '  rc += mcmcpp_hip_run_device_async(h, 20, 100, dev, 0);\n'
                   '  rc += mcmcpp_hip_wait_stored(h, 10) + mcmcpp_hip_run_wait(h);\n'
                   '  rc += mcmcpp_hip_calc_logp_device(h, 0, dev, (int64_t)20 * 64, dev);\n'
                   '  rc += mcmcpp_hip_moments_add_device_steps_strided(m, dev, 4, 5);\n'
                   '  return rc;\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "use.o")])


def test_the_library_exports_the_device_chain_interface():
    capi.build_library()
    L = C.CDLL(capi.library_path())
    for name in NEW:
        assert hasattr(L, name), name
    for name in ("run_device", "run_device_async", "calc_logp_device"):
        assert callable(getattr(capi.HipSampler, name))


def test_the_wrapper_keeps_torch_lazy():
    """import torch stays inside the calls that need it, as for log_prob."""
    text = open(os.path.join(ROOT, "mcmcpp_amd", "capi.py")).read()
    assert not re.search(r"^(import torch|from torch)", text, re.M)


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def _torch():
    import torch
    return torch


PATTERN = {8: np.uint64(0x7FF8C0DEC0DEC0DE), 4: np.uint32(0x7FC0C0DE)}  # quiet NaNs with a payload nothing computes


class Guarded:
    """A device destination of `shape` = (..., W, D) between two guards of at least one stored step (a multiple of 16 bytes)."""

    def __init__(self, shape, np_t):
        torch = _torch()
        self.item = np.dtype(np_t).itemsize
        self.bits = PATTERN[self.item]
        self.n = int(np.prod(shape))
        self.g = (shape[-2] * shape[-1] + 3) // 4 * 4
        host = np.full(self.g + self.n + self.g, self.bits).view(np_t)
        self.buf = torch.from_numpy(host).cuda()
        self.out = self.buf[self.g:self.g + self.n].view(shape)
        assert self.out.data_ptr() % 16 == 0 and self.out.is_contiguous()

    def check(self):
        """Both guards untouched, every cell of the destination written; returns the destination as numpy."""
        back = self.buf.cpu().numpy()
        raw = back.view(self.bits.dtype)
        assert (raw[:self.g] == self.bits).all(), "the guard in front of the destination was written"
        assert (raw[self.g + self.n:] == self.bits).all(), "the guard behind the destination was written"
        assert not (raw[self.g:self.g + self.n] == self.bits).any(), "a cell of the destination was never written"
        return back[self.g:self.g + self.n].reshape(tuple(self.out.shape))


def _same_handles(a, b):
    for x, y, what in zip(a.get_state(), b.get_state(), ("positions", "logp", "n_accept")):
        np.testing.assert_array_equal(x, y, err_msg=what)
    assert a.counters() == b.counters()


def _twins(make, pos, logp, n_saved, interval, runs=1):
    """make() twice; one twin through run into host memory, the other through run_device.  Returns (handle, device tensor,
    host chain) of the last of `runs` consecutive runs."""
    host, dev = make(), make()
    host.set_state(pos, logp)
    dev.set_state(pos, logp)
    for _ in range(runs):
        want_chain, want_acc = host.run(n_saved, interval=interval)
        lead = (dev.K,) if dev.K > 1 else ()
        dst = Guarded(lead + (n_saved, dev.W, dev.D), dev.np_t)
        got, got_acc = dev.run_device(n_saved, interval=interval, out=dst.out)
        assert got is dst.out
        np.testing.assert_array_equal(dst.check(), want_chain)
        np.testing.assert_array_equal(got_acc, want_acc)
        _same_handles(dev, host)
    return dev, dst.out, want_chain


def _golden_twins(name, n_saved, interval, **kw):
    g = Golden(name)
    make = lambda: capi.HipSampler(g.W, g.D, g.calc, g.params, seed=g.seed, dtype=g.dtype, alpha=g.alpha, mover=g.mover, **kw)
    _, _, chain = _twins(make, g.init_pos, g.init_logp, n_saved, interval)
    # the fixture's own stored steps (the reference ran it with slicing g.slicing = 1)
    assert g.slicing == 1
    for k in g.full_steps:
        if k % interval == 0 and k // interval <= n_saved:
            g.check_chain_step(k, chain[k // interval - 1])


def _dense(D, np_t, seed):
    a = np.random.default_rng(seed).standard_normal((D, D))
    return (a @ a.T / D + np.eye(D)).astype(np_t).ravel()


def _start(W, D, calc, params, dtype, salt=3, K=1):
    pos = np.stack([po.init_positions(dtype, W, D, salt=salt + k) for k in range(K)])
    orc = po.Oracle(W, D, calc, params, dtype=dtype)
    logp = np.stack([orc.logp(p) for p in pos])
    return (pos, logp) if K > 1 else (pos[0], logp[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_saved,interval", [
    ("iso64x4", 70, 1),        # more stored steps than the largest ring of the host path: a slot reused or masked shows
    ("iso64x4", 9, 3),         # the host path forwards slices between stored steps
    ("iso64x4", 5, 1),         # an odd total: the ensemble comes home from the second buffer
    ("dense96x16", 6, 2),
    ("dense80x5_f32", 6, 2),
])
def test_full_step_kernels(name, n_saved, interval):
    _golden_twins(name, n_saved, interval)


@pytest.mark.gpu
@pytest.mark.parametrize("batch_draws", [None, "0"])
def test_matrix_core_full_step_kernel(monkeypatch, batch_draws):
    """64 x 20 dense fp64 (D in 18..32): draw records made ahead in batches, and made by the launches themselves."""
    if batch_draws is not None:
        monkeypatch.setenv("MCMCPP_HIP_BATCH_DRAWS", batch_draws)
    W, D = 64, 20
    P = _dense(D, np.float64, 7)
    pos, logp = _start(W, D, po.CALC_DENSE_GAUSSIAN, P, po.F64)
    _twins(lambda: capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, seed=13), pos, logp, 6, 2, runs=2)


@pytest.mark.gpu
def test_half_step_kernels_golden(monkeypatch):
    """Nine stored steps are five sub-chunks on the host path (an eighth of the run each) and one piece on the device path."""
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "0")
    _golden_twins("iso100x7", 9, 2)


@pytest.mark.gpu
def test_half_step_kernels_at_a_step_of_168_bytes(monkeypatch):
    """14 x 3 fp32: a stored step that is no multiple of 16 bytes, the host path that can never trickle."""
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "0")
    W, D = 14, 3
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F32)
    _twins(lambda: capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=3, dtype=po.F32), pos, logp, 9, 2, runs=2)


@pytest.mark.gpu
def test_full_step_kernel_at_a_step_of_168_bytes():
    W, D = 14, 3
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F32)
    _twins(lambda: capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=3, dtype=po.F32), pos, logp, 9, 2)


def _single_chain_runs(W, D, calc, blocks, seed, pos, logp, n_saved, interval):
    out = []
    for k, prm in enumerate(blocks):
        h = capi.HipSampler(W, D, calc, prm, seed=seed + k)
        h.set_state(pos[k], logp[k])
        out.append(h.run(n_saved, interval=interval)[0])
    return out


@pytest.mark.gpu
def test_several_chains_iso():
    W, D, K, seed, n_saved, interval = 64, 4, 3, 40, 7, 2
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64, K=K)
    _, out, chain = _twins(lambda: capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=seed, num_chains=K), pos, logp, n_saved, interval)
    assert tuple(out.shape) == (K, n_saved, W, D)
    for k, want in enumerate(_single_chain_runs(W, D, po.CALC_ISO_GAUSSIAN, [None] * K, seed, pos, logp, n_saved, interval)):
        np.testing.assert_array_equal(out[k].cpu().numpy(), want, err_msg="chain %d" % k)


@pytest.fixture(scope="module")
def dense_k3():
    """96 x 16 dense, K = 3, chain 1 with a block of its own: (handle, device chain (K, 6, W, D), blocks, start)."""
    W, D, K, seed = 96, 16, 3, 50
    blocks = [_dense(D, np.float64, 1), _dense(D, np.float64, 2), _dense(D, np.float64, 1)]
    pos = np.stack([po.init_positions(po.F64, W, D, salt=5 + k) for k in range(K)])
    logp = np.stack([po.Oracle(W, D, po.CALC_DENSE_GAUSSIAN, blocks[k]).logp(pos[k]) for k in range(K)])

    def make():
        h = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, blocks[0], seed=seed, num_chains=K)
        h.set_chain_params(1, blocks[1])
        return h
    dev, out, _ = _twins(make, pos, logp, 6, 2)
    return dev, out, blocks, (W, D, seed, pos, logp)


@pytest.mark.gpu
def test_several_chains_dense_with_a_block_of_its_own(dense_k3):
    dev, out, blocks, (W, D, seed, pos, logp) = dense_k3
    for k, want in enumerate(_single_chain_runs(W, D, po.CALC_DENSE_GAUSSIAN, blocks, seed, pos, logp, 6, 2)):
        np.testing.assert_array_equal(out[k].cpu().numpy(), want, err_msg="chain %d" % k)


@pytest.mark.gpu
def test_calc_logp_device_with_chain_parameters(dense_k3):
    dev, out, blocks, _ = dense_k3
    for k in range(3):
        got = dev.calc_logp_device(out[k], chain=k)
        assert tuple(got.shape) == tuple(out[k].shape[:-1]) and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy().ravel(), dev.calc_logp(out[k].cpu().numpy(), chain=k))
    # (chains 0 and 1 differ in their parameters: the same rows give other values)
    assert not np.array_equal(dev.calc_logp_device(out[0], chain=1).cpu().numpy(), dev.calc_logp_device(out[0], chain=0).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_saved,interval", [("de_iso14x3", 12, 1), ("de_iso64x4", 8, 2)])
def test_differential_evolution(name, n_saved, interval):
    _golden_twins(name, n_saved, interval)


@pytest.mark.gpu
def test_differential_evolution_across_a_piece_boundary():
    """The largest stored step the mover accepts at the smallest step count: 2050 x 1024 fp64 (the smallest even W above 2 D)
    is 16 793 600 bytes, so the 256 MiB of device chain behind a host destination hold 15 stored steps and a run of 17 leaves
    in two pieces (15 + 2: plan_de_pieces, tests/test_run_entry.py).  The twin stores into device memory, which is one piece
    by construction.  Chains, per-step accepted counts, final states and counters are identical; a run that set the mover's
    error flag would have failed.  The other bound of a piece, 64 MiB of accepted counters, needs more than 2^24 ensemble
    steps in one run -- minutes, not seconds, at any shape: the CPU grid of tests/test_run_entry.py is its check."""
    W, D, n_saved = 2050, 1024, 17
    assert (256 << 20) // (W * D * 8) == 15 < n_saved
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    make = lambda: capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=11, mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    dev = _twins(make, pos, logp, n_saved, 1)[0]
    c = dev.counters()
    assert c["near_ties"] == 0 and c["ensemble_steps"] == n_saved
    # (the 320 MB destination goes back to the runtime: left in torch's cache, it would be carved up for later tests' tensors)
    _torch().cuda.empty_cache()


# ---- batch targets ------------------------------------------------------------------------------------------------------------

from tests.test_batch_calc import CTarget, _torch_iso, cb_lib  # noqa: E402,F401  (the callback library's fixture and a torch target)


def _fused_iso(W, D, seed, pos, logp, n_saved, interval, monkeypatch):
    monkeypatch.setenv("MCMCPP_HIP_FULL_STEP", "0")
    f = capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=seed)
    f.set_state(pos, logp)
    return f, f.run(n_saved, interval=interval)


@pytest.mark.gpu
def test_batch_target_c_callback(cb_lib, monkeypatch):
    W, D, seed, n_saved, interval = 64, 4, 17, 6, 1
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    tgt = CTarget(cb_lib, po.CALC_ISO_GAUSSIAN, D, None, po.F64)
    make = lambda: capi.HipSampler(W, D, capi.CALC_BATCH, seed=seed, batch_callback=tgt.callback())
    dev, out, chain = _twins(make, pos, logp, n_saved, interval)
    f, (want_chain, _) = _fused_iso(W, D, seed, pos, logp, n_saved, interval, monkeypatch)
    np.testing.assert_array_equal(chain, want_chain)
    _same_handles(dev, f)
    # calc_logp_device: the callback on the stored rows themselves, several chunks of W/2 rows
    got = dev.calc_logp_device(out)
    assert tuple(got.shape) == (n_saved, W)
    np.testing.assert_array_equal(got.cpu().numpy().ravel(), dev.calc_logp(chain))
    np.testing.assert_array_equal(got.cpu().numpy().ravel(), f.calc_logp(chain))
    with pytest.raises(capi.HipError) as e:
        dev.calc_logp_device(out, chain=1)
    assert e.value.code == E_ARG and "chain" in str(e.value)


@pytest.mark.gpu
def test_batch_target_across_sub_chunks(cb_lib, monkeypatch):
    """Nine stored steps, two ensemble steps apart: the host destination takes them in five sub-chunks (an eighth of the run,
    rounded up, is two stored steps; the last sub-chunk holds one), the device destination in one.  Both are the chain of the
    fused half-step kernels."""
    W, D, seed, n_saved, interval = 64, 4, 29, 9, 2
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    tgt = CTarget(cb_lib, po.CALC_ISO_GAUSSIAN, D, None, po.F64)
    make = lambda: capi.HipSampler(W, D, capi.CALC_BATCH, seed=seed, batch_callback=tgt.callback())
    dev, _, chain = _twins(make, pos, logp, n_saved, interval)
    f, (want_chain, _) = _fused_iso(W, D, seed, pos, logp, n_saved, interval, monkeypatch)
    np.testing.assert_array_equal(chain, want_chain)
    _same_handles(dev, f)


@pytest.mark.gpu
def test_batch_target_torch_log_prob(monkeypatch):
    torch = _torch()
    W, D, seed, n_saved, interval = 64, 4, 19, 5, 2
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    make = lambda: capi.HipSampler(W, D, capi.CALC_BATCH, seed=seed, log_prob=_torch_iso)
    dev, out, chain = _twins(make, pos, logp, n_saved, interval)
    assert isinstance(out, torch.Tensor) and out.is_cuda
    f, (want_chain, _) = _fused_iso(W, D, seed, pos, logp, n_saved, interval, monkeypatch)
    np.testing.assert_array_equal(chain, want_chain)
    _same_handles(dev, f)
    np.testing.assert_array_equal(dev.calc_logp_device(out).cpu().numpy().ravel(), f.calc_logp(chain))


# ---- asynchronous ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_run_device_async_and_wait_stored():
    torch = _torch()
    W, D, n_saved, interval = 64, 4, 40, 2
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    # (a graph replay of four steps: chunks of two stored steps, so that wait_stored has progress to hear of)
    make = lambda: capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=23, graph_steps=4)
    host, dev = make(), make()
    host.set_state(pos, logp)
    dev.set_state(pos, logp)
    want_chain, want_acc = host.run(n_saved, interval=interval)
    dst = Guarded((n_saved, W, D), np.float64)
    got, acc = dev.run_device_async(n_saved, interval=interval, out=dst.out, want_accepted=True)
    dev.wait_stored(10)
    mine = torch.cuda.Stream()
    with torch.cuda.stream(mine):
        first = got[:10].clone()
    mine.synchronize()
    with pytest.raises(capi.HipError) as e:  # between run_device_async and run_wait the handle accepts only wait_stored
        dev.run_device(1, out=dst.out[:1])
    assert e.value.code == E_STATE and "asynchronous run" in str(e.value)
    assert capi.lib().mcmcpp_hip_run_wait(dev.h) == 0
    np.testing.assert_array_equal(first.cpu().numpy(), want_chain[:10])
    np.testing.assert_array_equal(dst.check(), want_chain)
    np.testing.assert_array_equal(acc, want_acc)
    _same_handles(dev, host)


# ---- sample and analyse without leaving the device ------------------------------------------------------------------------------

@pytest.mark.gpu
def test_pipeline_on_one_device_chain():
    W, D, n_saved = 96, 16, 64
    P = _dense(D, np.float64, 4)
    pos, logp = _start(W, D, po.CALC_DENSE_GAUSSIAN, P, po.F64)
    s = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, seed=31)
    s.set_state(pos, logp)
    dst = Guarded((n_saved, W, D), np.float64)
    chain, _ = s.run_device(n_saved, out=dst.out)
    host = dst.check()

    a, b = capi.HipHistograms(W, D, 20), capi.HipHistograms(W, D, 20)
    a.compute_device(chain, slice_interval=3)
    b.compute(host, slice_interval=3)
    for x, y in zip(a.result(), b.result()):
        np.testing.assert_array_equal(x, y)

    np.testing.assert_array_equal(capi.autocorr_times_device(chain), capi.autocorr_times(host))

    ma, mb = capi.HipMoments(W, D), capi.HipMoments(W, D)
    ma.add_device_steps(chain, slice_interval=5)
    mb.add_steps(host, slice_interval=5)
    (na, mean_a, cov_a, corr_a), (nb, mean_b, cov_b, corr_b) = ma.finish(), mb.finish()
    assert na == nb == len(host[::5]) * W
    # the tolerance tests/test_moments.py states for fp64: covariance within 1e-10 sqrt(var_i var_j), correlation within 1e-10
    scale = np.sqrt(np.abs(np.outer(np.diag(cov_b), np.diag(cov_b))))
    print("moments: max |cov difference| / scale = %g, max |corr difference| = %g" % ((np.abs(cov_a - cov_b) / scale).max(), np.abs(corr_a - corr_b).max()))
    assert np.all(np.abs(cov_a - cov_b) <= 1e-10 * scale) and np.all(np.abs(corr_a - corr_b) <= 1e-10)
    # ... and in fact identical: the steps used are gathered on the device into the chunks add_steps uploads, and summed alike
    for x, y in ((mean_a, mean_b), (cov_a, cov_b), (corr_a, corr_b)):
        np.testing.assert_array_equal(x, y)
    # the raw address of the same steps, as callers without torch give it
    mc = capi.HipMoments(W, D)
    mc.add_device_steps(chain.data_ptr(), n_saved, slice_interval=5)
    np.testing.assert_array_equal(mc.finish()[2], cov_a)

    lp = s.calc_logp_device(chain)
    assert tuple(lp.shape) == (n_saved, W)
    np.testing.assert_array_equal(lp.cpu().numpy().ravel(), s.calc_logp(host))
    # the last stored step is the walkers' state: its log-posteriors are the handle's
    np.testing.assert_array_equal(lp[-1].cpu().numpy(), s.get_state()[1])

    # shape and dtype of a tensor are checked against the handle
    with pytest.raises(ValueError):
        ma.add_device_steps(chain[:, :, :8].contiguous())
    with pytest.raises(ValueError):
        a.compute_device(chain.float())
    with pytest.raises(ValueError):
        s.run_device(3, out=chain)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_leave_the_handle_alive():
    torch = _torch()
    W, D = 64, 4
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    make = lambda **kw: capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=2, **kw)
    s, twin = make(), make()
    s.set_state(pos, logp)
    twin.set_state(pos, logp)
    L = capi.lib()

    def refused(rc, code, *words):
        msg = L.mcmcpp_hip_last_error(s.h).decode()
        assert rc == code, (rc, msg)
        assert msg and all(w in msg for w in words), msg

    pageable = np.zeros((3, W, D))
    refused(L.mcmcpp_hip_run_device(s.h, 3, 1, pageable.ctypes.data, None), E_ARG, "not device memory")
    assert not pageable.any(), "a host pointer must be refused, not written"
    pinned = capi.pinned_empty((3, W, D))
    pinned[:] = 0
    refused(L.mcmcpp_hip_run_device(s.h, 3, 1, pinned.ctypes.data, None), E_ARG, "not device memory")
    assert not pinned.any()
    dev = torch.zeros(3 * W * D + 2, dtype=torch.float64, device="cuda")
    refused(L.mcmcpp_hip_run_device(s.h, 3, 1, dev.data_ptr() + 8, None), E_ARG, "16-byte aligned")
    refused(L.mcmcpp_hip_run_device(s.h, 3, 1, None, None), E_ARG, "NULL")
    refused(L.mcmcpp_hip_run_device(s.h, -1, 1, dev.data_ptr(), None), E_ARG)
    assert L.mcmcpp_hip_run_device(s.h, 0, 1, None, None) == 0  # nothing to store: NULL is fine
    assert not dev.cpu().numpy().any()

    lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    x = torch.from_numpy(pos).cuda()
    refused(L.mcmcpp_hip_calc_logp_device(s.h, 1, x.data_ptr(), W, lp.data_ptr()), E_ARG, "chain 1")
    refused(L.mcmcpp_hip_calc_logp_device(s.h, -1, x.data_ptr(), W, lp.data_ptr()), E_ARG, "chain -1")
    refused(L.mcmcpp_hip_calc_logp_device(s.h, 0, pos.ctypes.data, W, lp.data_ptr()), E_ARG, "not device memory")
    refused(L.mcmcpp_hip_calc_logp_device(s.h, 0, x.data_ptr(), W, logp.copy().ctypes.data), E_ARG, "not device memory")

    # between run_async and run_wait
    chain, _ = s.run_async(4)
    rc = L.mcmcpp_hip_run_device(s.h, 3, 1, dev.data_ptr(), None)
    rc2 = L.mcmcpp_hip_calc_logp_device(s.h, 0, x.data_ptr(), W, lp.data_ptr())
    msg = L.mcmcpp_hip_last_error(s.h).decode()
    s.run_wait()
    assert rc == E_STATE and rc2 == E_STATE and "asynchronous run" in msg
    twin.run(4)

    # the handle has lost nothing: it goes on as its twin does
    got, _ = s.run_device(5, interval=2)
    np.testing.assert_array_equal(got.cpu().numpy(), twin.run(5, interval=2)[0])
    _same_handles(s, twin)
    np.testing.assert_array_equal(s.calc_logp_device(x).cpu().numpy(), logp)

    # before set_state
    fresh = make()
    with pytest.raises(capi.HipError) as e:
        fresh.run_device(2)
    assert e.value.code == E_STATE

    # a sharded handle stores through bind_device_chain
    shard = make(shard_begin=0, shard_count=W // 4)
    shard.set_state(pos, logp)
    with pytest.raises(capi.HipError) as e:
        shard.run_device(2)
    assert e.value.code == E_UNSUPPORTED and "sharded" in str(e.value)


@pytest.mark.gpu
def test_chain_must_be_zero_on_de_and_batch_handles():
    torch = _torch()
    W, D = 64, 4
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    x = torch.from_numpy(pos).cuda()
    de = capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    np.testing.assert_array_equal(de.calc_logp_device(x).cpu().numpy(), logp)
    noop = capi.BATCH_LOGP_FN(lambda *a: 0)
    batch = capi.HipSampler(W, D, capi.CALC_BATCH, batch_callback=(noop, None))
    for h in (de, batch):
        with pytest.raises(capi.HipError) as e:
            h.calc_logp_device(x, chain=1)
        assert e.value.code == E_ARG and "chain 1" in str(e.value)
    # a host destination is refused by these movers as well
    de.set_state(pos, logp)
    batch.set_state(pos, logp)
    host = np.zeros((2, W, D))
    for h in (de, batch):
        assert capi.lib().mcmcpp_hip_run_device(h.h, 2, 1, host.ctypes.data, None) == E_ARG
        assert "not device memory" in capi.lib().mcmcpp_hip_last_error(h.h).decode()
    assert not host.any()


# ---- tensors that torch is still working on, or that are views ---------------------------------------------------------------

def _views(chain, W):
    """Views of a stored chain that are not contiguous, and tensors whose producer has only just been enqueued."""
    return [("every fifth step", chain[::5]), ("the red half", chain[:, :W // 2]), ("one walker", chain[:, 3]),
            ("just made", chain.flip(0) + 0.0), ("a transposed copy of rows", chain[:4].transpose(0, 1))]


@pytest.mark.gpu
def test_calc_logp_device_of_views_and_fresh_tensors():
    """The library launches on streams of its own: the wrapper has to order them behind torch's stream, which makes x
    contiguous (a copy kernel) and allocates the result."""
    W, D, n_saved = 96, 16, 20
    P = _dense(D, np.float64, 4)
    pos, logp = _start(W, D, po.CALC_DENSE_GAUSSIAN, P, po.F64)
    s = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P, seed=31)
    s.set_state(pos, logp)
    chain, _ = s.run_device(n_saved)
    for what, x in _views(chain, W):
        got = s.calc_logp_device(x)
        assert tuple(got.shape) == tuple(x.shape[:-1]), what
        np.testing.assert_array_equal(got.cpu().numpy().ravel(), s.calc_logp(x.cpu().numpy()), err_msg=what)
    # the analysis entry points behind work torch has only just enqueued
    fresh = chain.flip(0).flip(0) + 0.0
    a, b = capi.HipMoments(W, D), capi.HipMoments(W, D)
    a.add_device_steps(fresh)
    b.add_device_steps(chain)
    for x, y in zip(a.finish(), b.finish()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(capi.autocorr_times_device(chain.flip(0).flip(0) + 0.0), capi.autocorr_times_device(chain))
    ha, hb = capi.HipHistograms(W, D, 20), capi.HipHistograms(W, D, 20)
    ha.compute_device(chain.flip(0).flip(0) + 0.0)
    hb.compute_device(chain)
    for x, y in zip(ha.result(), hb.result()):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_calc_logp_device_of_views_batch_targets(cb_lib, monkeypatch):
    W, D, seed, n_saved = 64, 4, 17, 10
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    tgt = CTarget(cb_lib, po.CALC_ISO_GAUSSIAN, D, None, po.F64)
    c = capi.HipSampler(W, D, capi.CALC_BATCH, seed=seed, batch_callback=tgt.callback())
    t = capi.HipSampler(W, D, capi.CALC_BATCH, seed=seed, log_prob=_torch_iso)
    f, _ = _fused_iso(W, D, seed, pos, logp, 1, 1, monkeypatch)
    c.set_state(pos, logp)
    chain, _ = c.run_device(n_saved)
    for what, x in _views(chain, W):
        want = f.calc_logp(x.cpu().numpy())
        for h in (c, t):
            got = h.calc_logp_device(x)
            assert tuple(got.shape) == tuple(x.shape[:-1]), what
            np.testing.assert_array_equal(got.cpu().numpy().ravel(), want, err_msg=what)


@pytest.mark.gpu
def test_batch_chunks_are_16_byte_aligned(cb_lib):
    """14 x 3 fp32: W/2 = 7 rows are 84 bytes of rows and 28 bytes of log-posteriors.  Chunks of 4 rows keep every pointer the
    callback is handed 16-byte aligned, as in a run."""
    torch = _torch()
    W, D = 14, 3
    seen = []

    def cb(user, proposals, logp_out, count, num_params, hip_stream):
        seen.append((proposals, logp_out, count))
        return 0
    h = capi.HipSampler(W, D, capi.CALC_BATCH, dtype=po.F32, batch_callback=(capi.BATCH_LOGP_FN(cb), None))
    x = torch.zeros((30, D), dtype=torch.float32, device="cuda")
    h.calc_logp_device(x)
    assert [c for _, _, c in seen] == [4] * 7 + [2]
    assert all(p % 16 == 0 and l % 16 == 0 for p, l, _ in seen)
    assert seen[0][0] == x.data_ptr() and seen[1][0] == x.data_ptr() + 4 * D * 4
    # the values: the C callback in the same chunks against the fused handle
    tgt = CTarget(cb_lib, po.CALC_ISO_GAUSSIAN, D, None, po.F32)
    c = capi.HipSampler(W, D, capi.CALC_BATCH, dtype=po.F32, batch_callback=tgt.callback())
    rows = po.init_positions(po.F32, 30, D, salt=9)
    got = c.calc_logp_device(torch.from_numpy(rows).cuda())
    np.testing.assert_array_equal(got.cpu().numpy(), capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, dtype=po.F32).calc_logp(rows))


@pytest.mark.gpu
def test_torch_target_goes_through_the_library():
    """calc_logp_device of a log_prob handle is the C entry point: refused during an asynchronous run, the callback's result
    validated, its failures E_CALLBACK."""
    torch = _torch()
    W, D = 64, 4
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    x = torch.from_numpy(pos).cuda()
    t = capi.HipSampler(W, D, capi.CALC_BATCH, seed=1, log_prob=_torch_iso)
    t.set_state(pos, logp)
    np.testing.assert_array_equal(t.calc_logp_device(x).cpu().numpy(), logp)
    with pytest.raises(capi.HipError) as e:
        t.calc_logp_device(x, chain=1)
    assert e.value.code == E_ARG and "chain 1" in str(e.value)
    t.run_device_async(6)
    with pytest.raises(capi.HipError) as e:
        t.calc_logp_device(x)
    t.run_wait()
    assert e.value.code == E_STATE and "asynchronous run" in str(e.value)
    # rows the wrapper has not announced (a bare C call): the callback cannot wrap them, and says so
    lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    assert capi.lib().mcmcpp_hip_calc_logp_device(t.h, 0, x.data_ptr(), W, lp.data_ptr()) == capi.E_CALLBACK
    assert isinstance(t._cb_error, ValueError)
    t._cb_error = None
    bad = capi.HipSampler(W, D, capi.CALC_BATCH, log_prob=lambda v: v.sum(1, keepdim=True))
    with pytest.raises(capi.HipError) as e:
        bad.calc_logp_device(x)
    assert e.value.code == capi.E_CALLBACK and isinstance(e.value.__cause__, TypeError)


@pytest.mark.gpu
def test_a_destination_must_end_inside_its_allocation():
    """Device memory from the first byte is not enough: the array has to lie in ONE allocation.  A 64 MiB tensor is an
    allocation of its own to the caching allocator; a destination of three stored steps that starts two steps before its end
    is refused, the same start with two steps is stored into."""
    torch = _torch()
    W, D = 64, 4
    pos, logp = _start(W, D, po.CALC_ISO_GAUSSIAN, None, po.F64)
    s = capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=2)
    s.set_state(pos, logp)
    block = torch.zeros(64 << 17, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    seg = [b for b in torch.cuda.memory_snapshot() if b["address"] <= block.data_ptr() < b["address"] + b["total_size"]]
    assert len(seg) == 1 and seg[0]["address"] == block.data_ptr() and seg[0]["total_size"] == block.numel() * 8, "the tensor is not an allocation of its own"
    tail = block.data_ptr() + (block.numel() - 2 * W * D) * 8
    L = capi.lib()
    assert L.mcmcpp_hip_run_device(s.h, 3, 1, tail, None) == E_ARG
    msg = L.mcmcpp_hip_last_error(s.h).decode()
    assert "allocation ends" in msg and str(2 * W * D * 8) in msg, msg
    assert not block.cpu().numpy().any()
    assert L.mcmcpp_hip_run_device(s.h, 2, 1, tail, None) == 0
    twin = capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=2)
    twin.set_state(pos, logp)
    np.testing.assert_array_equal(block[-2 * W * D:].cpu().numpy().reshape(2, W, D), twin.run(2)[0])
    lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    assert L.mcmcpp_hip_calc_logp_device(s.h, 0, tail, 3 * W, lp.data_ptr()) == E_ARG
    assert "allocation ends" in L.mcmcpp_hip_last_error(s.h).decode()
