"""GPU side of tests/test_ess.py, run in a child process under a time limit of its own:
    python -m tests.ess_device '<json spec>' <out.npz>
One child runs every case of the spec and writes, per case, what the library returned through the host-pointer and the device
entry points; the parent builds the same samples from the same spec (make_series) and compares with the restatement
(tests/ess_restatement.py) bit for bit.  A HIP error ends the child at once: capi raises, nothing catches it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.rhat_device import make_steps, place_on_device, reshaped  # noqa: E402

KEYS = ("ess", "tau", "lags_used", "closed", "rho", "autocov", "rhat", "mean", "within", "between")
FIRST_LAGS, WORK_MB = "MCMCPP_HIP_ESS_FIRST_LAGS", "MCMCPP_HIP_ESS_WORK_MB"


def make_series(spec):
    """the samples of a case, from its spec alone: those of tests/rhat_device.make_steps, then with spec["ar"] every series
    made an AR(1) series of that coefficient (per parameter where a list), with spec["ramp"] that slope a step added, with
    spec["alternating"] parameter 0 replaced by +1, -1, +1, ... plus a thousandth of its noise"""
    x = make_steps(spec)
    T = x.dtype.type
    K, n, W, P = x.shape
    if spec.get("ar") is not None:
        phi = np.broadcast_to(np.asarray(spec["ar"], dtype=np.float64), (P,)).astype(T)
        center = x.mean(axis=(1, 2), keepdims=True, dtype=np.float64).astype(T)
        z = x - center
        for s in range(1, n):
            z[:, s] = phi * z[:, s - 1] + z[:, s]
        x = z + center
    if spec.get("ramp"):
        x = x + (T(spec["ramp"]) * np.arange(n, dtype=T)).reshape(1, n, 1, 1)
    if spec.get("alternating"):
        x[..., 0] = (T(1) - T(2) * (np.arange(n) % 2).astype(T)).reshape(1, n, 1) + T(1e-3) * x[..., 0]
    return np.ascontiguousarray(x, dtype=T)


def run_case(name, spec, out, torch, capi):
    x = reshaped(spec, make_series(spec))
    sl, split = spec.get("slice", 1), bool(spec.get("split", 1))
    kw = dict(split=split, max_lag=spec.get("max_lag", 0), n_functions=spec.get("nf", 0), slice_interval=sl)
    for knob, key in ((FIRST_LAGS, "first_lags"), (WORK_MB, "work_mb")):
        if key in spec:
            os.environ[knob] = str(spec[key])  # read per call
        else:
            os.environ.pop(knob, None)

    def keep(prefix, got):
        for key in KEYS:
            out["%s/%s%s" % (name, prefix, key)] = got[key]
        out["%s/%sshape" % (name, prefix)] = np.array([got["sequence_length"], got["num_sequences"]])

    if spec.get("host", True):
        host = x
        if spec.get("scattered"):  # host steps that are not contiguous in memory: every step a row of a wider array, in reverse
            wide = np.zeros((x.shape[0], x.shape[1], 2) + x.shape[2:], x.dtype)
            wide[:, ::-1, 1] = x
            host = wide[:, ::-1, 1]
            assert not host.flags.c_contiguous and np.array_equal(host, x, equal_nan=True)
        keep("host_", capi.effective_sample_size(host, **kw))
    if spec.get("device", True):
        d = place_on_device(spec, x, torch)
        keep("dev_", capi.effective_sample_size(d[0] if spec.get("one_chain_3d") else d, **kw))
    os.environ.pop(FIRST_LAGS, None)
    os.environ.pop(WORK_MB, None)


def sampler_chain(out, torch, capi):
    """chains the sampler wrote into device memory: HipSampler(num_chains=3).run_device, 64 x 4 iso-Gaussian, 900 stored steps"""
    W, P, n, K = 64, 4, 900, 3
    pos = np.random.default_rng(5).standard_normal((K, W, P))
    s = capi.HipSampler(W, P, capi.CALC_ISO_GAUSSIAN, None, seed=3, num_chains=K)
    s.set_state(pos, s.calc_logp(pos).reshape(K, W))
    chain, _ = s.run_device(n)
    assert tuple(chain.shape) == (K, n, W, P)
    for tag, view in (("all", chain), ("burn", chain[:, 100:])):
        got = capi.effective_sample_size(view, n_functions=8)
        for key in KEYS:
            out["sampler/%s_%s" % (tag, key)] = got[key]
    out["sampler/chain"] = chain.cpu().numpy()


def errors(out, torch, capi):
    """the failures that need a device, through the C ABI itself so that the outputs can be watched"""
    import ctypes as C
    L = capi.lib()
    K, n, W, P = 3, 12, 10, 2
    x = make_steps(dict(dtype="f64", K=K, n=n, W=W, P=P, seed=11))
    outs = [np.full(P, 777.0), np.full(P, 777.0), np.full(P, 777, np.int64), np.full(P, 777, np.int64), np.full((P, 4), 777.0), np.full((P, 4), 777.0)] + \
           [np.full(P, 777.0) for _ in range(4)]
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    ptrs = [capi._ptr(a) for a in outs + shape]
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()

    def attempt(tag, device_steps, stride):
        rc = L.mcmcpp_hip_effective_sample_size_device(capi.F64, -1, C.c_void_p(device_steps), K, stride, n, 1, W, P, 1, 0, 4, *ptrs)
        out["errors/%s_code" % tag] = np.int32(rc)
        out["errors/%s_message" % tag] = np.array((L.mcmcpp_hip_effective_sample_size_last_error() or b"").decode())
        out["errors/%s_untouched" % tag] = np.int32(all((a == 777).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6)

    attempt("host_pointer", x.ctypes.data, 0)
    attempt("past_the_end", d.data_ptr(), 10 ** 7)  # chains so far apart that the last ends outside any allocation around the first
    # the next call succeeds
    got = capi.effective_sample_size(d, n_functions=4)
    out["errors/steps"] = x
    for key in KEYS:
        out["errors/after_" + key] = got[key]


def main():
    import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
    from mcmcpp_amd import capi
    spec = json.loads(sys.argv[1])
    out = {}
    out["cus"] = np.int64(torch.cuda.get_device_properties(0).multi_processor_count)
    for name, case in spec.get("cases", {}).items():
        run_case(name, case, out, torch, capi)
        print("case %s done" % name, flush=True)
    if spec.get("sampler"):
        sampler_chain(out, torch, capi)
    if spec.get("errors"):
        errors(out, torch, capi)
    np.savez(sys.argv[2], **out)
    print("ess_device OK")


if __name__ == "__main__":
    main()
