"""GPU side of tests/test_rhat.py, run in a child process under a time limit of its own:
    python -m tests.rhat_device '<json spec>' <out.npz>
One child runs every case of the spec (importing torch and opening the device costs more than the cases do) and writes, per
case, what the library returned through the host-pointer and the device entry points; the parent builds the same samples from
the same spec (make_steps) and compares with the restatement (tests/rhat_restatement.py) bit for bit."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("rhat", "mean", "within", "between", "chain_mean", "chain_within", "sequence_mean", "sequence_m2")
KNOB = "MCMCPP_HIP_RHAT_CHUNK_MB"
PLAN_CUS = "MCMCPP_HIP_RHAT_PLAN_CUS"  # plan as for a device of that many CUs: which lanes own whole sequences, and no result


def np_type(name):
    return np.float32 if name == "f32" else np.float64


def make_steps(spec):
    """the samples of a case, from its spec alone: [K][n][W][P], Gaussian columns of different scales around spec["offset"],
    chain k shifted by k * spec["chain_shift"]; with spec["nonfinite"] one inf and one NaN sample; with spec["constant"] the last
    column constant"""
    T = np_type(spec["dtype"])
    K, n, W, P = spec["K"], spec["n"], spec["W"], spec["P"]
    rng = np.random.default_rng(spec.get("seed", 1))
    x = rng.standard_normal((K, n, W, P), dtype=T)
    x *= rng.uniform(0.2, 4.0, P).astype(T)
    x += (rng.uniform(-3, 3, P) + spec.get("offset", 0.0)).astype(T)
    if spec.get("chain_shift"):
        x += (np.arange(K) * spec["chain_shift"]).astype(T).reshape(K, 1, 1, 1)
    if spec.get("nonfinite"):
        x[0, n // 3, W // 2, 0] = np.inf
        x[K - 1, n - 2, 1, P - 1] = np.nan
    if spec.get("constant"):
        x[..., P - 1] = T(2.5)
    return x


def reshaped(spec, x):
    """the same bytes seen as another shape (spec["view"] = [K, n, W, P])"""
    return x.reshape(spec["view"]) if "view" in spec else x


def place_on_device(spec, x, torch):
    """the device tensor the case reads: its chains more than n steps apart and one step inside a larger allocation ("room",
    the default); behind a burn-in of spec["burn"] steps in a [K][n_saved][W][P] array; from a base that is 8 bytes off a
    16-byte boundary ("base8"); as chain[:, burn:] of a contiguous [K][burn + n][W][P] tensor, which the last chain ends ("tail");
    or as it is ("exact")"""
    t = torch.from_numpy(x)
    how = spec.get("place", "room")
    K, n = x.shape[:2]
    if how == "exact":
        return t.cuda()
    if how == "tail":
        whole = torch.full((K, spec["burn"] + n) + x.shape[2:], 1.0e30, dtype=t.dtype, device="cuda")
        whole[:, spec["burn"]:] = t.cuda()
        d = whole[:, spec["burn"]:]
        assert whole.is_contiguous() and d.stride(0) == (spec["burn"] + n) * x.shape[2] * x.shape[3]
        return d
    if how == "base8":
        flat = torch.zeros(x.size + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.reshape(-1).cuda()
        d = flat[1:].view(x.shape)
        assert d.data_ptr() % 16 == 8
        return d
    lead = spec["burn"] if how == "burn" else 1
    room = torch.full((K, lead + n + 1) + x.shape[2:], 1.0e30, dtype=t.dtype, device="cuda")
    room[:, lead:lead + n] = t.cuda()
    d = room[:, lead:lead + n]
    assert d.data_ptr() != room.data_ptr() and d.stride(0) > n * x.shape[2] * x.shape[3]
    return d


def run_case(name, spec, out, torch, capi):
    x = reshaped(spec, make_steps(spec))
    sl, split = spec.get("slice", 1), bool(spec.get("split", 1))
    if "chunk_mb" in spec:
        os.environ[KNOB] = str(spec["chunk_mb"])  # read per call
    else:
        os.environ.pop(KNOB, None)
    if "plan_cus" in spec:
        os.environ[PLAN_CUS] = str(spec["plan_cus"])
    else:
        os.environ.pop(PLAN_CUS, None)
    if spec.get("host", True):
        host = x
        if spec.get("scattered"):  # host steps that are not contiguous in memory: every step a row of a wider array, in reverse
            wide = np.zeros((x.shape[0], x.shape[1], 2) + x.shape[2:], x.dtype)
            wide[:, ::-1, 1] = x
            host = wide[:, ::-1, 1]
            assert not host.flags.c_contiguous and np.array_equal(host, x)
        got = capi.gelman_rubin(host, split=split, slice_interval=sl, want_sequences=True)
        for key in KEYS:
            out["%s/host_%s" % (name, key)] = got[key]
        out[name + "/host_shape"] = np.array([got["sequence_length"], got["num_sequences"]])
    os.environ.pop(KNOB, None)
    if spec.get("device", True):
        d = place_on_device(spec, x, torch)
        got = capi.gelman_rubin(d[0] if spec.get("one_chain_3d") else d, split=split, slice_interval=sl, want_sequences=True)
        for key in KEYS:
            out["%s/dev_%s" % (name, key)] = got[key]
        out[name + "/dev_shape"] = np.array([got["sequence_length"], got["num_sequences"]])
    os.environ.pop(PLAN_CUS, None)


def sampler_chain(out, torch, capi):
    """chains the sampler wrote into device memory: HipSampler(num_chains=3).run_device, 64 x 4 iso-Gaussian, 900 stored steps"""
    W, P, n, K = 64, 4, 900, 3
    pos = np.random.default_rng(5).standard_normal((K, W, P))
    s = capi.HipSampler(W, P, capi.CALC_ISO_GAUSSIAN, None, seed=3, num_chains=K)
    s.set_state(pos, s.calc_logp(pos).reshape(K, W))
    chain, _ = s.run_device(n)
    assert tuple(chain.shape) == (K, n, W, P)
    for tag, view in (("all", chain), ("burn", chain[:, 100:])):
        got = capi.gelman_rubin(view, want_sequences=True)
        for key in KEYS:
            out["sampler/%s_%s" % (tag, key)] = got[key]
    out["sampler/chain"] = chain.cpu().numpy()


def errors(out, torch, capi):
    """the failures that need a device, through the C ABI itself so that the outputs can be watched"""
    import ctypes as C
    L = capi.lib()
    K, n, W, P = 3, 12, 10, 2
    x = make_steps(dict(dtype="f64", K=K, n=n, W=W, P=P, seed=11))
    outs = [np.full(P, 777.0) for _ in range(4)] + [np.full((K, P), 777.0) for _ in range(2)] + [np.full((K * 2 * W, P), 777.0) for _ in range(2)]
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    ptrs = [capi._ptr(a) for a in outs + shape]
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()

    def attempt(tag, device_steps, stride):
        rc = L.mcmcpp_hip_gelman_rubin_device(capi.F64, -1, C.c_void_p(device_steps), K, stride, n, 1, W, P, 1, *ptrs)
        out["errors/%s_code" % tag] = np.int32(rc)
        out["errors/%s_message" % tag] = np.array((L.mcmcpp_hip_gelman_rubin_last_error() or b"").decode())
        out["errors/%s_untouched" % tag] = np.int32(all((a == 777.0).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6)

    attempt("host_pointer", x.ctypes.data, 0)
    attempt("past_the_end", d.data_ptr(), 10 ** 7)  # chains so far apart that the last ends outside any allocation around the first
    # the next call succeeds
    got = capi.gelman_rubin(d, want_sequences=True)
    out["errors/steps"] = x
    for key in KEYS:
        out["errors/after_" + key] = got[key]


def main():
    import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
    from mcmcpp_amd import capi
    spec = json.loads(sys.argv[1])
    out = {}
    prop = torch.cuda.get_device_properties(0)
    out["cus"] = np.int64(prop.multi_processor_count)
    for name, case in spec.get("cases", {}).items():
        run_case(name, case, out, torch, capi)
        print("case %s done" % name, flush=True)
    if spec.get("sampler"):
        sampler_chain(out, torch, capi)
    if spec.get("errors"):
        errors(out, torch, capi)
    np.savez(sys.argv[2], **out)
    print("rhat_device OK")


if __name__ == "__main__":
    main()
