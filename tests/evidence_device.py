"""GPU side of tests/test_evidence.py, run in a child process under a time limit of its own:
    python -m tests.evidence_device '<json spec>' <out.npz>
One child runs every case of the spec (importing torch and opening the device costs more than the cases do) and writes, per
case, the log-posteriors the existing calc_logp(pos, chain=) returned for the case's draws and what the new call returned
through the host-pointer and the device entry points; the parent builds the same draws from the same spec (make_draws) and
compares with the restatement (tests/evidence_restatement.py) on those log-posteriors, bit for bit."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("log_ratio", "mcse", "ess", "kish", "max_u", "nonfinite", "log_ratio_total", "mcse_total")
KNOB = "MCMCPP_HIP_EVIDENCE_CHUNK_MB"
CALC = {"iso": 0, "dense": 1, "rosen": 2}
E_ARG, E_UNSUPPORTED, E_STATE = 1, 4, 5


def np_type(name):
    return np.float32 if name == "f32" else np.float64


def betas_of(spec):
    return spec.get("betas") or [0.75 ** k for k in range(spec["K"])]


def make_params(spec):
    """the ladder's parameter blocks [K][len] (None: a calculator without parameters): rung 0's target flattened by beta_k"""
    T, D = np_type(spec["dtype"]), spec["D"]
    if spec["calc"] == "dense":
        a = np.random.default_rng(100 + D).standard_normal((D, D))
        P = np.eye(D) if spec.get("identity") else a @ a.T / D + np.eye(D)
        return np.stack([(b * P).astype(T).ravel() for b in betas_of(spec)])
    if spec["calc"] == "rosen":
        return np.stack([np.array([1.0, 5.0, 0.5 * b], dtype=T) for b in betas_of(spec)])
    return None


def make_draws(spec):
    """the draws of a case, from its spec alone: [K][n_steps][W][D], Gaussian, rung k's wider by 1 / sqrt(beta_k); these do not come
    from the sampler.  spec["nan"]: a NaN coordinate in one draw of rung 1.  spec["overflow"]: one draw of rung 1 so far out that
    its quadratic form overflows under rung 0's matrix and not under rung 1's."""
    T = np_type(spec["dtype"])
    K, n, W, D = spec["K"], spec["n"], spec["W"], spec["D"]
    rng = np.random.default_rng(spec.get("seed", 1))
    x = rng.standard_normal((K, n, W, D))
    x /= np.sqrt(np.array(betas_of(spec))).reshape(K, 1, 1, 1)
    if spec["calc"] == "rosen":
        x = 1.0 + 0.5 * x
    x = x.astype(T)
    if spec.get("nan"):
        x[1, n // 2, W // 3, D - 1] = np.nan
    if spec.get("overflow"):
        x[1, n // 3, 1, :] = T(1.5e19)
    return x


def place_on_device(spec, x, torch):
    """the device tensor the case reads: as it is ("exact", the default); its chains more than n steps apart, one step inside a
    larger allocation ("room"); or behind a burn-in of spec["burn"] steps ("burn")"""
    t = torch.from_numpy(x)
    how = spec.get("place", "exact")
    if how == "exact":
        return t.cuda()
    K, n = x.shape[:2]
    lead = spec["burn"] if how == "burn" else 1
    room = torch.full((K, lead + n + 2) + x.shape[2:], 1.0e30, dtype=t.dtype, device="cuda")
    room[:, lead:lead + n] = t.cuda()
    d = room[:, lead:lead + n]
    assert d.data_ptr() != room.data_ptr() and d.stride(0) > n * x.shape[2] * x.shape[3]
    return d


def make_handle(spec, capi, **kw):
    dtype = capi.F32 if spec["dtype"] == "f32" else capi.F64
    return capi.HipSampler(spec["W"], spec["D"], CALC[spec["calc"]], make_params(spec), seed=3, dtype=dtype, num_chains=spec["K"], **kw)


def log_posteriors(s, x):
    """own, lower, upper [K][n][W] through the existing calc_logp(pos, chain=)"""
    K, n, W, _ = x.shape
    own, lower, upper = (np.zeros((K, n, W), x.dtype) for _ in range(3))
    for k in range(K):
        own[k] = s.calc_logp(x[k], chain=k).reshape(n, W)
        if k > 0:
            lower[k] = s.calc_logp(x[k], chain=k - 1).reshape(n, W)
        if k + 1 < K:
            upper[k] = s.calc_logp(x[k], chain=k + 1).reshape(n, W)
    return own, lower, upper


def run_case(name, spec, out, torch, capi):
    x = make_draws(spec)
    sl = spec.get("slice", 1)
    s = make_handle(spec, capi)
    own, lower, upper = log_posteriors(s, x)
    for key, v in (("own", own), ("lower", lower), ("upper", upper)):
        out["%s/logp_%s" % (name, key)] = v
    if "chunk_mb" in spec:
        os.environ[KNOB] = str(spec["chunk_mb"])  # read per call
    else:
        os.environ.pop(KNOB, None)
    if spec.get("host", True):
        got = s.evidence_ratios(x, slice_interval=sl)
        for key in KEYS:
            out["%s/host_%s" % (name, key)] = got[key]
        out[name + "/host_num_draws"] = np.int64(got["num_draws"])
    if spec.get("device", True):
        d = place_on_device(spec, x, torch)
        got = s.evidence_ratios(d, slice_interval=sl)
        for key in KEYS:
            out["%s/dev_%s" % (name, key)] = got[key]
        out[name + "/dev_num_draws"] = np.int64(got["num_draws"])
    os.environ.pop(KNOB, None)
    s.close()


def end_to_end(spec, out, torch, capi):
    """run_tempered(device=True), then evidence_ratios on the returned tensor, on a view behind a burn-in, and on its download"""
    K, W, D, n = spec["K"], spec["W"], spec["D"], spec["n"]
    s = make_handle(spec, capi)
    pos = np.random.default_rng(5).standard_normal((K, W, D))
    s.set_state(pos, np.stack([s.calc_logp(pos[k], chain=k) for k in range(K)]))
    chain, _, swaps, _ = s.run_tempered(n, interval=1, exchange_every=2, device=True)
    assert tuple(chain.shape) == (K, n, W, D)
    before = s.get_state(), s.counters()
    x = chain.cpu().numpy()
    for tag, view, host in (("all", chain, x), ("burn", chain[:, spec["burn"]:], x[:, spec["burn"]:])):
        for how, steps in (("dev", view), ("host", host)):
            got = s.evidence_ratios(steps)
            for key in KEYS:
                out["e2e/%s_%s_%s" % (tag, how, key)] = got[key]
            out["e2e/%s_%s_num_draws" % (tag, how)] = np.int64(got["num_draws"])
    after = s.get_state(), s.counters()
    out["e2e/state_untouched"] = np.int32(all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1] == after[1])
    own, lower, upper = log_posteriors(s, x)
    for key, v in (("own", own), ("lower", lower), ("upper", upper)):
        out["e2e/logp_" + key] = v
    out["e2e/accepted"] = swaps["accepted"]
    s.close()


def refusals(out, torch, capi):
    """every refusal, through the C ABI itself so that the outputs can be watched"""
    import ctypes as C
    L = capi.lib()
    spec = dict(dtype="f64", calc="dense", K=2, n=6, W=10, D=4, betas=[1.0, 0.5])
    K, n, W, D = 2, 6, 10, 4
    x = make_draws(spec)
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    P = make_params(spec)
    outs = [np.full((2, K - 1), 777.0) for _ in range(5)] + [np.full((2, K - 1), -7, np.int64)] + [np.full(2, 777.0) for _ in range(2)] + [np.full(1, -5, np.int64)]
    ptrs = [capi._ptr(a) for a in outs]
    host_ptrs = (C.c_void_p * (K * n))(*[x[k, s].ctypes.data for k in range(K) for s in range(n)])

    def untouched():
        return all((a == 777.0).all() for a in outs[:5] + outs[6:8]) and (outs[5] == -7).all() and outs[8][0] == -5

    def attempt(tag, s, device=True, steps="own", stride=0, n_steps=n, sl=1):
        if device:
            rc = L.mcmcpp_hip_evidence_ratios_device(s.h, C.c_void_p(d.data_ptr() if steps == "own" else steps), stride, n_steps, sl, *ptrs)
        else:
            rc = L.mcmcpp_hip_evidence_ratios(s.h, host_ptrs if steps == "own" else steps, n_steps, sl, *ptrs)
        out["refusals/%s_code" % tag] = np.int32(rc)
        out["refusals/%s_message" % tag] = np.array((L.mcmcpp_hip_last_error(s.h) or b"").decode())
        out["refusals/%s_untouched" % tag] = np.int32(untouched())

    ladder = capi.HipSampler(W, D, 1, P, num_chains=K)
    for device in (True, False):
        t = "dev" if device else "host"
        attempt("de_" + t, capi.HipSampler(512, D, 1, P[0], mover=capi.MOVER_DIFFERENTIAL_EVOLUTION), device)
        attempt("batch_" + t, capi.HipSampler(512, D, capi.CALC_BATCH, None, batch_callback=(capi.BATCH_LOGP_FN(lambda *a: 0), None)), device)
        attempt("sharded_" + t, capi.HipSampler(512, D, 1, P[0], shard_begin=0, shard_count=128), device)
        attempt("communicator_" + t, capi.HipSampler(512, D, 1, P[0], comm_world=1, comm_rank=0, comm_id=capi.comm_unique_id()), device)
        buf = torch.zeros((512, D), dtype=torch.float64, device="cuda")
        attempt("owned_" + t, capi.HipSampler(512, D, 1, P[0], device_positions=buf.data_ptr()), device)
        attempt("one_chain_" + t, capi.HipSampler(W, D, 1, P[0]), device)
        attempt("three_steps_" + t, ladder, device, n_steps=3)
        attempt("three_used_steps_" + t, ladder, device, sl=2)  # 6 steps, every second
        attempt("slice_" + t, ladder, device, sl=0)
        attempt("null_" + t, ladder, device, steps=None)
    host_ptrs_hole = (C.c_void_p * (K * n))(*[x[k, s].ctypes.data if (k, s) != (1, 2) else None for k in range(K) for s in range(n)])
    attempt("null_step_host", ladder, False, steps=host_ptrs_hole)
    attempt("stride_dev", ladder, True, stride=n - 1)
    attempt("host_pointer_dev", ladder, True, steps=x.ctypes.data)
    attempt("past_the_end_dev", ladder, True, stride=10 ** 7)  # chains so far apart that the last ends outside the allocation of the first
    # while an asynchronous run is in progress
    busy = capi.HipSampler(512, D, 1, P[0])
    pos = np.random.default_rng(2).standard_normal((512, D))
    busy.set_state(pos, busy.calc_logp(pos))
    busy.run_async(200)
    attempt("async_dev", busy, True)
    attempt("async_host", busy, False)
    busy.run_wait()
    # the next call succeeds, without set_state
    got = ladder.evidence_ratios(d)
    out["refusals/steps"] = x
    own, lower, upper = log_posteriors(ladder, x)
    for key, v in (("own", own), ("lower", lower), ("upper", upper)):
        out["refusals/logp_" + key] = v
    for key in KEYS:
        out["refusals/after_" + key] = got[key]


def main():
    import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
    from mcmcpp_amd import capi
    spec = json.loads(sys.argv[1])
    out = {}
    for name, case in spec.get("cases", {}).items():
        run_case(name, case, out, torch, capi)
        print("case %s done" % name, flush=True)
    if spec.get("e2e"):
        end_to_end(spec["e2e"], out, torch, capi)
        print("end to end done", flush=True)
    if spec.get("refusals"):
        refusals(out, torch, capi)
    np.savez(sys.argv[2], **out)
    print("evidence_device OK")


if __name__ == "__main__":
    main()
