"""GPU side of tests/test_summary.py, run in a child process under a time limit of its own:
    python -m tests.summary_device '<json spec>' <out.npz>
One child runs every case of the spec and writes, per case, what capi.posterior_summary returned through the host-pointer and
the device entry points, and what the existing entry points (capi.effective_sample_size, capi.quantiles) return on the same
draws; the parent builds the same draws from the same spec (tests/rank_device.make_draws) and compares with the restatement
(tests/summary_restatement.py) bit for bit.  A HIP error ends the child at once: capi raises, nothing catches it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import rank_restatement as rk  # noqa: E402
from tests.rank_device import CHUNK_MB, WORK_MB, host_view, make_draws  # noqa: E402
from tests.rhat_device import make_steps, place_on_device  # noqa: E402

KEYS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_sd", "mcse_sd", "quantile", "ess_quantile", "mcse_quantile", "rank_lower", "rank_upper", "hdi_lower", "hdi_upper")
DEFAULT_PROBS = (0.05, 0.5, 0.95)
KEEP_MB = "MCMCPP_HIP_SUMMARY_KEEP_MB"


def case_arguments(spec, S):
    """(probs, hdi_prob) of a case: spec["probs"] (default 0.05, 0.5, 0.95); spec["hdi_m"] = m asks for the hdi_prob in the
    middle of those whose floor(hdi_prob S) is m, spec["hdi"] names it (default 0.94)"""
    hdi = (spec["hdi_m"] + 0.5) / S if "hdi_m" in spec else spec.get("hdi", 0.94)
    return list(spec.get("probs", DEFAULT_PROBS)), hdi


def run_case(name, spec, out, torch, capi):
    x = make_draws(spec)
    sl, split = spec.get("slice", 1), bool(spec.get("split", 1))
    ranked = rk.draws(x, split, sl)
    probs, hdi = case_arguments(spec, ranked[..., 0].size)
    for knob, key in ((WORK_MB, "work_mb"), (CHUNK_MB, "chunk_mb"), (KEEP_MB, "keep_mb")):
        if key in spec:
            os.environ[knob] = str(spec[key])  # read per call
        else:
            os.environ.pop(knob, None)
    d = place_on_device(spec, x, torch)
    for prefix, src in (("host_", host_view(spec, x)), ("dev_", d[0] if spec.get("one_chain_3d") else d)):
        got = capi.posterior_summary(src, probs=probs, hdi_prob=hdi, split=split, max_lag=spec.get("max_lag", 0), slice_interval=sl)
        for key in KEYS:
            out["%s/%s%s" % (name, prefix, key)] = got[key]
        out["%s/%sshape" % (name, prefix)] = np.array([got["sequence_length"], got["num_sequences"]])
    # the existing entry points on the same input
    ess = capi.effective_sample_size(d[0] if spec.get("one_chain_3d") else d, split=split, max_lag=spec.get("max_lag", 0), slice_interval=sl)
    out[name + "/ess_mean"], out[name + "/ess_ess"] = ess["mean"], ess["ess"]
    if probs:  # capi.quantiles on the same draws, as one chain of K H L steps (in the chain's type)
        out[name + "/quantiles"] = capi.quantiles(torch.from_numpy(ranked.reshape((-1,) + ranked.shape[2:])).cuda(), probs)
    for knob in (WORK_MB, CHUNK_MB, KEEP_MB):
        os.environ.pop(knob, None)


def sampler_chain(out, torch, capi):
    """chains the sampler wrote into device memory: HipSampler(num_chains=3).run_device, 64 x 4 iso-Gaussian, 900 stored steps,
    stretch scale 6 (three draws in four repeat the one before), summarised behind a burn-in of 100 steps"""
    W, P, n, K = 64, 4, 900, 3
    pos = np.random.default_rng(5).standard_normal((K, W, P))
    s = capi.HipSampler(W, P, capi.CALC_ISO_GAUSSIAN, None, seed=3, num_chains=K, alpha=(6, 1))
    s.set_state(pos, s.calc_logp(pos).reshape(K, W))
    chain, _ = s.run_device(n)
    assert tuple(chain.shape) == (K, n, W, P)
    dev = capi.posterior_summary(chain[:, 100:])
    host = capi.posterior_summary(chain[:, 100:].cpu().numpy())
    for key in KEYS:
        out["sampler/dev_" + key], out["sampler/host_" + key] = dev[key], host[key]
    out["sampler/chain"] = chain.cpu().numpy()


def errors(out, torch, capi):
    """the failures that need a device, through the C ABI itself so that the outputs can be watched; a call that succeeds
    follows each"""
    import ctypes as C
    L = capi.lib()
    K, n, W, P, Q = 3, 12, 10, 2, 3
    x = make_steps(dict(dtype="f64", K=K, n=n, W=W, P=P, seed=11))
    bad = x.copy()
    bad[1, 7, 3, 1] = np.nan
    d, d_bad = torch.from_numpy(x).cuda(), torch.from_numpy(bad).cuda()
    probs = np.array(DEFAULT_PROBS)
    outs = [np.full(P, 777.0) for _ in range(6)] + [np.full((P, Q), 777.0) for _ in range(3)] + [np.full((P, Q), 777, np.int64) for _ in range(2)] + \
           [np.full(P, 777.0) for _ in range(2)]
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    ptrs = [capi._ptr(a) for a in outs + shape]
    torch.cuda.synchronize()

    def attempt(tag, device_steps):
        rc = L.mcmcpp_hip_posterior_summary_device(capi.F64, -1, C.c_void_p(device_steps), K, 0, n, 1, W, P, 1, 0, capi._ptr(probs), Q, 0.94, *ptrs)
        out["errors/%s_code" % tag] = np.int32(rc)
        out["errors/%s_message" % tag] = np.array((L.mcmcpp_hip_posterior_summary_last_error() or b"").decode())
        out["errors/%s_untouched" % tag] = np.int32(all((a == 777).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6)
        good = capi.posterior_summary(d)  # the next call succeeds
        for key in KEYS:
            out["errors/after_%s_%s" % (tag, key)] = good[key]

    attempt("nan_draw", d_bad.data_ptr())
    attempt("host_pointer", x.ctypes.data)
    # the host form refuses the NaN too
    host_ptrs = (C.c_void_p * (K * n))(*[bad[k, s].ctypes.data for k in range(K) for s in range(n)])
    rc = L.mcmcpp_hip_posterior_summary(capi.F64, -1, host_ptrs, K, n, W, P, 1, 0, capi._ptr(probs), Q, 0.94, *ptrs)
    out["errors/nan_draw_host_code"] = np.int32(rc)
    out["errors/nan_draw_host_message"] = np.array((L.mcmcpp_hip_posterior_summary_last_error() or b"").decode())
    out["errors/nan_draw_host_untouched"] = np.int32(all((a == 777).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6)
    out["errors/steps"] = x


def error_slots(out, torch, capi):
    """tests/test_analysis_errors.py: what the ESS and the R-hat family's *_last_error say after a failure of their own, before
    and after a summary and rank diagnostics that succeed and a summary that fails.  Those calls run the two families' code on
    chains of their own and have a message slot of their own.  (None of these calls fails inside the nested ESS or R-hat
    code -- the NaN is refused by the summary's own check -- so this would not see a nested failure's message written to the
    other family's slot; that rank.hip and summary.hip reference no symbol of the two families' C ABI is what rules it out.)"""
    import ctypes as C
    L = capi.lib()
    K, n, W, P = 3, 12, 10, 2
    x = make_steps(dict(dtype="f64", K=K, n=n, W=W, P=P, seed=11))
    bad = x.copy()
    bad[1, 7, 3, 1] = np.nan
    d, d_bad = torch.from_numpy(x).cuda(), torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()

    def slots(tag):
        out["slots/%s_ess" % tag] = np.array((L.mcmcpp_hip_effective_sample_size_last_error() or b"").decode())
        out["slots/%s_rhat" % tag] = np.array((L.mcmcpp_hip_gelman_rubin_last_error() or b"").decode())

    host = C.c_void_p(x.ctypes.data)  # a host pointer as device_steps
    out["slots/ess_code"] = np.int32(L.mcmcpp_hip_effective_sample_size_device(capi.F64, -1, host, K, 0, n, 1, W, P, 1, 0, 0, *([None] * 12)))
    out["slots/rhat_code"] = np.int32(L.mcmcpp_hip_gelman_rubin_device(capi.F64, -1, host, K, 0, n, 1, W, P, 1, *([None] * 10)))
    slots("first")
    summary, diag = capi.posterior_summary(d), capi.rank_diagnostics(d)
    out["slots/ess_mean"], out["slots/ess_bulk"] = summary["ess_mean"], diag["ess_bulk"]
    slots("after_success")
    probs = np.array(DEFAULT_PROBS)
    out["slots/nan_code"] = np.int32(L.mcmcpp_hip_posterior_summary_device(capi.F64, -1, C.c_void_p(d_bad.data_ptr()), K, 0, n, 1, W, P, 1, 0, capi._ptr(probs), 3, 0.94,
                                                                         *([None] * 15)))
    out["slots/nan_message"] = np.array((L.mcmcpp_hip_posterior_summary_last_error() or b"").decode())
    slots("after_failure")


def main():
    import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
    from mcmcpp_amd import capi
    spec = json.loads(sys.argv[1])
    out = {}
    for name, case in spec.get("cases", {}).items():
        run_case(name, case, out, torch, capi)
        print("case %s done" % name, flush=True)
    if spec.get("sampler"):
        sampler_chain(out, torch, capi)
        print("sampler done", flush=True)
    if spec.get("errors"):
        errors(out, torch, capi)
    if spec.get("error_slots"):
        error_slots(out, torch, capi)
    np.savez(sys.argv[2], **out)
    print("summary_device OK")


if __name__ == "__main__":
    main()
