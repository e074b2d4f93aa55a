"""GPU side of tests/test_evidence_mbar.py, run in a child process under a time limit of its own:
    python -m tests.mbar_device '<json spec>' <out.npz>
One child runs every case of the spec and writes, per case, the log-posteriors the existing calc_logp(pos, chain=k) returned for
the draws of every rung under every chain's parameters, [K chains][K rungs][n][W], and what evidence_mbar returned through the
host-pointer and the device entry points; the parent compares with the restatement (tests/mbar_restatement.py) on those
log-posteriors, bit for bit.  The draws, ladders and placements are those of tests/evidence_device.py."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import evidence_device as ed  # noqa: E402

KEYS = ("log_z", "cov", "log_ratio", "mcse", "ess", "nonfinite", "log_ratio_total", "mcse_total", "passes", "converged")
BRIDGE_KEYS = ("log_ratio", "mcse", "overlap", "ess", "passes", "converged", "nonfinite", "log_ratio_total", "mcse_total")


def log_posteriors(s, x):
    """[K chains][K rungs][n][W] through the existing calc_logp(pos, chain=)"""
    K, n, W, _ = x.shape
    return np.stack([np.stack([s.calc_logp(x[r], chain=k).reshape(n, W) for r in range(K)]) for k in range(K)])


def store(out, prefix, got):
    for key in KEYS:
        out["%s_%s" % (prefix, key)] = np.asarray(got[key])
    out[prefix + "_num_draws"] = np.int64(got["num_draws"])


def run_case(name, spec, out, torch, capi):
    x = ed.make_draws(spec)
    sl = spec.get("slice", 1)
    s = ed.make_handle(spec, capi)
    out[name + "/logp"] = log_posteriors(s, x)
    if "chunk_mb" in spec:
        os.environ[ed.KNOB] = str(spec["chunk_mb"])  # read per call
    else:
        os.environ.pop(ed.KNOB, None)
    if spec.get("host", True):
        store(out, name + "/host", s.evidence_mbar(x, slice_interval=sl))
    if spec.get("device", True):
        store(out, name + "/dev", s.evidence_mbar(ed.place_on_device(spec, x, torch), slice_interval=sl))
    os.environ.pop(ed.KNOB, None)
    s.close()


def end_to_end(spec, out, torch, capi):
    """run_tempered(device=True), then evidence_mbar on the returned tensor in place and behind a burn-in, and evidence_bridge"""
    K, W, D, n = spec["K"], spec["W"], spec["D"], spec["n"]
    s = ed.make_handle(spec, capi)
    pos = np.random.default_rng(5).standard_normal((K, W, D))
    s.set_state(pos, np.stack([s.calc_logp(pos[k], chain=k) for k in range(K)]))
    chain, _, swaps, _ = s.run_tempered(n, interval=1, exchange_every=2, device=True)
    assert tuple(chain.shape) == (K, n, W, D)
    before = s.get_state(), s.counters()
    store(out, "e2e/dev", s.evidence_mbar(chain))
    store(out, "e2e/burn", s.evidence_mbar(chain[:, spec["burn"]:]))
    bridge = s.evidence_bridge(chain)
    for key in BRIDGE_KEYS:
        out["e2e/bridge_" + key] = np.asarray(bridge[key])
    after = s.get_state(), s.counters()
    out["e2e/state_untouched"] = np.int32(all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1] == after[1])
    out["e2e/logp"] = log_posteriors(s, chain.cpu().numpy())
    out["e2e/accepted"] = swaps["accepted"]
    s.close()


def refusals(out, torch, capi):
    """every refusal of evidence_ratios, through the C ABI itself so that the outputs can be watched"""
    import ctypes as C
    L = capi.lib()
    spec = dict(dtype="f64", calc="dense", K=2, n=6, W=10, D=4, betas=[1.0, 0.5])
    K, n, W, D = 2, 6, 10, 4
    x = ed.make_draws(spec)
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    P = ed.make_params(spec)
    # log_z [K], cov [K][K], log_ratio, mcse [K-1], ess [K]; nonfinite [K][K]; the totals; passes, converged, num_draws
    outs = [np.full(K, 777.0), np.full((K, K), 777.0), np.full(K - 1, 777.0), np.full(K - 1, 777.0), np.full(K, 777.0), np.full((K, K), -7, np.int64)] + \
           [np.full(1, 777.0) for _ in range(2)] + [np.full(1, -7, np.int64) for _ in range(3)]
    ptrs = [capi._ptr(a) for a in outs]
    host_ptrs = (C.c_void_p * (K * n))(*[x[k, s].ctypes.data for k in range(K) for s in range(n)])

    def untouched():
        return all((a == (777.0 if a.dtype == np.float64 else -7)).all() for a in outs)

    def attempt(tag, s, device=True, steps="own", stride=0, n_steps=n, sl=1):
        if device:
            rc = L.mcmcpp_hip_evidence_mbar_device(s.h, C.c_void_p(d.data_ptr() if steps == "own" else steps), stride, n_steps, sl, *ptrs)
        else:
            rc = L.mcmcpp_hip_evidence_mbar(s.h, host_ptrs if steps == "own" else steps, n_steps, sl, *ptrs)
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
    # the next call succeeds, without set_state; and with every output NULL
    store(out, "refusals/after", ladder.evidence_mbar(d))
    out["refusals/all_null_code"] = np.int32(L.mcmcpp_hip_evidence_mbar_device(ladder.h, C.c_void_p(d.data_ptr()), 0, n, 1, *([None] * 11)))
    out["refusals/logp"] = log_posteriors(ladder, x)


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
    print("mbar_device OK")


if __name__ == "__main__":
    main()
