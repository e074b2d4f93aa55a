"""GPU side of tests/test_evidence_gaussian.py, run in a child process under a time limit of its own:
    python -m tests.gaussian_bridge_device '<json spec>' <out.npz>
One child runs every case of the spec and writes, per case, what evidence_gaussian returned through the host-pointer and the
device entry points -- the proposals and log q included -- and the log-posteriors the existing calc_logp(pos, chain=) returned
for the case's draws and for the returned proposals; the parent builds the same draws and the same Gaussian from the same spec
and compares with the restatement (tests/gaussian_bridge_restatement.py), bit for bit."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import evidence_device as ed  # noqa: E402

KEYS = ("log_evidence", "mcse", "overlap", "ess", "passes", "converged", "nonfinite", "log_q", "proposals")
KNOB = ed.KNOB
E_ARG, E_UNSUPPORTED, E_STATE = ed.E_ARG, ed.E_UNSUPPORTED, ed.E_STATE


def make_gaussian(spec):
    """the case's Gaussian from its spec alone: a mean near the draws' and a full lower factor (spec["scale"]: its size); what lies
    above the diagonal must not be read, so it is NaN"""
    D = spec["D"]
    rng = np.random.default_rng(200 + D + spec.get("seed", 1))
    L = np.tril(rng.standard_normal((D, D))) * (0.1 / np.sqrt(D))
    L[np.diag_indices(D)] = 0.8 + 0.4 * rng.random(D)
    L *= spec.get("scale", 1.0) * (0.5 if spec["calc"] == "rosen" else 1.0)
    L[np.triu_indices(D, 1)] = np.nan
    mean = 0.1 * rng.standard_normal(D) + (1.0 if spec["calc"] == "rosen" else 0.0)
    return mean, L


def make_draws(spec):
    """[n_steps][W][D] of the chain the case bridges: ed.make_draws' draws of rung spec["chain"]"""
    return ed.make_draws(spec)[spec.get("chain", 0)]


def place_on_device(spec, y, torch):
    """the device tensor the case reads: as it is, or a view behind spec["burn"] steps of a larger allocation ("burn"), or one step
    inside a larger allocation with room behind it ("room")"""
    t = torch.from_numpy(y)
    how = spec.get("place", "exact")
    if how == "exact":
        return t.cuda()
    lead = spec["burn"] if how == "burn" else 1
    room = torch.full((lead + y.shape[0] + 2,) + y.shape[1:], 1.0e30, dtype=t.dtype, device="cuda")
    room[lead:lead + y.shape[0]] = t.cuda()
    return room[lead:lead + y.shape[0]]


def store(out, prefix, got):
    for key in KEYS:
        out["%s_%s" % (prefix, key)] = np.asarray(got[key])
    out[prefix + "_num_draws"] = np.int64(got["num_draws"])


def dense_callback(dense, capi):
    """a batch callback that returns the dense handle's bits: its calc_logp_device on the rows it is handed"""
    L = capi.lib()
    return capi.BATCH_LOGP_FN(lambda user, rows, logp_out, count, D, stream: L.mcmcpp_hip_calc_logp_device(dense.h, 0, rows, count, logp_out))


def make_handle(spec, capi, keep):
    kind = spec.get("handle", "stretch")
    if kind == "stretch":
        return ed.make_handle(spec, capi)
    P = ed.make_params(spec)[0]
    dtype = capi.F32 if spec["dtype"] == "f32" else capi.F64
    if kind == "de":
        return capi.HipSampler(spec["W"], spec["D"], ed.CALC[spec["calc"]], P, seed=3, dtype=dtype, mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    dense = capi.HipSampler(spec["W"], spec["D"], ed.CALC[spec["calc"]], P, seed=3, dtype=dtype)
    cb = dense_callback(dense, capi)
    keep += [dense, cb]
    return capi.HipSampler(spec["W"], spec["D"], capi.CALC_BATCH, None, dtype=dtype, batch_callback=(cb, None))


def run_case(name, spec, out, torch, capi):
    y = make_draws(spec)
    mean, chol = make_gaussian(spec)
    sl, chain = spec.get("slice", 1), spec.get("chain", 0)
    keep = []
    s = make_handle(spec, capi, keep)
    # (the log-posteriors the restatement takes: the stretch handle's calc_logp with the chain's parameters)
    ref = s if spec.get("handle", "stretch") == "stretch" else ed.make_handle(spec, capi)
    if "chunk_mb" in spec:
        os.environ[KNOB] = str(spec["chunk_mb"])  # read per call
    else:
        os.environ.pop(KNOB, None)
    args = dict(chain=chain, mean=mean, chol=chol, slice_interval=sl, seed=spec.get("pseed", 9), stream=spec.get("pstream", 4), want_proposals=True)
    got = None
    if spec.get("host", True):
        got = s.evidence_gaussian(y, **args)
        store(out, name + "/host", got)
    if spec.get("device", True):
        got = s.evidence_gaussian(place_on_device(spec, y, torch), **args)
        store(out, name + "/dev", got)
    os.environ.pop(KNOB, None)
    out[name + "/logp_draws"] = ref.calc_logp(y[::sl], chain=chain)
    out[name + "/logp_proposals"] = ref.calc_logp(got["proposals"], chain=chain)
    for h in [s] + [k for k in keep if hasattr(k, "close")] + ([ref] if ref is not s else []):
        h.close()


def end_to_end(spec, out, torch, capi):
    """run_device, then the Python wrapper's fit-and-bridge on the returned tensor behind a burn-in, and on its download"""
    W, D, n, burn = spec["W"], spec["D"], spec["n"], spec["burn"]
    s = ed.make_handle(spec, capi)
    pos = np.random.default_rng(5).standard_normal((W, D))
    s.set_state(pos, s.calc_logp(pos))
    chain, _ = s.run_device(n)
    assert tuple(chain.shape) == (n, W, D)
    before = s.get_state(), s.counters()
    got = s.evidence_gaussian(chain[burn:], seed=21, want_proposals=True)
    after = s.get_state(), s.counters()
    out["e2e/state_untouched"] = np.int32(all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1] == after[1])
    store(out, "e2e/dev", got)
    out["e2e/mean"], out["e2e/chol"] = got["mean"], got["chol"]
    x = chain.cpu().numpy()
    out["e2e/steps"] = x
    head = ((n - burn) // 2)
    store(out, "e2e/host", s.evidence_gaussian(x[burn + head:], mean=got["mean"], chol=got["chol"], seed=21, want_proposals=True))
    out["e2e/logp_draws"] = s.calc_logp(x[burn + head:])
    out["e2e/logp_proposals"] = s.calc_logp(got["proposals"])
    # the fit is HipMoments' on the first half behind the burn-in
    m = capi.HipMoments(W, D)
    m.add_device_steps(chain[burn:burn + head])
    out["e2e/fit_mean"], out["e2e/fit_cov"] = m.finish()[1:3]
    m.close()
    s.close()


def refusals(out, torch, capi):
    """every refusal, through the C ABI itself so that the outputs can be watched"""
    import ctypes as C
    L = capi.lib()
    spec = dict(dtype="f64", calc="dense", K=1, n=6, W=10, D=4, betas=[1.0])
    n, W, D = 6, 10, 4
    N = n * W
    y = make_draws(spec)
    d = torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    P = ed.make_params(spec)[0]
    mean, chol = make_gaussian(spec)
    # log_evidence, mcse, overlap; ess [2]; passes, converged; nonfinite [2]; num_draws; proposals [N][D]; log_q [2][N]
    outs = [np.full(1, 777.0) for _ in range(3)] + [np.full(2, 777.0)] + [np.full(1, -7, np.int64) for _ in range(2)] + [np.full(2, -7, np.int64), np.full(1, -7, np.int64)] + \
           [np.full((N, D), 777.0), np.full((2, N), 777.0)]
    ptrs = [capi._ptr(a) for a in outs]
    host_ptrs = (C.c_void_p * n)(*[y[s].ctypes.data for s in range(n)])

    def untouched():
        return all((a == (777.0 if a.dtype == np.float64 else -7)).all() for a in outs)

    def attempt(tag, s, device=True, steps="own", n_steps=n, sl=1, chain=0, mean=mean, chol=chol):
        g = [capi._ptr(mean), capi._ptr(chol), 5, 0]
        if device:
            rc = L.mcmcpp_hip_evidence_gaussian_device(s.h, chain, C.c_void_p(d.data_ptr() if steps == "own" else steps), n_steps, sl, *(g + ptrs))
        else:
            rc = L.mcmcpp_hip_evidence_gaussian(s.h, chain, host_ptrs if steps == "own" else steps, n_steps, sl, *(g + ptrs))
        out["refusals/%s_code" % tag] = np.int32(rc)
        out["refusals/%s_message" % tag] = np.array((L.mcmcpp_hip_last_error(s.h) or b"").decode())
        out["refusals/%s_untouched" % tag] = np.int32(untouched())

    plain = capi.HipSampler(W, D, 1, P)
    wide = capi.HipSampler(132, 65, 0, None)
    y65 = np.zeros((n, 132, 65))
    d65 = torch.from_numpy(y65).cuda()
    torch.cuda.synchronize()
    ptrs65 = (C.c_void_p * n)(*[y65[s].ctypes.data for s in range(n)])
    for device in (True, False):
        t = "dev" if device else "host"
        attempt("d65_" + t, wide, device, steps=d65.data_ptr() if device else ptrs65, mean=np.zeros(65), chol=np.eye(65))
        attempt("sharded_" + t, capi.HipSampler(512, D, 1, P, shard_begin=0, shard_count=128), device)
        attempt("communicator_" + t, capi.HipSampler(512, D, 1, P, comm_world=1, comm_rank=0, comm_id=capi.comm_unique_id()), device)
        buf = torch.zeros((512, D), dtype=torch.float64, device="cuda")
        attempt("owned_" + t, capi.HipSampler(512, D, 1, P, device_positions=buf.data_ptr()), device)
        attempt("three_steps_" + t, plain, device, n_steps=3)
        attempt("three_used_steps_" + t, plain, device, sl=2)  # 6 steps, every second
        attempt("slice_" + t, plain, device, sl=0)
        attempt("null_" + t, plain, device, steps=None)
        attempt("null_mean_" + t, plain, device, mean=None)
        attempt("null_chol_" + t, plain, device, chol=None)
        attempt("chain_" + t, plain, device, chain=1)
        bad = mean.copy()
        bad[2] = np.inf
        attempt("mean_" + t, plain, device, mean=bad)
        bad = chol.copy()
        bad[3, 1] = np.nan
        attempt("factor_" + t, plain, device, chol=bad)
        bad = chol.copy()
        bad[1, 1] = 0.0
        attempt("diagonal_" + t, plain, device, chol=bad)
        attempt("batch_chain_" + t, capi.HipSampler(512, D, capi.CALC_BATCH, None, batch_callback=(capi.BATCH_LOGP_FN(lambda *a: 0), None)), device, chain=1)
        attempt("de_chain_" + t, capi.HipSampler(512, D, 1, P, mover=capi.MOVER_DIFFERENTIAL_EVOLUTION), device, chain=1)
    host_ptrs_hole = (C.c_void_p * n)(*[y[s].ctypes.data if s != 2 else None for s in range(n)])
    attempt("null_step_host", plain, False, steps=host_ptrs_hole)
    attempt("host_pointer_dev", plain, True, steps=y.ctypes.data)
    attempt("past_the_end_dev", plain, True, n_steps=10 ** 7)
    # while an asynchronous run is in progress
    busy = capi.HipSampler(512, D, 1, P)
    pos = np.random.default_rng(2).standard_normal((512, D))
    busy.set_state(pos, busy.calc_logp(pos))
    busy.run_async(200)
    attempt("async_dev", busy, True)
    attempt("async_host", busy, False)
    busy.run_wait()
    # the next call succeeds, without set_state; and with every output NULL
    got = plain.evidence_gaussian(d, mean=mean, chol=chol, seed=5, want_proposals=True)
    store(out, "refusals/after", got)
    out["refusals/all_null_code"] = np.int32(L.mcmcpp_hip_evidence_gaussian_device(plain.h, 0, C.c_void_p(d.data_ptr()), n, 1, capi._ptr(mean), capi._ptr(chol), 5, 0, *([None] * 10)))
    out["refusals/logp_draws"] = plain.calc_logp(y)
    out["refusals/logp_proposals"] = plain.calc_logp(got["proposals"])


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
    print("gaussian_bridge_device OK")


if __name__ == "__main__":
    main()
