"""GPU side of tests/test_rank_diagnostics.py, run in a child process under a time limit of its own:
    python -m tests.rank_device '<json spec>' <out.npz>
One child runs every case of the spec and writes, per case, what capi.normal_scores (fold 0 and 1) and capi.rank_diagnostics
returned through the host-pointer and the device entry points, and what the existing entry points (capi.effective_sample_size,
capi.gelman_rubin) return on those scores and on numpy-built indicator chains placed on the device; the parent builds the same
draws from the same spec (make_draws) and compares with the restatement (tests/rank_restatement.py) bit for bit.  A HIP error
ends the child at once: capi raises, nothing catches it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import rank_restatement as rk  # noqa: E402
from tests.rhat_device import make_steps, np_type, place_on_device  # noqa: E402

SCORE_KEYS = ("scores", "median", "q05", "q95")
DIAG_KEYS = ("rhat", "rhat_rank", "rhat_folded", "ess_bulk", "ess_tail", "ess_tail_lower", "ess_tail_upper", "median", "q05", "q95", "closed_bulk", "closed_tail")
WORK_MB, CHUNK_MB = "MCMCPP_HIP_RANK_WORK_MB", "MCMCPP_HIP_RHAT_CHUNK_MB"


def make_draws(spec):
    """the draws of a case, from its spec alone, [K][n][W][P]: those of tests/rhat_device.make_steps, or with spec["mode"]
      equal       every draw 2.5
      two         -1.5 or 3.0
      low_digit   numbers whose keys differ in the lowest digit only
      high_digit  numbers whose keys differ in the highest digit only (sign and exponent; all finite)
      sign        +c or -c
      special     -inf, negative, negative subnormal, -0, +0, subnormal, positive, +inf mixed with Gaussian draws
      apart       Gaussian columns; in the last column chain K - 1 has three times the scale of the others"""
    T = np_type(spec["dtype"])
    U = np.uint32 if T == np.float32 else np.uint64
    K, n, W, P = spec["K"], spec["n"], spec["W"], spec["P"]
    shape = (K, n, W, P)
    rng = np.random.default_rng(spec.get("seed", 1) + 1000)
    mode = spec.get("mode")
    if mode is None:
        return make_steps(spec)
    if mode == "equal":
        return np.full(shape, 2.5, T)
    if mode == "two":
        return np.where(rng.integers(0, 2, shape) == 1, T(3.0), T(-1.5)).astype(T)
    if mode == "low_digit":
        one = U(0x3F800000) if T == np.float32 else U(0x3FF0000000000000)
        return (one + rng.integers(0, 256, shape).astype(U)).view(T)
    if mode == "high_digit":
        low = U(0x2BCDEF) if T == np.float32 else U(0x0ABCDEF0123456)
        return ((rng.integers(0, 256, shape).astype(U) << U(8 * np.dtype(T).itemsize - 8)) | low).view(T)
    if mode == "sign":
        return np.where(rng.integers(0, 2, shape) == 1, T(0.7), T(-0.7)).astype(T)
    if mode == "special":
        tiny = np.finfo(T).smallest_subnormal
        palette = np.array([-np.inf, -2.0, -3 * tiny, -tiny, -0.0, 0.0, tiny, 5 * tiny, np.finfo(T).tiny, 1.5, np.inf], dtype=T)
        x = rng.standard_normal(shape).astype(T)
        pick = rng.integers(0, 3 * palette.size, shape)  # a third of the draws come from the palette
        return np.where(pick < palette.size, palette[pick % palette.size], x).astype(T)
    if mode == "apart":
        x = rng.standard_normal(shape).astype(T)
        x[K - 1, :, :, P - 1] *= T(3.0)
        return x
    raise ValueError(mode)


def host_view(spec, x):
    if not spec.get("scattered"):
        return x
    wide = np.zeros((x.shape[0], x.shape[1], 2) + x.shape[2:], x.dtype)  # every step a row of a wider array, in reverse
    wide[:, ::-1, 1] = x
    host = wide[:, ::-1, 1]
    assert not host.flags.c_contiguous and np.array_equal(host, x)
    return host


def run_case(name, spec, out, torch, capi):
    x = make_draws(spec)
    sl, split = spec.get("slice", 1), bool(spec.get("split", 1))
    for knob, key in ((WORK_MB, "work_mb"), (CHUNK_MB, "chunk_mb")):
        if key in spec:
            os.environ[knob] = str(spec[key])  # read per call
        else:
            os.environ.pop(knob, None)
    sources = []
    if spec.get("host", True):
        sources.append(("host_", host_view(spec, x)))
    if spec.get("device", True):
        d = place_on_device(spec, x, torch)
        sources.append(("dev_", d[0] if spec.get("one_chain_3d") else d))
    for prefix, src in sources:
        got = {}
        for fold in (0, 1):
            got[fold] = capi.normal_scores(src, split=split, fold=bool(fold), slice_interval=sl)
            for key in SCORE_KEYS:
                v = got[fold][key]
                out["%s/%sf%d_%s" % (name, prefix, fold, key)] = v.cpu().numpy() if capi._is_tensor(v) else v
            out["%s/%sf%d_shape" % (name, prefix, fold)] = np.array([got[fold]["sequence_length"], got[fold]["num_sequences"]])
        if prefix == "dev_":  # capi.quantiles on the same draws, as one chain of K H L steps (in the chain's type)
            ranked = rk.draws(x, split, sl)
            out[name + "/dev_quantiles"] = capi.quantiles(torch.from_numpy(ranked.reshape((-1,) + ranked.shape[2:])).cuda(), [0.5, 0.05, 0.95])
        if spec.get("diag"):
            dg = capi.rank_diagnostics(src, split=split, max_lag=spec.get("max_lag", 0), slice_interval=sl)
            for key in DIAG_KEYS:
                out["%s/%sdiag_%s" % (name, prefix, key)] = dg[key]
            out["%s/%sdiag_shape" % (name, prefix)] = np.array([dg["sequence_length"], dg["num_sequences"]])
            if prefix == "dev_":
                # the composition, by the existing entry points on chains in device memory
                kw = dict(split=split, max_lag=spec.get("max_lag", 0))
                q = got[0]
                dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                comp = rk.compose(lambda c: capi.effective_sample_size(c, **kw), lambda c: capi.gelman_rubin(c, split=split), got[0]["scores"], got[1]["scores"],
                                  dev(rk.indicators(x, q["q05"], split, sl)), dev(rk.indicators(x, q["q95"], split, sl)), q)
                for key in DIAG_KEYS:
                    out["%s/comp_%s" % (name, key)] = comp[key]
    os.environ.pop(WORK_MB, None)
    os.environ.pop(CHUNK_MB, None)


def sampler_chain(out, torch, capi):
    """chains the sampler wrote into device memory: HipSampler(num_chains=3).run_device, 64 x 4 iso-Gaussian, 900 stored steps,
    with the stretch scale 6 that gives four dimensions the acceptance of the large targets (a quarter): three draws in four
    repeat the one before"""
    W, P, n, K = 64, 4, 900, 3
    pos = np.random.default_rng(5).standard_normal((K, W, P))
    s = capi.HipSampler(W, P, capi.CALC_ISO_GAUSSIAN, None, seed=3, num_chains=K, alpha=(6, 1))
    s.set_state(pos, s.calc_logp(pos).reshape(K, W))
    chain, _ = s.run_device(n)
    assert tuple(chain.shape) == (K, n, W, P)
    for fold in (0, 1):
        got = capi.normal_scores(chain, fold=bool(fold))
        for key in SCORE_KEYS:
            v = got[key]
            out["sampler/f%d_%s" % (fold, key)] = v.cpu().numpy() if capi._is_tensor(v) else v
    dg = capi.rank_diagnostics(chain[:, 100:])
    host = capi.rank_diagnostics(chain[:, 100:].cpu().numpy())  # the host form, on the same steps
    for key in DIAG_KEYS:
        out["sampler/burn_diag_" + key] = dg[key]
        out["sampler/burn_host_diag_" + key] = host[key]
    out["sampler/chain"] = chain.cpu().numpy()


def errors(out, torch, capi):
    """the failures that need a device, through the C ABI itself so that the outputs can be watched"""
    import ctypes as C
    L = capi.lib()
    K, n, W, P = 3, 12, 10, 2
    x = make_steps(dict(dtype="f64", K=K, n=n, W=W, P=P, seed=11))
    bad = x.copy()
    bad[1, 7, 3, 1] = np.nan
    d, d_bad = torch.from_numpy(x).cuda(), torch.from_numpy(bad).cuda()
    scores = torch.full((K, n, W, P), 777.0, dtype=torch.float64, device="cuda")
    # half of what the scores need, as an allocation of its own (a torch tensor lies in a block of torch's allocator, which is
    # the allocation the runtime knows and may well hold the scores)
    small = L.mcmcpp_hip_device_alloc(-1, K * n * W * P * 8 // 2)
    assert small
    host_scores = np.full((K, n, W, P), 777.0)
    outs = [np.full(P, 777.0) for _ in range(3)]
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    ptrs = [capi._ptr(a) for a in outs + shape]
    torch.cuda.synchronize()

    def attempt(tag, device_steps, scores_ptr, fold=0):
        rc = L.mcmcpp_hip_normal_scores_device(capi.F64, -1, C.c_void_p(device_steps), K, 0, n, 1, W, P, 1, fold, C.c_void_p(scores_ptr), *ptrs)
        out["errors/%s_code" % tag] = np.int32(rc)
        out["errors/%s_message" % tag] = np.array((L.mcmcpp_hip_rank_diagnostics_last_error() or b"").decode())
        torch.cuda.synchronize()
        clean = all((a == 777.0).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6
        clean = clean and bool((scores == 777.0).all()) and bool((host_scores == 777.0).all())
        out["errors/%s_untouched" % tag] = np.int32(clean)

    attempt("nan_draw", d_bad.data_ptr(), scores.data_ptr())
    attempt("nan_draw_folded", d_bad.data_ptr(), scores.data_ptr(), fold=1)
    attempt("host_pointer", x.ctypes.data, scores.data_ptr())
    attempt("scores_small", d.data_ptr(), small)
    L.mcmcpp_hip_device_free(C.c_void_p(small))
    attempt("scores_host", d.data_ptr(), host_scores.ctypes.data)
    attempt("scores_null", d.data_ptr(), 0)
    # a median that is not finite: six walkers in ten at +inf in parameter 1 (median +inf); half of the draws at -inf (the
    # median interpolates between -inf and a finite draw: NaN).  Unfolded both are ranked; folded both fail.
    inf_med, nan_med = x.copy(), x.copy()
    inf_med[:, :, :6, 1] = np.inf
    nan_med[:, :, :5, 1] = -np.inf
    d_inf, d_nanmed = torch.from_numpy(inf_med).cuda(), torch.from_numpy(nan_med).cuda()
    torch.cuda.synchronize()
    attempt("inf_median_folded", d_inf.data_ptr(), scores.data_ptr(), fold=1)
    attempt("nan_median_folded", d_nanmed.data_ptr(), scores.data_ptr(), fold=1)
    for tag, dev, arr in (("inf_median", d_inf, inf_med), ("nan_median", d_nanmed, nan_med)):
        got = capi.normal_scores(dev)
        out["errors/%s_steps" % tag] = arr
        out["errors/%s_scores" % tag] = got["scores"].cpu().numpy()
        out["errors/%s_median" % tag] = got["median"]
    # the diagnostics refuse the NaN too, and leave their outputs alone
    dg = [np.full(P, 777.0) for _ in range(10)] + [np.full(P, 777, np.int64) for _ in range(2)]
    rc = L.mcmcpp_hip_rank_diagnostics_device(capi.F64, -1, C.c_void_p(d_bad.data_ptr()), K, 0, n, 1, W, P, 1, 0, *([capi._ptr(a) for a in dg] + ptrs[3:]))
    out["errors/diag_nan_code"] = np.int32(rc)
    out["errors/diag_nan_message"] = np.array((L.mcmcpp_hip_rank_diagnostics_last_error() or b"").decode())
    out["errors/diag_nan_untouched"] = np.int32(all((a == 777).all() for a in dg) and shape[0][0] == -5 and shape[1][0] == -6)
    rc = L.mcmcpp_hip_rank_diagnostics_device(capi.F64, -1, C.c_void_p(d_inf.data_ptr()), K, 0, n, 1, W, P, 1, 0, *([capi._ptr(a) for a in dg] + ptrs[3:]))
    out["errors/diag_inf_median_code"] = np.int32(rc)
    out["errors/diag_inf_median_message"] = np.array((L.mcmcpp_hip_rank_diagnostics_last_error() or b"").decode())
    out["errors/diag_inf_median_untouched"] = np.int32(all((a == 777).all() for a in dg) and shape[0][0] == -5 and shape[1][0] == -6)
    # the next call succeeds
    got = capi.normal_scores(d)
    out["errors/steps"] = x
    out["errors/after_scores"] = got["scores"].cpu().numpy()


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
    if spec.get("chains_file"):  # chains another program wrote ([K][n][W][P] float64, .npy): the C ABI on them, both forms
        x = np.load(spec["chains_file"])
        for prefix, src in (("host_", x), ("dev_", torch.from_numpy(x).cuda())):
            dg = capi.rank_diagnostics(src, split=bool(spec["split"]), slice_interval=spec["slice"])
            for key in DIAG_KEYS + ("sequence_length", "num_sequences"):
                out["file/%s%s" % (prefix, key)] = dg[key]
    np.savez(sys.argv[2], **out)
    print("rank_device OK")


if __name__ == "__main__":
    main()
