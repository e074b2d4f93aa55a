"""GPU side of tests/test_quantiles.py, run in a child process under a time limit of its own:
    python -m tests.quantile_device '<json spec>' <out.npz>
One child runs every case of the spec (importing torch and opening the device costs more than the cases do) and writes, per
case, what the library returned; the parent builds the same samples from the same spec (make_steps) and checks the results
against the restatement (tests/quantile_restatement.py) and numpy."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ADVERSARIAL = ["constant", "three", "runs", "negative", "zeros", "inf", "subnormal", "last_digit", "first_digit"]


def np_type(name):
    return np.float32 if name == "f32" else np.float64


def adversarial_column(kind, N, T, rng):
    """one parameter's N samples of a shape that is hard on a radix select (tests/test_quantiles.py names them)"""
    U = np.uint32 if T == np.float32 else np.uint64
    key_bits = 8 * np.dtype(U).itemsize
    if kind == "constant":
        return np.full(N, -1.75, T)
    if kind == "three":
        return rng.choice(np.array([-2.0, 0.5, 7.0], T), N)
    if kind == "runs":  # what rejected proposals leave in a chain: runs of repeated values, run lengths geometric
        values = rng.standard_normal(N).astype(T)
        return np.repeat(values, rng.geometric(0.3, N))[:N]
    if kind == "negative":
        return (-np.abs(rng.standard_normal(N)) - 0.125).astype(T)
    if kind == "zeros":
        return rng.choice(np.array([-0.0, 0.0], T), N)
    if kind == "inf":
        return rng.choice(np.array([-np.inf, -1.0, 0.25, 3.0, np.inf], T), N)
    if kind == "subnormal":
        return (rng.integers(-1000, 1001, N) * np.float64(np.finfo(T).smallest_subnormal)).astype(T)
    if kind == "last_digit":  # the bits of 1.5 with the last eight varied
        return (np.full(N, 1.5, T).view(U) + rng.integers(0, 256, N).astype(U)).view(T)
    if kind == "first_digit":  # sign and the leading exponent bits varied, the rest fixed (no exponent of all ones: finite)
        return ((rng.integers(0, 256, N).astype(U) << U(key_bits - 8)) | U(0x12345)).view(T)
    raise ValueError(kind)


def make_steps(spec):
    """the samples of a case, from its spec alone: [n][W][P], Gaussian columns of different scales and offsets, column
    spec["column"] % P replaced by the adversarial column spec["adversarial"]"""
    T = np_type(spec["dtype"])
    n, W, P = spec["n"], spec["W"], spec["P"]
    rng = np.random.default_rng(spec.get("seed", 1))
    x = (rng.standard_normal((n, W, P)) * rng.uniform(0.2, 4.0, P) + rng.uniform(-3, 3, P)).astype(T)
    if spec.get("adversarial"):
        x[:, :, spec.get("column", 0) % P] = adversarial_column(spec["adversarial"], n * W, T, rng).reshape(n, W)
    return x


def make_ranks(spec, N):
    """the ranks of a case among N samples"""
    mode = spec.get("ranks", "percentiles")
    if mode == "ends":
        return [0, N - 1]
    if mode == "percentiles":
        return [int(np.floor(q * (N - 1))) for q in (0.025, 0.16, 0.5, 0.84, 0.975)]
    if mode == "many":  # 64 ranks, unsorted, repeats where N is small
        return [int(r) for r in np.random.default_rng(spec.get("seed", 1) + 1000).integers(0, N, 64)]
    if mode == "repeats":
        return [N - 1, 0, N // 2, 0, N // 2, N - 1]
    raise ValueError(mode)


def make_queries(steps, slice_interval):
    """[P][7] per parameter: a value equal to a sample, one below the minimum, one above the maximum, -0, +0, -inf, +inf"""
    x = steps[::slice_interval].reshape(-1, steps.shape[-1])
    T = x.dtype.type
    finite = np.where(np.isfinite(x), x, T(0))
    return np.stack([x[x.shape[0] // 3], finite.min(axis=0) - T(1), finite.max(axis=0) + T(1), np.full(x.shape[1], -0.0, T), np.full(x.shape[1], 0.0, T),
                     np.full(x.shape[1], -np.inf, T), np.full(x.shape[1], np.inf, T)], axis=1).astype(T)


def used_count(spec):
    sl = spec.get("slice", 1)
    return (spec["n"] + sl - 1) // sl * spec["W"]


def run_case(name, spec, out, torch, capi):
    steps = make_steps(spec)
    sl = spec.get("slice", 1)
    ranks = make_ranks(spec, used_count(spec))
    queries = make_queries(steps, sl)
    if "chunk_mb" in spec:
        os.environ["MCMCPP_HIP_QUANTILE_CHUNK_MB"] = str(spec["chunk_mb"])  # read per call
    else:
        os.environ.pop("MCMCPP_HIP_QUANTILE_CHUNK_MB", None)
    host = steps
    if spec.get("scattered"):  # host steps that are not contiguous in memory: every step a row of a wider array, in reverse
        wide = np.zeros((steps.shape[0], 2) + steps.shape[1:], steps.dtype)
        wide[::-1, 1] = steps
        host = wide[::-1, 1]
        assert not host.flags.c_contiguous and np.array_equal(host, steps)
    out[name + "/host_values"] = capi.order_statistics(host, ranks, sl)
    below, not_above = capi.rank_counts(host, queries, sl)
    out[name + "/host_below"], out[name + "/host_not_above"] = below, not_above
    if spec.get("device", True):
        # the steps one step inside a larger allocation: device_steps is not the start of its allocation
        room = torch.zeros((steps.shape[0] + 2,) + steps.shape[1:], dtype=torch.float32 if steps.dtype == np.float32 else torch.float64, device="cuda")
        room[1:-1] = torch.from_numpy(steps).cuda()
        d = room[1:-1]
        assert d.is_contiguous() and d.data_ptr() != room.data_ptr()
        values = capi.order_statistics(d, ranks, sl)
        out[name + "/dev_values"] = values
        below, not_above = capi.rank_counts(d, queries, sl)
        out[name + "/dev_below"], out[name + "/dev_not_above"] = below, not_above
        # the rank of every order statistic returned (as many queries as ranks: several query tiles of the kernel)
        below, not_above = capi.rank_counts(d, values, sl)
        out[name + "/dev_value_below"], out[name + "/dev_value_not_above"] = below, not_above
    os.environ.pop("MCMCPP_HIP_QUANTILE_CHUNK_MB", None)


def sampler_chain(out, torch, capi):
    """a chain written by the sampler into device memory: HipSampler.run_device, 64 x 4 iso-Gaussian, 200 stored steps"""
    W, P, n = 64, 4, 200
    pos = np.random.default_rng(5).standard_normal((W, P))
    s = capi.HipSampler(W, P, capi.CALC_ISO_GAUSSIAN, None, seed=3)
    s.set_state(pos, s.calc_logp(pos))
    chain, _ = s.run_device(n)
    q = [0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0]
    out["sampler/q"] = np.array(q)
    for method in ("linear", "lower", "higher"):
        out["sampler/" + method] = capi.quantiles(chain, q, method)
    out["sampler/linear_slice3"] = capi.quantiles(chain, q, "linear", 3)
    out["sampler/chain"] = chain.cpu().numpy()


def _failure(out, name, fn, capi, outputs):
    """fn must raise HipError; its code and message, and whether the outputs stayed as they were"""
    before = [o.copy() for o in outputs]
    try:
        fn()
        out["errors/" + name + "_raised"] = np.int32(0)
    except capi.HipError as e:
        out["errors/" + name + "_raised"] = np.int32(1)
        out["errors/" + name + "_code"] = np.int32(e.code)
        out["errors/" + name + "_message"] = np.array(str(e))
    out["errors/" + name + "_untouched"] = np.int32(all(np.array_equal(a, b) for a, b in zip(before, outputs)))


def errors(out, torch, capi):
    """the failures that need a device, through the C ABI itself so that the outputs can be watched"""
    import ctypes as C
    L = capi.lib()
    n, W, P = 4, 70, 3
    steps = make_steps(dict(dtype="f64", n=n, W=W, P=P, seed=11))
    bad = steps.copy()
    bad[2, 5, 1] = np.nan
    ranks = np.array([0, n * W // 2], np.int64)
    values = np.full((P, 2), 777.0)
    query = np.zeros((P, 1))
    below, not_above = np.full((P, 1), -5, np.int64), np.full((P, 1), -6, np.int64)

    def pointers(a):
        return (C.c_void_p * a.shape[0])(*[a[k].ctypes.data for k in range(a.shape[0])])

    def check(rc):
        if rc != capi.OK:
            raise capi.HipError(rc, (L.mcmcpp_hip_order_statistics_last_error() or b"").decode())

    p_good, p_bad = pointers(steps), pointers(bad)
    _failure(out, "nan_sample", lambda: check(L.mcmcpp_hip_order_statistics(capi.F64, -1, p_bad, n, W, P, capi._ptr(ranks), 2, capi._ptr(values))), capi, [values])
    _failure(out, "nan_sample_counts", lambda: check(L.mcmcpp_hip_rank_counts(capi.F64, -1, p_bad, n, W, P, capi._ptr(query), 1, capi._ptr(below),
                                                                               capi._ptr(not_above))), capi, [below, not_above])
    nan_query = np.full((P, 1), np.nan)
    _failure(out, "nan_query", lambda: check(L.mcmcpp_hip_rank_counts(capi.F64, -1, p_good, n, W, P, capi._ptr(nan_query), 1, capi._ptr(below),
                                                                       capi._ptr(not_above))), capi, [below, not_above])
    rank_n = np.array([0, n * W], np.int64)
    _failure(out, "rank_n", lambda: check(L.mcmcpp_hip_order_statistics(capi.F64, -1, p_good, n, W, P, capi._ptr(rank_n), 2, capi._ptr(values))), capi, [values])
    # a host pointer handed to the device entry points
    _failure(out, "host_pointer", lambda: check(L.mcmcpp_hip_order_statistics_device(capi.F64, -1, C.c_void_p(steps.ctypes.data), n, 1, W, P, capi._ptr(ranks), 2,
                                                                                     capi._ptr(values))), capi, [values])
    _failure(out, "host_pointer_counts", lambda: check(L.mcmcpp_hip_rank_counts_device(capi.F64, -1, C.c_void_p(steps.ctypes.data), n, 1, W, P, capi._ptr(query), 1,
                                                                                       capi._ptr(below), capi._ptr(not_above))), capi, [below, not_above])
    # device steps that do not end inside their allocation
    d = torch.from_numpy(steps).cuda()
    torch.cuda.synchronize()
    _failure(out, "past_the_end", lambda: check(L.mcmcpp_hip_order_statistics_device(capi.F64, -1, C.c_void_p(d.data_ptr()), n + 100000, 1, W, P, capi._ptr(ranks), 2,
                                                                                     capi._ptr(values))), capi, [values])
    # the next calls succeed
    out["errors/steps"] = steps
    out["errors/after_values"] = capi.order_statistics(steps, ranks)
    out["errors/after_dev_values"] = capi.order_statistics(d, ranks)
    out["errors/after_below"], out["errors/after_not_above"] = capi.rank_counts(d, query)


def main():
    import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
    from mcmcpp_amd import capi
    spec = json.loads(sys.argv[1])
    out = {}
    prop = torch.cuda.get_device_properties(0)
    out["cus"] = np.int64(prop.multi_processor_count)
    out["shared_mem_per_block"] = np.int64(prop.shared_memory_per_block)
    for name, case in spec.get("cases", {}).items():
        run_case(name, case, out, torch, capi)
        print("case %s done" % name, flush=True)
    if spec.get("sampler"):
        sampler_chain(out, torch, capi)
    if spec.get("errors"):
        errors(out, torch, capi)
    np.savez(sys.argv[2], **out)
    print("quantile_device OK")


if __name__ == "__main__":
    main()
