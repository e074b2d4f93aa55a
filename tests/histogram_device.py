"""GPU side of tests/test_histograms.py, run in a child process under a time limit of its own:
    python -m tests.histogram_device '<json spec>' <out.npz>
Every case writes the samples it used next to the device's results, so that the parent checks them against the
restatement (tests/histogram_restatement.py) or the reference's fixtures."""
import json
import os
import sys

import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mcmcpp_amd import capi  # noqa: E402
from tests import histogram_restatement as hr  # noqa: E402

EDGE_KS = 40  # random bin edges per parameter, beside the fixed ones


def _dt(name):
    return (np.float32, capi.F32) if name == "f32" else (np.float64, capi.F64)


def _results(prefix, h, out):
    n, bounds, single, pairs, clamped = h.result()
    out[prefix + "num_points"] = np.int64(n)
    out[prefix + "bounds"] = bounds
    out[prefix + "single"] = single
    if pairs is not None:
        out[prefix + "pairs"] = pairs
    out[prefix + "clamped"] = clamped


def fixture(spec, out):
    z = np.load(os.path.join(ROOT, "tests", "golden", spec["name"] + ".npz"))
    steps, sl = z["steps"], int(z["slice_interval"])
    dt = capi.F32 if steps.dtype == np.float32 else capi.F64
    W, P = steps.shape[1:]
    corner = capi.HipHistograms(W, P, int(z["corner_bins"]), True, dt)
    corner.compute(steps, sl)
    _results("corner_", corner, out)
    finder = capi.HipHistograms(W, P, int(z["finder_bins"]), False, dt)
    finder.compute(steps, sl)
    _results("finder_", finder, out)


def make_steps(spec):
    t, _ = _dt(spec["dtype"])
    rng = np.random.default_rng(spec.get("seed", 1))
    n, W, P = spec["n"], spec["W"], spec["P"]
    x = (rng.standard_normal((n, W, P)) * rng.uniform(0.2, 4.0, P) + rng.uniform(-3, 3, P)).astype(t)
    if n == 0:
        return x
    if not spec.get("positive"):
        x = (x - (x.reshape(-1, P).max(axis=0) + t(0.5))).astype(t)  # <= 0: the reference's defined case
    else:
        x = np.abs(x).astype(t) + t(0.25)
    for p in spec.get("constant", []):
        x[..., p] = t(spec.get("constant_value", -1.75))
    for p in spec.get("zero", []):
        x[..., p] = t(0)
    if spec.get("edges"):
        place_edges(x, spec["bins"], spec.get("slice", 1))
    return x


def place_edges(x, bins, slice_interval=1):
    """Overwrites samples of the used steps of non-positive x with values on the bin edges and beside them: per parameter,
    for k in 1, 2, 3, bins/3, bins/2, bins - 2, bins - 1, bins and EDGE_KS random k, the edge fl(lo + fl(k width)) as the
    analysis classes compute it and its two neighbours in T.  Only values above the parameter's minimum and not above 0 are
    placed, and never on the minimum's sample: the bounds stay what they were.  Returns the number of samples placed."""
    T = x.dtype.type
    P = x.shape[-1]
    used = x[::slice_interval]
    bounds = hr.find_binning(used, bins)
    flat = used.reshape(-1, P).copy()
    rng = np.random.default_rng(99)
    placed = 0
    for p in range(P):
        lo, w = T(bounds[p, 0]), T(bounds[p, 1])
        smallest, at = flat[:, p].min(), int(flat[:, p].argmin())
        ks = sorted(set([1, 2, 3, bins // 3, bins // 2, bins - 2, bins - 1, bins] + [int(k) for k in rng.integers(1, bins, EDGE_KS)]))
        vals = []
        for k in ks:
            e = T(lo + T(T(k) * w))
            for v in (np.nextafter(e, T(-np.inf)), e, np.nextafter(e, T(np.inf))):
                if v > smallest and v <= 0:
                    vals.append(v)
        rows = [r for r in rng.permutation(flat.shape[0]) if r != at][:len(vals)]
        flat[rows, p] = vals[:len(rows)]
        placed += len(rows)
    x[::slice_interval] = flat.reshape(used.shape)
    return placed


def random_case(spec, out):
    if "chunk_mb" in spec:
        os.environ["MCMCPP_HIP_HIST_CHUNK_MB"] = str(spec["chunk_mb"])  # read when the handle is created
    t, dt = _dt(spec["dtype"])
    steps = make_steps(spec)
    out["steps"] = steps
    W, P = steps.shape[1:]
    h = capi.HipHistograms(W, P, spec["bins"], spec.get("pairs", True), dt)
    h.compute(steps, spec.get("slice", 1))
    _results("host_", h, out)
    if spec.get("device", True):
        d = torch.from_numpy(steps).cuda() if steps.shape[0] else torch.zeros(1, device="cuda")  # (no steps: any address)
        h.compute_device(d.data_ptr(), steps.shape[0], spec.get("slice", 1))
        torch.cuda.synchronize()
        _results("dev_", h, out)


def device_chain(spec, out):
    """a chain written into device memory by the sampler's own half-steps (mcmcpp_hip_bind_device_chain)"""
    t, dt = _dt(spec["dtype"])
    W, P, n = spec["W"], spec["P"], spec["n"]
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((W, P)).astype(t)
    s = capi.HipSampler(W, P, capi.CALC_ISO_GAUSSIAN, None, seed=3, dtype=dt)
    s.set_state(pos, s.calc_logp(pos))
    chain = torch.zeros((n, W, P), dtype=torch.float32 if t == np.float32 else torch.float64, device="cuda")
    s.bind_device_chain(chain.data_ptr(), n)
    for k in range(n):
        s.half_step_async(0, -1)
        s.half_step_async(1, k)
    s.synchronize()
    h = capi.HipHistograms(W, P, spec["bins"], True, dt)
    h.compute_device(chain.data_ptr(), n, spec.get("slice", 1))
    _results("dev_", h, out)
    out["steps"] = chain.cpu().numpy()


def errors(spec, out):
    t, dt = _dt(spec["dtype"])
    steps = make_steps(dict(spec, n=4, W=70, P=3))
    h = capi.HipHistograms(70, 3, 16, True, dt)
    bad = steps.copy()
    bad[2, 5, 1] = np.nan
    try:
        h.compute(bad)
        out["nan_raised"] = np.int32(0)
    except capi.HipError as e:
        out["nan_raised"] = np.int32(1)
        out["nan_code"] = np.int32(e.code)
        out["nan_message"] = np.array(str(e))
    try:
        h.result()
        out["result_after_failure"] = np.int32(1)
    except capi.HipError:
        out["result_after_failure"] = np.int32(0)
    h.compute(steps)  # the handle stays usable
    out["steps"] = steps
    _results("after_", h, out)
    try:
        capi.HipHistograms(64, 1000, 1000, True, dt)  # 499 500 pairs of 10^6 64-bit counters: 4 TB
        out["oversize_raised"] = np.int32(0)
    except capi.HipError as e:
        out["oversize_raised"] = np.int32(1)
        out["oversize_code"] = np.int32(e.code)
        out["oversize_message"] = np.array(str(e))
    ok = capi.HipHistograms(70, 3, 16, True, dt)  # the library still works after the refusal
    ok.compute(steps)
    _results("later_", ok, out)


def device_info(spec, out):
    """what the library's launch plan depends on (mcmcpp_amd/csrc/hist_plan.hpp), of the device the cases run on"""
    prop = torch.cuda.get_device_properties(0)
    out["cus"] = np.int64(prop.multi_processor_count)
    out["shared_mem_per_block"] = np.int64(prop.shared_memory_per_block)


def main():
    spec = json.loads(sys.argv[1])
    out = {}
    {"fixture": fixture, "random": random_case, "device_chain": device_chain, "errors": errors, "device_info": device_info}[spec["kind"]](spec, out)
    np.savez(sys.argv[2], **out)
    print("histogram_device OK")


if __name__ == "__main__":
    main()
