#!/usr/bin/env python3
"""Row f2 measurement: Analysis::CornerHistograms (100 bins) and Analysis::PercentileAndMaximumFinder (10 000 bins) over
a C2-sized chain (n stored steps of 16384 x 32 fp64): the device counting from a device-resident chain and from host
memory (upload included), against the restatement of the reference (tests/histogram_restatement.py) on one host core,
timed on a few steps and scaled per sample.  Prints one JSON line.
    STEPS=200 python tools/bench_histograms.py"""
import json, os, sys, time
import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi
from tests import histogram_restatement as hr

n, W, P = int(os.environ.get("STEPS", 200)), 16384, 32
reps = int(os.environ.get("REPS", 5))
rng = np.random.default_rng(0)
steps = (rng.standard_normal((n, W, P)) * np.linspace(0.5, 2.0, P)).astype(np.float64)
samples = n * W
dev = torch.from_numpy(steps).cuda()
torch.cuda.synchronize()


def timed(fn):
    fn()  # warm-up: allocations, first launches
    best = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); best.append(time.perf_counter() - t0)
    return min(best), float(np.median(best))


corner = capi.HipHistograms(W, P, 100, True)
finder = capi.HipHistograms(W, P, 10000, False)
c_dev = timed(lambda: corner.compute_device(dev.data_ptr(), n))
_, cb_dev, cs_dev, cp_dev, _ = corner.result()
f_dev = timed(lambda: finder.compute_device(dev.data_ptr(), n))
_, fb_dev, fs_dev, _, _ = finder.result()
c_host = timed(lambda: corner.compute(steps))
_, cb_h, cs_h, cp_h, _ = corner.result()
assert (cs_h == cs_dev).all() and (cp_h == cp_dev).all() and cb_h.tobytes() == cb_dev.tobytes()
f_host = timed(lambda: finder.compute(steps))

cpu_n = min(n, 2)
t0 = time.perf_counter(); want = hr.histograms(steps[:cpu_n], 100, 1, True); t_cpu_c = time.perf_counter() - t0
t0 = time.perf_counter(); hr.histograms(steps[:cpu_n], 10000, 1, False); t_cpu_f = time.perf_counter() - t0
corner.compute(steps[:cpu_n])
_, _, s2, p2, _ = corner.result()
assert (s2 == want["single"]).all() and (p2 == want["pairs"]).all()
cpu_c_per_sample = t_cpu_c / (cpu_n * W)
cpu_f_per_sample = t_cpu_f / (cpu_n * W)
pairs = P * (P - 1) // 2
print(json.dumps({
    "metric": "Analysis::CornerHistograms, 16384 walkers x 32 params fp64 x %d stored steps, 100 bins, device-resident chain" % n,
    "value": c_dev[0] * 1e3, "unit": "ms", "median_ms": c_dev[1] * 1e3, "samples": samples, "pair_increments": samples * pairs,
    "pair_increments_per_s": samples * pairs / c_dev[0], "chain_GB": steps.nbytes / 1e9,
    "host_chain": {"ms": c_host[0] * 1e3, "median_ms": c_host[1] * 1e3, "upload_GBps": 2 * steps.nbytes / c_host[0] / 1e9
                   if steps.nbytes > (1024 << 20) else steps.nbytes / c_host[0] / 1e9},
    "percentile_finder_10000_bins": {"device_ms": f_dev[0] * 1e3, "host_chain_ms": f_host[0] * 1e3},
    "cpu_baseline": {"kind": "port", "cores": 1, "corner_ms_scaled": cpu_c_per_sample * samples * 1e3,
                     "finder_ms_scaled": cpu_f_per_sample * samples * 1e3, "sample": "%d stored steps: %.2f s + %.2f s" % (cpu_n, t_cpu_c, t_cpu_f)},
    "speedup_corner_device_vs_cpu": cpu_c_per_sample * samples / c_dev[0],
    "speedup_finder_device_vs_cpu": cpu_f_per_sample * samples / f_dev[0],
}))
