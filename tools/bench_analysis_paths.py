#!/usr/bin/env python3
"""The two cases the other analysis benches leave out: autocorrelation times of a device-resident chain (bench_autocorr.py
uploads its chain) and percentiles of a host chain (bench_quantiles.py reads a device chain); autocorr's host path again at
the same size, for comparison.  Minimum and median of five timed calls behind a warm-up; prints one JSON line.
    MCMCPP_HIP_LIB=<another build> python tools/bench_analysis_paths.py"""
import json, os, sys, time
import numpy as np
import torch  # (before the library)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi

reps = 5
rng = np.random.default_rng(3)


def timed(fn):
    fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
    return {"min_ms": min(t) * 1e3, "median_ms": float(np.median(t)) * 1e3}


ac = rng.standard_normal((500, 4096, 16))
ac_dev = torch.from_numpy(ac).cuda()
qh = rng.standard_normal((200, 16384, 32))
q = np.array([2.5, 16.0, 50.0, 84.0, 97.5]) / 100.0
out = {"autocorr_device_500x4096x16": timed(lambda: capi.autocorr_times_device(ac_dev)),
       "autocorr_host_500x4096x16": timed(lambda: capi.autocorr_times(ac, 0, 4)),
       "quantiles_host_200x16384x32": timed(lambda: capi.quantiles(qh, q)),
       "lib": os.environ.get("MCMCPP_HIP_LIB", "this build")}
print(json.dumps(out))
