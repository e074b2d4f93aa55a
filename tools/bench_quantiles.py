#!/usr/bin/env python3
"""Exact percentiles of a device-resident chain (mcmcpp_hip_order_statistics_device) against what a user had before them:
copying the chain to the host and selecting there.  One job, three timings, on a chain HipSampler.run_device wrote (STEPS stored
steps of 16 384 x 32 fp64, dense Gaussian target; 1000 steps are 4.2 GB):

1. capi.quantiles(chain, q) for the percentiles 2.5, 16, 50, 84, 97.5 -- ten order statistics of every parameter, selected where
   the chain lies;
2. the copy of that chain to pinned host memory, alone;
3. numpy.partition at the same ten ranks on the downloaded chain, for one parameter (its column gathered first, as a user
   would), scaled by P.

The bar is 2, as measured here: a device path slower than the copy alone would leave a user nothing to lose by downloading.
The order statistics of the timed call are checked against numpy's for the parameter numpy selected.  Prints one JSON line.
    STEPS=1000 python tools/bench_quantiles.py"""
import json, os, sys, time
import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi, workloads

n, W, P = int(os.environ.get("STEPS", 1000)), 16384, 32
reps = int(os.environ.get("REPS", 5))
q = np.array([2.5, 16.0, 50.0, 84.0, 97.5]) / 100.0

s = capi.HipSampler(W, P, capi.CALC_DENSE_GAUSSIAN, workloads.ar1_precision(P, 0.5).ravel(), seed=0)
pos = workloads.init_positions(W, P, salt=0)
s.set_state(pos, s.calc_logp(pos))
chain, _ = s.run_device(n, want_accepted=False)
s.close()
torch.cuda.synchronize()
N = n * W


def timed(fn):
    fn()  # warm-up: allocations, first launches
    best = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); best.append(time.perf_counter() - t0)
    return min(best), float(np.median(best))


result = {}
def device_path():
    result["linear"] = capi.quantiles(chain, q)
t_dev = timed(device_path)
h, lo, hi = capi.quantile_ranks(q, N)
ranks = np.unique(np.concatenate([lo, hi]))
t_select = timed(lambda: result.__setitem__("values", capi.order_statistics(chain, ranks)))
t_counts = timed(lambda: result.__setitem__("counts", capi.rank_counts(chain, result["linear"])))

host = torch.empty(chain.shape, dtype=chain.dtype, pin_memory=True)
t_copy = timed(lambda: host.copy_(chain))
host_np = host.numpy()


def numpy_one_parameter():
    column = np.ascontiguousarray(host_np[:, :, 0]).ravel()
    result["numpy"] = np.partition(column, ranks)[ranks]
t_np = timed(numpy_one_parameter)
assert result["values"][0].tobytes() == result["numpy"].tobytes(), "the device's order statistics are not numpy's"
below, not_above = result["counts"]
assert (below <= np.ceil(h)).all() and (np.floor(h) < not_above).all()  # x_lo <= value <= x_hi

print(json.dumps({
    "metric": "exact percentiles 2.5/16/50/84/97.5 of every parameter, device-resident chain of %d x %d x %d fp64 (run_device)" % (n, W, P),
    "value": t_dev[0] * 1e3, "unit": "ms", "median_ms": t_dev[1] * 1e3, "chain_GB": chain.numel() * 8 / 1e9, "samples_per_parameter": N,
    "order_statistics_of_%d_ranks_ms" % ranks.size: {"min": t_select[0] * 1e3, "median": t_select[1] * 1e3,
                                                      "chain_reads_GBps": 8 * chain.numel() * 8 / t_select[0] / 1e9},
    "rank_counts_of_5_values_ms": {"min": t_counts[0] * 1e3, "median": t_counts[1] * 1e3},
    "copy_to_pinned_host_ms": {"min": t_copy[0] * 1e3, "median": t_copy[1] * 1e3, "GBps": chain.numel() * 8 / t_copy[0] / 1e9},
    "numpy_partition": {"one_parameter_ms": t_np[0] * 1e3, "scaled_by_P_ms": t_np[0] * 1e3 * P, "cores": 1},
    "device_path_over_copy": t_dev[0] / t_copy[0],
    "device_path_meets_the_bar": bool(t_dev[1] < t_copy[1]),
}))
