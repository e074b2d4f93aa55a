#!/usr/bin/env python3
"""The Gelman-Rubin split R-hat of a device-resident chain (mcmcpp_hip_gelman_rubin_device) against what a user had before it:
copying the chains to the host and looping in numpy.  One job, on a chain HipSampler.run_device wrote (STEPS stored steps of
16 384 x 32 fp64, dense Gaussian target; 1000 steps are 4.2 GB), read as one chain and, the same bytes, as four chains of
STEPS / 4 steps:

1. capi.gelman_rubin(chain, split=True), the chain read once where it lies;
2. a device-to-device copy of the same bytes, the bandwidth yardstick (a copy reads and writes every byte; the rate quoted is
   the bytes copied over the time);
3. the copy of the chain to pinned host memory, alone.

The bar is 3, as measured here: a device path slower than the copy alone would leave a user nothing to lose by downloading.
Medians of REPS (at least 10) calls behind a warm-up.  The four-chain result is checked against the numpy restatement of the
definition on the downloaded chain for two walkers' worth of columns.  Prints one JSON line and writes it to OUT
(profiles/rhat_bench.json).
    STEPS=1000 python tools/bench_rhat.py"""
import json, os, sys, time
import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi, workloads
from tests import rhat_restatement as rr

n, W, P, K = int(os.environ.get("STEPS", 1000)) // 4 * 4, 16384, 32, 4
reps = max(10, int(os.environ.get("REPS", 10)))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "rhat_bench.json"))

s = capi.HipSampler(W, P, capi.CALC_DENSE_GAUSSIAN, workloads.ar1_precision(P, 0.5).ravel(), seed=0)
pos = workloads.init_positions(W, P, salt=0)
s.set_state(pos, s.calc_logp(pos))
chain, _ = s.run_device(n, want_accepted=False)
s.close()
torch.cuda.synchronize()
nbytes = chain.numel() * 8
four = chain.view(K, n // K, W, P)


def timed(fn):
    fn()  # warm-up: allocations, first launches
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
    return {"min_ms": min(t) * 1e3, "median_ms": float(np.median(t)) * 1e3, "GBps": nbytes / float(np.median(t)) / 1e9}


result = {}
t_one = timed(lambda: result.__setitem__("one", capi.gelman_rubin(chain)))
t_four = timed(lambda: result.__setitem__("four", capi.gelman_rubin(four)))
twin = torch.empty_like(chain)
t_d2d = timed(lambda: twin.copy_(chain))
del twin
host = torch.empty(chain.shape, dtype=chain.dtype, pin_memory=True)
t_copy = timed(lambda: host.copy_(chain))

# the device's figures against the restatement, on the sequences of walkers 0 and 16383 of every chain and half
host_np = host.numpy().reshape(K, n // K, W, P)
want = rr.gelman_rubin(np.ascontiguousarray(host_np[:, :, [0, W - 1], :]))
got = capi.gelman_rubin(four, want_sequences=True)  # (not timed: the M x P sequence figures come to the host too)
assert all(np.array_equal(got[k], result["four"][k]) for k in ("rhat", "mean", "within", "between"))
rows = np.array([z * W + w for z in range(2 * K) for w in (0, W - 1)])
assert np.array_equal(got["sequence_mean"][rows], want["sequence_mean"]) and np.array_equal(got["sequence_m2"][rows], want["sequence_m2"]), \
    "the device's sequence means and sums of squares are not the restatement's"
assert np.isfinite(got["rhat"]).all() and np.isfinite(result["one"]["rhat"]).all()

line = {
    "metric": "Gelman-Rubin split R-hat of every parameter, device-resident chain of %d x %d x %d fp64 (run_device), read once" % (n, W, P),
    "value": t_one["median_ms"], "unit": "ms", "reps": reps, "chain_GB": nbytes / 1e9,
    "one_chain": dict(t_one, sequences=result["one"]["num_sequences"], sequence_length=result["one"]["sequence_length"]),
    "four_chains_of_%d_steps" % (n // K): dict(t_four, sequences=got["num_sequences"], sequence_length=got["sequence_length"]),
    "device_to_device_copy": t_d2d,
    "copy_to_pinned_host": t_copy,
    "fraction_of_d2d_copy_rate": {"one_chain": t_d2d["median_ms"] / t_one["median_ms"], "four_chains": t_d2d["median_ms"] / t_four["median_ms"]},
    "device_path_over_copy_to_host": {"one_chain": t_one["median_ms"] / t_copy["median_ms"], "four_chains": t_four["median_ms"] / t_copy["median_ms"]},
    "device_path_meets_the_bar": bool(t_one["median_ms"] < t_copy["median_ms"] and t_four["median_ms"] < t_copy["median_ms"]),
    "rhat_one_chain_max": float(result["one"]["rhat"].max()), "rhat_four_chains_max": float(got["rhat"].max()),
}
print(json.dumps(line))
with open(out_path, "w") as fh:
    fh.write(json.dumps(line, indent=1) + "\n")
