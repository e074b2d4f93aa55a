#!/usr/bin/env python3
"""The effective sample size of a device-resident chain (mcmcpp_hip_effective_sample_size_device) against what a user had
before it: copying the chains to the host, where a single-core estimate could then start.  One job, on a chain
HipSampler.run_device wrote (STEPS stored steps of 16 384 x 32 fp64, dense Gaussian target; 1000 steps are 4.2 GB), read as one
chain and, the same bytes, as four chains of STEPS / 4 steps:

1. capi.effective_sample_size(chain, split=True) with max_lag = 0 (the windows decide how many lags are evaluated) and with
   max_lag = 64 (one round of 64 lags: the cost per lag);
2. capi.gelman_rubin(chain), the first phase alone;
3. the copy of the chain to pinned host memory, alone.

The bar is 3, as measured here, as for R-hat.  Medians of REPS (at least 10) calls behind a warm-up.  The four-chain result is
checked on the downloaded chain:
the R-hat outputs bit for bit against capi.gelman_rubin, and tau against the
restatement of a chain thinned to 64 walkers (an estimate of the same time, not the same bits).  Prints one JSON line and
writes it to OUT (profiles/ess_bench.json).
    STEPS=1000 python tools/bench_ess.py"""
import json, os, sys, time
import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi, workloads
from tests import ess_restatement as er

n, W, P, K = int(os.environ.get("STEPS", 1000)) // 4 * 4, 16384, 32, 4
reps = max(10, int(os.environ.get("REPS", 10)))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "ess_bench.json"))

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
    return {"min_ms": min(t) * 1e3, "median_ms": float(np.median(t)) * 1e3}


result = {}
timings = {}
for tag, view in (("one_chain", chain), ("four_chains", four)):
    timings[tag] = timed(lambda: result.__setitem__(tag, capi.effective_sample_size(view)))
    timings[tag + "_max_lag_64"] = timed(lambda: result.__setitem__(tag + "_64", capi.effective_sample_size(view, max_lag=64)))
    timings[tag + "_gelman_rubin"] = timed(lambda: result.__setitem__(tag + "_rhat", capi.gelman_rubin(view)))
    timings[tag + "_ms_per_lag_at_64"] = (timings[tag + "_max_lag_64"]["median_ms"] - timings[tag + "_gelman_rubin"]["median_ms"]) / 64
host = torch.empty(chain.shape, dtype=chain.dtype, pin_memory=True)
t_copy = timed(lambda: host.copy_(chain))

for tag in ("one_chain", "four_chains"):
    for key in ("rhat", "mean", "within", "between"):
        assert np.array_equal(result[tag][key], result[tag + "_rhat"][key]) and np.array_equal(result[tag + "_64"][key], result[tag + "_rhat"][key]), (tag, key)
    assert np.isfinite(result[tag]["ess"]).all() and (result[tag]["tau"] > 1).all()
# the same time estimated by the restatement from 64 of the walkers
thin = np.ascontiguousarray(host.numpy().reshape(K, n // K, W, P)[:, :, ::W // 64, :])
want = er.effective_sample_size(thin)
ratio = result["four_chains"]["tau"] / want["tau"]

line = {
    "metric": "effective sample size of every parameter, device-resident chain of %d x %d x %d fp64 (run_device), split, max_lag 0" % (n, W, P),
    "value": timings["one_chain"]["median_ms"], "unit": "ms", "reps": reps, "chain_GB": nbytes / 1e9,
    "timings": timings, "copy_to_pinned_host": t_copy,
    "lags_used": {tag: [int(v) for v in result[tag]["lags_used"]] for tag in ("one_chain", "four_chains")},
    "closed": {tag: [int(v) for v in result[tag]["closed"]] for tag in ("one_chain", "four_chains")},
    "tau": {tag: [float(v) for v in result[tag]["tau"]] for tag in ("one_chain", "four_chains")},
    "ess_min": {tag: float(result[tag]["ess"].min()) for tag in ("one_chain", "four_chains")},
    "sequence_length": {tag: int(result[tag]["sequence_length"]) for tag in ("one_chain", "four_chains")},
    "tau_over_restatement_of_64_walkers_min_max": [float(ratio.min()), float(ratio.max())],
    "device_path_over_copy_to_host": {tag: timings[tag]["median_ms"] / t_copy["median_ms"] for tag in ("one_chain", "four_chains")},
    "device_path_meets_the_bar": bool(timings["one_chain"]["median_ms"] < t_copy["median_ms"] and timings["four_chains"]["median_ms"] < t_copy["median_ms"]),
}
print(json.dumps(line))
with open(out_path, "w") as fh:
    fh.write(json.dumps(line, indent=1) + "\n")
