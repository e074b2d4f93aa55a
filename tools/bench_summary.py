#!/usr/bin/env python3
"""The posterior summary of a device-resident chain (mcmcpp_hip_posterior_summary_device) against the cost of its parts through
the existing entry points, and against what a user had before it: copying the chains to the host.  One job, on the chain of
tools/bench_rank_diagnostics.py (STEPS stored steps of 16 384 x 32 fp64 that HipSampler.run_device wrote, dense Gaussian
target; 1000 steps are 4.2 GB), read as four chains of STEPS / 4 steps:

1. capi.posterior_summary(chain) with the default probs (0.05, 0.5, 0.95) and the 94 % interval, the whole call;
2. its parts: one capi.normal_scores with fold 0 (the one sort of 64-bit keys; it also ranks and scores, which the summary does
   not) and 2 + n_probs calls of capi.effective_sample_size (one is timed on the chain, the others cost the same: an fp64 chain
   of the same shape);
3. the copy of the chain to pinned host memory, alone: the floor of any host-side alternative.

Medians of REPS (3) calls behind a warm-up.  mean and ess_mean are checked against the ESS call, the quantiles against
capi.normal_scores.  Prints one JSON line and writes it to OUT (profiles/summary_bench.json).  With ONCE=1 only the summary is
run, once, and nothing is written: the run a kernel trace is taken of.
    STEPS=1000 python tools/bench_summary.py"""
import json, os, sys, time
import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi, workloads

n, W, P, K = int(os.environ.get("STEPS", 1000)) // 8 * 8, 16384, 32, 4
once = os.environ.get("ONCE") == "1"
reps = 1 if once else max(3, int(os.environ.get("REPS", 3)))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "summary_bench.json"))
PROBS, HDI = (0.05, 0.5, 0.95), 0.94

s = capi.HipSampler(W, P, capi.CALC_DENSE_GAUSSIAN, workloads.ar1_precision(P, 0.5).ravel(), seed=0)
pos = workloads.init_positions(W, P, salt=0)
s.set_state(pos, s.calc_logp(pos))
chain, _ = s.run_device(n, want_accepted=False)
s.close()
torch.cuda.synchronize()
nbytes = chain.numel() * 8
four = chain.view(K, n // K, W, P)


def timed(fn):
    if not once:
        fn()  # warm-up: allocations, first launches
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
    return {"min_ms": min(t) * 1e3, "median_ms": float(np.median(t)) * 1e3}


result, timings = {}, {}
timings["posterior_summary"] = timed(lambda: result.__setitem__("all", capi.posterior_summary(four, PROBS, HDI)))
a = result["all"]
if once:
    print(json.dumps({"posterior_summary_ms": timings["posterior_summary"]["median_ms"], "mcse_mean_max": float(a["mcse_mean"].max())}))
    sys.exit(0)
timings["normal_scores_fold0"] = timed(lambda: result.__setitem__("s0", capi.normal_scores(four)))
timings["effective_sample_size"] = timed(lambda: result.__setitem__("ess", capi.effective_sample_size(four)))
host = torch.empty(chain.shape, dtype=chain.dtype, pin_memory=True)
t_copy = timed(lambda: host.copy_(chain))

assert np.array_equal(a["mean"], result["ess"]["mean"]) and np.array_equal(a["ess_mean"], result["ess"]["ess"])
assert np.array_equal(a["quantile"][:, 1], result["s0"]["median"]) and np.array_equal(a["quantile"][:, 0], result["s0"]["q05"])
assert np.isfinite(a["mcse_quantile"]).all() and np.isfinite(a["mcse_sd"]).all() and (a["hdi_lower"] < a["mean"]).all() and (a["mean"] < a["hdi_upper"]).all()

S = K * 2 * W * (n // K // 2)
parts = timings["normal_scores_fold0"]["median_ms"] + (2 + len(PROBS)) * timings["effective_sample_size"]["median_ms"]
line = {
    "metric": "posterior summary (mean, sd, 3 quantiles, 94 %% HDI, their MCSE and ESS) of every parameter, device-resident chain of %d x %d x %d fp64 (run_device), four chains, split" % (n, W, P),
    "value": timings["posterior_summary"]["median_ms"], "unit": "ms", "reps": reps, "chain_GB": nbytes / 1e9, "draws_per_parameter": S,
    "timings": timings, "copy_to_pinned_host": t_copy, "parts_through_the_entry_points_ms": parts,
    "summary_over_parts": timings["posterior_summary"]["median_ms"] / parts,
    "summary_over_copy_to_host": timings["posterior_summary"]["median_ms"] / t_copy["median_ms"],
    "mcse_mean_max": float(a["mcse_mean"].max()), "mcse_median_max": float(a["mcse_quantile"][:, 1].max()), "ess_quantile_min": float(a["ess_quantile"].min()),
}
print(json.dumps(line))
with open(out_path, "w") as fh:
    fh.write(json.dumps(line, indent=1) + "\n")
