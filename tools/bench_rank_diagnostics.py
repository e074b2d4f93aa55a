#!/usr/bin/env python3
"""Rank-normalised R-hat, bulk-ESS and tail-ESS of a device-resident chain (mcmcpp_hip_rank_diagnostics_device) against what a
user had before it: copying the chains to the host, where another package could then start.  One job, on the chain of
tools/bench_ess.py (STEPS stored steps of 16 384 x 32 fp64 that HipSampler.run_device wrote, dense Gaussian target; 1000 steps
are 4.2 GB), read as four chains of STEPS / 4 steps:

1. capi.rank_diagnostics(chain), the whole call;
2. its parts, through the entry points it is composed of: capi.normal_scores with fold 0 (one sort of 64-bit keys, the ranks
   and scores) and fold 1 (the same twice: the median comes from a sort of the raw draws), capi.effective_sample_size and
   capi.gelman_rubin on the scores;
3. the copy of the chain to pinned host memory, alone: the floor of any host-side alternative.

The sort's traffic is counted from the plan: a pass reads the keys twice (histogram, scatter) and the indices once, and writes
both once: per draw 3 x key bytes + 2 x 4.  Medians of REPS calls behind a warm-up.  The whole call is checked against its
parts bit for bit.  Prints one JSON line and writes it to OUT (profiles/rank_diagnostics_bench.json).  With ONCE=1 every call
is made once and nothing is written: the run a kernel trace is taken of.
    STEPS=1000 python tools/bench_rank_diagnostics.py"""
import json, os, sys, time
import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi, workloads

n, W, P, K = int(os.environ.get("STEPS", 1000)) // 8 * 8, 16384, 32, 4
once = os.environ.get("ONCE") == "1"
reps = 1 if once else max(3, int(os.environ.get("REPS", 5)))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "rank_diagnostics_bench.json"))
PEAK_HBM_GBS = 8000.0  # MI355X

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
timings["rank_diagnostics"] = timed(lambda: result.__setitem__("all", capi.rank_diagnostics(four)))
timings["normal_scores_fold0"] = timed(lambda: result.__setitem__("s0", capi.normal_scores(four)))
timings["normal_scores_fold1"] = timed(lambda: result.__setitem__("s1", capi.normal_scores(four, fold=True)))
timings["ess_on_scores"] = timed(lambda: result.__setitem__("bulk", capi.effective_sample_size(result["s0"]["scores"])))
timings["gelman_rubin_on_scores"] = timed(lambda: result.__setitem__("folded", capi.gelman_rubin(result["s1"]["scores"])))
host = torch.empty(chain.shape, dtype=chain.dtype, pin_memory=True)
t_copy = timed(lambda: host.copy_(chain))

a = result["all"]
assert np.array_equal(a["rhat_rank"], result["bulk"]["rhat"]) and np.array_equal(a["ess_bulk"], result["bulk"]["ess"]) and np.array_equal(a["rhat_folded"], result["folded"]["rhat"])
assert np.array_equal(a["median"], result["s0"]["median"]) and np.isfinite(a["rhat"]).all() and np.isfinite(a["ess_tail"]).all()
x0 = host.numpy()[..., 0].ravel()
duplicates = 1.0 - np.unique(x0).size / x0.size

S = K * 2 * W * (n // K // 2)
pass_bytes = S * P * (3 * 8 + 2 * 4)
sort_bytes = 8 * pass_bytes  # eight passes of 64-bit keys
line = {
    "metric": "rank-normalised R-hat, bulk- and tail-ESS of every parameter, device-resident chain of %d x %d x %d fp64 (run_device), four chains, split" % (n, W, P),
    "value": timings["rank_diagnostics"]["median_ms"], "unit": "ms", "reps": reps, "chain_GB": nbytes / 1e9, "draws_per_parameter": S,
    "duplicates_of_parameter_0": duplicates, "timings": timings, "copy_to_pinned_host": t_copy,
    "sort_GB_per_pass_all_parameters": pass_bytes / 1e9, "sort_GB_of_one_sort": sort_bytes / 1e9,
    "one_sort_at_peak_hbm_ms": sort_bytes / (PEAK_HBM_GBS * 1e9) * 1e3,
    "rhat": [float(v) for v in a["rhat"]], "ess_bulk_min": float(a["ess_bulk"].min()), "ess_tail_min": float(a["ess_tail"].min()),
    "device_path_over_copy_to_host": timings["rank_diagnostics"]["median_ms"] / t_copy["median_ms"],
}
print(json.dumps(line))
if not once:
    with open(out_path, "w") as fh:
        fh.write(json.dumps(line, indent=1) + "\n")
