#!/usr/bin/env python3
"""Measurement of mcmcpp_hip_run_device at C2 (16 384 x 32 dense fp64, 2 000 ensemble steps), DESIGN.md section 6:

1. run_device, storing every step and every 100th, against mcmcpp_hip_run into mcmcpp_hip_host_alloc memory (the launches
   forward stored steps straight into it) -- of this build and, with --parent-lib, of another build of the library (the
   parent commit's), loaded through MCMCPP_HIP_LIB.  Five runs each behind a warm-up run: median, minimum and maximum of
   the wall time of the call and of the GPU time of its step launches.  The step launches of two processes of the SAME
   build differ by more (0.1 ms per 2 000 steps) than the five runs of one process do (0.03 ms): every measurement is
   therefore taken in --processes processes, the three kinds in turn, and the medians of the processes are reported
   beside each process's own five runs.
2. End to end for 20 stored steps: run -> HipMoments.add_steps (pageable host memory, what an ordinary caller has) against
   run_device -> HipMoments.add_device_steps, covariance included.

3. The slicing stride of the device covariance: every 5th of 2 000 stored steps (400 steps gathered by one device-to-device
   copy each into the chunk buffer, 64 MiB chunks) against 400 contiguous stored steps read where they lie.

Every measurement runs in a process of its own (a library is chosen once per process).  Prints one JSON document and, with
--out, writes it there.

    python tools/bench_device_chain.py --parent-lib /path/to/parent/libmcmcpp_hip.so --out profiles/device_chain_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, D, STEPS, RUNS = 16384, 32, 2000, 5


def across(procs):
    """One kind of measurement taken in several processes: each process's numbers, and the spread of their medians."""
    med = [p["wall_ms"]["median"] for p in procs]
    return {"wall_ms_median_of_process_medians": statistics.median(med), "wall_ms_process_medians": med,
            "largest_min_to_max_spread_inside_a_process_ms": max(p["wall_ms"]["max"] - p["wall_ms"]["min"] for p in procs),
            "min_to_max_spread_of_process_medians_ms": max(med) - min(med), "processes": procs}


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def worker(what, interval):
    import numpy as np
    import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
    sys.path.insert(0, ROOT)
    from mcmcpp_amd import capi, workloads
    P = workloads.ar1_precision(D, 0.5)
    s = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, P.ravel(), seed=0)
    pos = workloads.init_positions(W, D, salt=0)
    s.set_state(pos, s.calc_logp(pos))
    n_saved = STEPS // interval
    wall, gpu = [], []

    def timed(call):
        call()  # warm-up: allocations, graph capture
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(s.last_run_timing()[0])

    if what == "run_pinned":
        out = capi.pinned_empty((n_saved, W, D))
        timed(lambda: s.run(n_saved, interval=interval, out=out, want_accepted=False))
    elif what == "run_device":
        out = torch.empty((n_saved, W, D), dtype=torch.float64, device="cuda")
        timed(lambda: s.run_device(n_saved, interval=interval, out=out, want_accepted=False))
    elif what == "run_then_add_steps":
        out = np.empty((n_saved, W, D))
        m = capi.HipMoments(W, D)

        def call():
            m.reset()
            s.run(n_saved, interval=interval, out=out, want_accepted=False)
            m.add_steps(out)
            m.finish()
        timed(call)
    elif what == "run_device_then_add_device_steps":
        out = torch.empty((n_saved, W, D), dtype=torch.float64, device="cuda")
        m = capi.HipMoments(W, D)

        def call():
            m.reset()
            s.run_device(n_saved, interval=interval, out=out, want_accepted=False)
            m.add_device_steps(out)
            m.finish()
        timed(call)
    elif what in ("add_device_steps_every_5th_of_2000", "add_device_steps_400_contiguous"):
        chain = torch.randn((STEPS, W, D), dtype=torch.float64, device="cuda")
        m = capi.HipMoments(W, D)

        def call():
            m.reset()
            if what.endswith("contiguous"):
                m.add_device_steps(chain[:STEPS // 5])
            else:
                m.add_device_steps(chain, slice_interval=5)
        timed(call)
    else:
        raise SystemExit("unknown measurement %s" % what)
    print(json.dumps({"what": what, "stored_steps": n_saved, "interval": interval, "library": "the build named by MCMCPP_HIP_LIB" if os.environ.get("MCMCPP_HIP_LIB") else "this build",
                      "wall_ms": summary(wall), "gpu_ms_of_the_step_launches": summary(gpu)}))


def measure(what, interval, lib=None):
    env = dict(os.environ)
    if lib:
        env["MCMCPP_HIP_LIB"] = lib
    else:
        env.pop("MCMCPP_HIP_LIB", None)
    # (a fresh process per measurement; nothing else uses the device meanwhile)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", what, "--interval", str(interval)], env=env, capture_output=True,
                         text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit("%s failed (exit %d):\n%s" % (what, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--interval", type=int, default=1)
    ap.add_argument("--parent-lib", help="another build of libmcmcpp_hip.so to time mcmcpp_hip_run of (the parent commit's)")
    ap.add_argument("--processes", type=int, default=3, help="processes per kind of delivery measurement")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.interval)
    doc = {"workload": "C2: %d walkers x %d dims, correlated Gaussian (rho = 0.5, dense precision), fp64, StretchMove, %d ensemble steps per run" % (W, D, STEPS),
           "runs_each": RUNS, "delivery": {}, "end_to_end_20_stored_steps": {}}
    for interval, key in ((1, "every_step"), (100, "every_100th_step")):
        kinds = [("run_device", "run_device", None), ("run_into_pinned_host_memory", "run_pinned", None)]
        if args.parent_lib:
            kinds.append(("parent_run_into_pinned_host_memory", "run_pinned", args.parent_lib))
        got = {name: [] for name, _, _ in kinds}
        for _ in range(args.processes):
            for name, what, lib in kinds:
                got[name].append(measure(what, interval, lib))
        row = {name: across(procs) for name, procs in got.items()}
        if args.parent_lib:
            parent = row["parent_run_into_pinned_host_memory"]
            row["run_device_minus_parent_ms"] = row["run_device"]["wall_ms_median_of_process_medians"] - parent["wall_ms_median_of_process_medians"]
            row["parent_spread_inside_a_process_ms"] = parent["largest_min_to_max_spread_inside_a_process_ms"]
            row["parent_spread_of_process_medians_ms"] = parent["min_to_max_spread_of_process_medians_ms"]
        doc["delivery"][key] = row
    doc["end_to_end_20_stored_steps"] = {"run_then_add_steps": measure("run_then_add_steps", 100),
                                         "run_device_then_add_device_steps": measure("run_device_then_add_device_steps", 100)}
    doc["covariance_sums_of_400_stored_steps"] = {k: measure(k, 1) for k in ("add_device_steps_every_5th_of_2000", "add_device_steps_400_contiguous")}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
