"""The reference-style program end to end -- sample + sliceAndBurnChain + four analyses -- with a host chain and with a device
chain (MCMCPP_CHAIN_MEMORY=device): the same binary (tools/bench_device_facade.cpp), the variable unset and set.

Wall clock around the whole process, median of --runs runs (default five) per column; the per-phase split is the median
run's own (the program times its phases).  Shapes: 16 384 x 32 dense fp64 with 200 stored steps at interval 10, and 320 x 2, the
reference's own test shape.  Writes OUT/bench_device_facade.json (OUT: --out, default out/) and prints a table.

    python tools/bench_device_facade.py [--runs 5] [--out out]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16384, 32, 200, 10), (320, 2, 200, 10)]
PHASES = ["setup_ms", "sample_ms", "slice_ms", "autocorr_ms", "covariance_ms", "corner_ms", "percentile_ms", "main_ms"]


def build():
    sys.path.insert(0, ROOT)
    from mcmcpp_amd import capi
    lib_dir = os.path.join(ROOT, "mcmcpp_amd")
    if not os.path.exists(capi.library_path()):
        capi.build_library()
    exe = os.path.join(ROOT, "tools", "bench_device_facade.bin")
    src = os.path.join(ROOT, "tools", "bench_device_facade.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include", "MCMCpp"), "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                               "-L" + lib_dir, "-lmcmcpp_hip", "-Wl,-rpath," + lib_dir])
    return exe


def column(exe, shape, memory, runs):
    env = {k: v for k, v in os.environ.items() if k != "MCMCPP_CHAIN_MEMORY"}
    if memory:
        env["MCMCPP_CHAIN_MEMORY"] = memory
    results = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = subprocess.run([exe] + [str(v) for v in shape], capture_output=True, text=True, env=env, timeout=600, check=True).stdout
        wall = (time.perf_counter() - t0) * 1e3
        phases = json.loads(out.strip().split("\n")[-1])
        phases["process_wall_ms"] = wall
        results.append(phases)
    results.sort(key=lambda r: r["process_wall_ms"])
    median = results[len(results) // 2]
    median["process_wall_ms_all"] = [round(r["process_wall_ms"], 1) for r in results]
    median["process_wall_ms_median"] = statistics.median(r["process_wall_ms"] for r in results)
    return median


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.environ.get("OUT", "out"))
    args = ap.parse_args()
    exe = build()
    report = []
    for shape in SHAPES:
        host = column(exe, shape, None, args.runs)
        device = column(exe, shape, "device", args.runs)
        assert host["chain"] == "host" and device["chain"] == "device" and device["host_bytes_fetched"] == 0
        report.append({"shape": shape, "host": host, "device": device})
        print("%d x %d, %d stored steps at interval %d" % shape)
        print("  %-18s %12s %12s" % ("", "host chain", "device chain"))
        for k in ["process_wall_ms_median"] + PHASES:
            print("  %-18s %12.1f %12.1f" % (k.replace("_ms", "").replace("_median", ""), host[k], device[k]))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_device_facade.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
