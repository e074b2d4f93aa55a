#!/usr/bin/env python3
"""Generate the histogram fixtures in tests/golden/ by running the REFERENCE's CornerHistograms and
PercentileAndMaximumFinder (over its own Chain) through tests/golden/histogram_ref_driver.cpp.

Runs only where the reference exists (like make_golden.py).  The driver is compiled into a temporary directory, twice:
with g++ -std=c++11 -O2 -ffp-contract=off -fno-fast-math for the fixtures, and once more with -fsanitize=address to
assert that the reference ran clean on every case.  Inputs keep the reference defined: every sample is <= 0 (each
parameter is shifted below zero), so its upper bound stays at numeric_limits<T>::min() and no bin leaves the range;
the generator also asserts that the restatement (tests/histogram_restatement.py) clamps nothing and reproduces every
output bit for bit.  Only the .npz / .json data it writes is committed.

    python tests/golden/make_histogram_golden.py [/path/to/reference]
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import histogram_restatement as hr  # noqa: E402

PERCENTILES = [-1.0, 0.0, 0.5, 2.5, 15.9, 34.1, 50.0, 65.9, 84.1, 97.5, 100.0, 101.0]


def make_steps(rng, n, W, P, dtype, kind):
    x = rng.standard_normal((n, W, P))
    if kind == "skewed":  # a skewed pair, like the reference's SkewedGaussian test
        x[..., 1] = 0.6 * x[..., 0] + 0.8 * x[..., 1]
        x[..., 0] = np.abs(x[..., 0]) * 1.5 - 0.4 * x[..., 1]
    x = x * rng.uniform(0.5, 3.0, P) + rng.uniform(-4, 4, P)
    x = x.astype(dtype)
    # every sample <= 0: shift each parameter by its maximum plus a margin
    shift = (x.reshape(-1, P).max(axis=0) + dtype(0.25)).astype(dtype)
    x = (x - shift).astype(dtype)
    if kind == "degenerate":
        # a constant parameter, and one that takes a single value on all but one walker.  (An all-zero parameter cannot be
        # a fixture: for samples <= 0 a sample at 0 gives (0 - lo) / width == bins exactly, outside the reference's arrays;
        # tests/test_histograms.py covers it against the restatement, clamped.)
        x[..., P - 2] = dtype(-2.5)
        x[..., P - 1] = dtype(-0.125)
        x[:, 0, P - 1] = dtype(-7.0)
    assert (x <= 0).all()
    return x


CASES = {
    # name: shape, dtype, slice interval, corner bins, finder bins, kind, csv
    "hist_skewed320x2": dict(n=25, W=320, P=2, dtype=np.float64, slice=1, cb=100, pb=10000, kind="skewed"),
    "hist_skewed320x2_f32": dict(n=25, W=320, P=2, dtype=np.float32, slice=1, cb=100, pb=10000, kind="skewed"),
    "hist_96x5_slice3": dict(n=30, W=96, P=5, dtype=np.float64, slice=3, cb=20, pb=500, kind="degenerate"),
    "hist_96x5_slice3_f32": dict(n=30, W=96, P=5, dtype=np.float32, slice=3, cb=20, pb=500, kind="degenerate"),
    "hist_40x3_bins2": dict(n=10, W=40, P=3, dtype=np.float64, slice=1, cb=2, pb=2, kind="normal"),
    "hist_16x3_csv": dict(n=10, W=16, P=3, dtype=np.float64, slice=1, cb=8, pb=8, kind="normal", csv=True),
}


def value_queries(bounds, single, P, dtype):
    """a grid over and around every parameter's range, the range's edges and the peak"""
    T = dtype
    out = []
    for p in range(P):
        lo, w = T(bounds[p, 0]), T(bounds[p, 1])
        bins = single.shape[1]
        top = T(lo + T(w * T(bins)))
        grid = [T(lo - abs(w)), lo, top, T(lo + T(w * T(bins + 1))), hr.value_of_peak(bounds, single, p)]
        grid += [T(lo + T(T(f) * T(top - lo))) for f in (0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999)]
        out.append(np.array(grid, T))
    return np.stack(out)


def percentile_queries(bounds, single, num_points, P, dtype):
    """the fixed grid, minus the queries whose bisection would never end in the reference"""
    cs = hr.cum_sums(single)
    rows = []
    for p in range(P):
        rows.append([q for q in PERCENTILES if not hr.value_from_percentile(bounds, cs, num_points, p, q, report=True)[1]])
    k = min(len(r) for r in rows)
    return np.array([r[:k] for r in rows], dtype)


def build(ref, tmp):
    src = os.path.join(HERE, "histogram_ref_driver.cpp")
    exes = {}
    for tag, extra in (("plain", []), ("asan", ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"])):
        exe = os.path.join(tmp, "driver_" + tag)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math"] + extra +
                              ["-I" + os.path.join(ref, "MCMCpp"), src, "-o", exe])
        exes[tag] = exe
    return exes


def run_case(exes, tmp, name, c):
    rng = np.random.default_rng(sum(map(ord, name)))
    T = c["dtype"]
    W, P, n, sl, cb, pb = c["W"], c["P"], c["n"], c["slice"], c["cb"], c["pb"]
    steps = make_steps(rng, n, W, P, T, c["kind"])
    corner = hr.histograms(steps, cb, sl, True)
    finder = hr.histograms(steps, pb, sl, False)
    assert corner["clamped"].sum() == 0 and finder["clamped"].sum() == 0, "the input leaves the reference's range"
    vq = value_queries(finder["bounds"], finder["single"], P, T)
    pq = percentile_queries(finder["bounds"], finder["single"], finder["num_points"], P, T)
    inp = os.path.join(tmp, name + ".in")
    with open(inp, "wb") as f:
        f.write(struct.pack("9i", 0 if T == np.float64 else 1, W, P, n, sl, cb, pb, vq.shape[1], pq.shape[1]))
        f.write(steps.tobytes())
        f.write(vq.tobytes())
        f.write(pq.tobytes())
    csv_dir = os.path.join(tmp, name + "_csv")
    os.makedirs(csv_dir, exist_ok=True)
    outs = {}
    for tag, exe in exes.items():
        out = os.path.join(tmp, name + "." + tag)
        r = subprocess.run([exe, inp, out, csv_dir if c.get("csv") else "-"], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
        assert r.returncode == 0, "%s (%s): %s" % (name, tag, r.stderr[-3000:])
        outs[tag] = open(out, "rb").read()
    assert outs["plain"] == outs["asan"], name
    buf = np.frombuffer(outs["plain"], np.uint8)
    off = [0]

    def take(dt, count):
        a = np.frombuffer(buf, dt, count, off[0])
        off[0] += a.nbytes
        return a.copy()

    npairs = P * (P - 1) // 2
    z = dict(steps=steps, slice_interval=np.int32(sl), corner_bins=np.int32(cb), finder_bins=np.int32(pb),
             value_queries=vq, percentile_queries=pq)
    z["corner_bounds"] = take(T, 2 * P).reshape(P, 2)
    z["corner_single"] = take(np.int32, P * cb).reshape(P, cb)
    z["corner_pairs"] = take(np.int32, npairs * cb * cb).reshape(npairs, cb, cb)
    z["finder_bounds"] = take(T, 2 * P).reshape(P, 2)
    z["finder_single"] = take(np.int32, P * pb).reshape(P, pb)
    z["finder_cumsum"] = take(np.int32, P * (pb + 1)).reshape(P, pb + 1)
    z["num_points"] = take(np.int32, 1)[0]
    z["percentile_from_value"] = take(T, P * vq.shape[1]).reshape(P, -1)
    z["value_from_percentile"] = take(T, P * pq.shape[1]).reshape(P, -1)
    z["peak"] = take(T, P)
    z["param_minimum"] = take(T, P)
    z["param_maximum"] = take(T, P)
    assert off[0] == buf.size
    check(z)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)
    if c.get("csv"):
        files = {f: open(os.path.join(csv_dir, f)).read() for f in sorted(os.listdir(csv_dir))}
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump(files, f, indent=0, sort_keys=True)
    print("%s: %d points, %d value / %d percentile queries per parameter" % (name, z["num_points"], vq.shape[1], pq.shape[1]))


def check(z):
    """the restatement reproduces the reference's outputs bit for bit (the same checks as tests/test_histograms.py)"""
    steps, sl = z["steps"], int(z["slice_interval"])
    c = hr.histograms(steps, int(z["corner_bins"]), sl, True)
    f = hr.histograms(steps, int(z["finder_bins"]), sl, False)
    assert c["bounds"].tobytes() == z["corner_bounds"].tobytes() and f["bounds"].tobytes() == z["finder_bounds"].tobytes()
    assert (c["single"] == z["corner_single"]).all() and (c["pairs"] == z["corner_pairs"]).all()
    assert (f["single"] == z["finder_single"]).all() and (hr.cum_sums(f["single"]) == z["finder_cumsum"]).all()
    assert f["num_points"] == z["num_points"]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    with tempfile.TemporaryDirectory() as tmp:
        exes = build(ref, tmp)
        for name, c in CASES.items():
            run_case(exes, tmp, name, c)


if __name__ == "__main__":
    main()
