#!/usr/bin/env python3
"""Batch targets (calc_id MCMCPP_HIP_CALC_BATCH) against the fused half-step path at 16 384 walkers x 32 params fp64,
isotropic Gaussian: us per ensemble step between device events around the run (mcmcpp_hip_last_run_timing), and wall
us per step of the whole run() call, for
  fused  the fused half-step kernel with the built-in target (MCMCPP_HIP_FULL_STEP=0)
  c      the batch path with a C callback that launches a restated isotropic kernel (tests/cpp/batch_calc.hip)
  torch  the batch path with a torch callback (pairwise halving in torch ops)
All three produce the same chain (checked here).  Prints one JSON line.  Kernel times of propose / accept come from a
separate `rocprofv3 --kernel-trace --stats` run of this script.
    STEPS=2000 python tools/bench_batch_calc.py"""
import ctypes as C
import json, os, subprocess, sys, time
import numpy as np
import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmcpp_amd import capi
from oracle import pyoracle as po

W, D = 16384, 32
steps = int(os.environ.get("STEPS", 2000))
reps = int(os.environ.get("REPS", 3))

build = os.path.join(ROOT, "tests", "cpp", "_build")
os.makedirs(build, exist_ok=True)
so = os.path.join(build, "libbatch_calc.so")
subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                       "-shared", os.path.join(ROOT, "tests", "cpp", "batch_calc.hip"), "-o", so])
L = C.CDLL(so)
L.batch_calc_create.restype = C.c_void_p
L.batch_calc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
user = L.batch_calc_create(0, 0, D, None, 0)


def torch_iso(x):
    v = x * x
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0] * -0.5


pos = po.init_positions(po.F64, W, D, salt=0)
logp = po.Oracle(W, D, po.CALC_ISO_GAUSSIAN, None).logp(pos)
os.environ["MCMCPP_HIP_FULL_STEP"] = "0"
samplers = {
    "fused": capi.HipSampler(W, D, capi.CALC_ISO_GAUSSIAN, seed=0),
    "c": capi.HipSampler(W, D, capi.CALC_BATCH, seed=0, batch_callback=(C.cast(L.batch_calc_logp, C.c_void_p).value, user)),
    "torch": capi.HipSampler(W, D, capi.CALC_BATCH, seed=0, log_prob=torch_iso),
}
res, finals = {}, {}
for name, s in samplers.items():
    s.set_state(pos, logp)
    s.run(20, save_chain=False, want_accepted=False)  # warm-up
    gpu, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.run(steps, save_chain=False, want_accepted=False)
        wall.append(time.perf_counter() - t0)
        gpu.append(s.last_run_timing()[0])
    finals[name] = s.get_state()[0]
    res[name] = {"gpu_us_per_step": min(gpu) * 1e3 / steps, "wall_us_per_step": min(wall) * 1e6 / steps}
assert np.array_equal(finals["fused"], finals["c"]) and np.array_equal(finals["fused"], finals["torch"]), "the three paths part"
print(json.dumps({
    "metric": "stretch move, %d walkers x %d params fp64, isotropic Gaussian: fused half-step path vs batch target (C / torch callback)" % (W, D),
    "value": res["c"]["gpu_us_per_step"], "unit": "us per ensemble step (C callback, device events)", "steps": steps,
    "fused_half_step": res["fused"], "batch_c_callback": res["c"], "batch_torch_callback": res["torch"],
    "bytes_per_step": {"propose": 2 * (W // 2) * (32 + 3 * 8 * D + 24), "accept_min": 2 * (W // 2) * (32 + 8 * D + 3 * 8 + 4)},
}))
