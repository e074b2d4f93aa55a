#!/usr/bin/env python3
"""What a tempered run costs per ensemble step: HipSampler.run_exchanging (the segment loop: a run, a synchronisation and a
round with its counters' clearing, copy and synchronisation per segment) against HipSampler.run_tempered (one call).  A round is
the same two launches on both sides.  DESIGN.md section 6.

K = 4 and K = 16 chains of 16 384 walkers x 32 dims, dense fp64, ladder P_k = 0.9^k P, device=True, 2 000 ensemble steps, for
exchange_every in {1, 10, 100}.  One stored step per exchange_every steps (the loop needs exchange_every to be a multiple of the
interval); with exchange_every = 1 the 2 000 steps are made in ten calls of 200 into the same tensor, so that the destination
stays at 200 stored steps (12.5 GiB with 16 chains) -- for both sides alike.  Five repetitions behind a warm-up: median, minimum
and maximum of the wall time per ensemble step.  Every (K, exchange_every, side) runs in a process of its own.

Also the GPU time of one round, between events on the handle's stream, warm:
  loop      events around exchange_chains(r): a memset, the cross launch, the swap launch, the counters' copy; the medians
            of ten even and of ten odd rounds, averaged
  tempered  (events around run_tempered(200, exchange_every=1)) - (events around run_device(200)), medians of 20 each, over
            the 200 rounds

    python tools/tempered_timing.py --out profiles/tempered_timing.txt
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


def handle(K, hip_stream=None):
    import numpy as np
    from mcmcpp_amd import capi, workloads
    P = workloads.ar1_precision(D, 0.5)
    params = np.stack([(0.9 ** k) * P for k in range(K)]).reshape(K, -1)
    s = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, params, seed=0, num_chains=K, hip_stream=hip_stream)
    pos = np.stack([workloads.init_positions(W, D, salt=k) for k in range(K)])
    s.set_state(pos, np.stack([s.calc_logp(pos[k], chain=k) for k in range(K)]))
    return s


def worker_wall(K, every, side):
    import torch  # (before the library: two HIP runtimes in one process initialise in this order only)
    sys.path.insert(0, ROOT)
    s = handle(K)
    calls = 10 if every == 1 else 1
    n_saved = STEPS // every // calls
    out = torch.empty((K, n_saved, W, D), dtype=torch.float64, device="cuda")
    run = s.run_tempered if side == "tempered" else s.run_exchanging
    state = {"round": 0}

    def once():
        for _ in range(calls):
            state["round"] = run(n_saved, interval=every, exchange_every=every, first_round=state["round"], out=out, device=True)[3]

    once()  # warm-up: allocations, graph capture
    us = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        once()
        us.append((time.perf_counter() - t0) * 1e6 / STEPS)
    assert state["round"] == (RUNS + 1) * (STEPS // every)
    print(json.dumps({"K": K, "every": every, "side": side, "us_per_step": us}))


def worker_round(K):
    import torch
    sys.path.insert(0, ROOT)
    stream = torch.cuda.Stream()
    s = handle(K, hip_stream=stream.cuda_stream)
    n = 200
    out = torch.empty((K, n, W, D), dtype=torch.float64, device="cuda")

    def gpu_ms(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    s.run_device(n, out=out, want_accepted=False)
    s.run_tempered(n, out=out, device=True)
    for r in range(4):
        s.exchange_chains(r)
    # (even and odd rounds differ in their pairs: K/2 and (K - 1)/2; a tempered run has as many of the one as of the other)
    even = [gpu_ms(lambda: s.exchange_chains(r)) * 1e3 for r in range(4, 24, 2)]
    odd = [gpu_ms(lambda: s.exchange_chains(r)) * 1e3 for r in range(5, 25, 2)]
    loop = [(statistics.median(even) + statistics.median(odd)) / 2]
    plain = [gpu_ms(lambda: s.run_device(n, out=out, want_accepted=False)) for _ in range(20)]
    tempered = [gpu_ms(lambda: s.run_tempered(n, first_round=24, out=out, device=True)) for _ in range(20)]
    print(json.dumps({"K": K, "loop_round_us": statistics.median(loop),
                      "tempered_round_us": (statistics.median(tempered) - statistics.median(plain)) * 1e3 / n,
                      "plain_step_us": statistics.median(plain) * 1e3 / n}))


def child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("worker %r failed with %d:\n%s" % (args, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs="+", default=None)
    a = ap.parse_args()
    if a.worker:
        if a.worker[0] == "round":
            return worker_round(int(a.worker[1]))
        return worker_wall(int(a.worker[1]), int(a.worker[2]), a.worker[3])
    lines = ["wall time per ensemble step, us: median (min .. max) of %d repetitions of %d steps; %d x %d dense fp64, device chain" % (RUNS, STEPS, W, D),
             "%3s %6s %28s %28s %8s" % ("K", "every", "run_exchanging (loop)", "run_tempered", "ratio")]
    for K in (4, 16):
        for every in (1, 10, 100):
            loop, temp = child("wall", K, every, "loop")["us_per_step"], child("wall", K, every, "tempered")["us_per_step"]
            fmt = lambda xs: "%9.2f (%8.2f .. %8.2f)" % (statistics.median(xs), min(xs), max(xs))  # noqa: E731
            lines.append("%3d %6d %28s %28s %8.2f" % (K, every, fmt(loop), fmt(temp), statistics.median(loop) / statistics.median(temp)))
            print(lines[-1], flush=True)
    lines += ["", "GPU time of one round, us (events on the handle's stream, warm): a round of the loop (memset, two launches, copy) | the two launches inside a run | one ensemble step"]
    for K in (4, 16):
        r = child("round", K)
        lines.append("%3d %10.1f %10.1f %10.2f" % (K, r["loop_round_us"], r["tempered_round_us"], r["plain_step_us"]))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
