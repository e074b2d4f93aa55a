"""Cost of one replica-exchange round beside one ensemble step of the same handle.  Usage: python tools/bench_replica.py [OUT]  (default profiles/replica_round_cost.txt)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmcpp_amd import capi  # noqa: E402


def ladder(calc, D, K):
    betas = [0.85 ** k for k in range(K)]
    if calc == capi.CALC_DENSE_GAUSSIAN:
        a = np.random.default_rng(1).standard_normal((D, D))
        P = a @ a.T / D + np.eye(D)
        return np.stack([(b * P).ravel() for b in betas])
    return np.stack([np.array([0.13 / b]) for b in betas])


def measure(K, W, D, calc, out):
    s = torch.cuda.Stream()
    hip = capi.HipSampler(W, D, calc, ladder(calc, D, K), seed=1, num_chains=K, hip_stream=s.cuda_stream)
    pos = np.random.default_rng(2).standard_normal((K, W, D))
    logp = np.stack([hip.calc_logp(pos[k], chain=k) for k in range(K)])
    hip.set_state(pos, logp)
    hip.run(200, save_chain=False, want_accepted=False)  # warm-up: graphs, equilibration
    for r in range(4):
        hip.exchange_chains(r)
    steps = 2000
    step_us = []
    for _ in range(5):
        hip.run(steps, save_chain=False, want_accepted=False)
        ms, launches = hip.last_run_timing()
        step_us.append(1e3 * ms / steps)
    ev, wall, frac = [], [], []
    rnd = 4
    for rep in range(5):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        n = 50
        t0 = time.perf_counter()
        e[0].record(s)
        for _ in range(n):
            r = hip.exchange_chains(rnd)
            rnd += 1
        e[1].record(s)
        e[1].synchronize()
        wall.append(1e6 * (time.perf_counter() - t0) / n)
        ev.append(1e3 * e[0].elapsed_time(e[1]) / n)
        frac.append(float(r["accepted"].sum()) / max(float(r["proposed"].sum()), 1.0))
        hip.run(20, save_chain=False, want_accepted=False)
    line = ("K=%d W=%d D=%d calc=%d: one ensemble step (all chains, last_run_timing over %d steps) %.2f us [%.2f..%.2f]; one exchange round "
            "(HIP events around 50 rounds, each ending in a synchronise) %.1f us [%.1f..%.1f], host wall %.1f us [%.1f..%.1f]; "
            "launches of a round: 1 cross (%d pairs) + 1 swap (even) / 1 cross (%d pairs) + 1 swap (odd); last swap fraction %.2f"
            % (K, W, D, calc, steps, np.median(step_us), min(step_us), max(step_us), np.median(ev), min(ev), max(ev), np.median(wall), min(wall), max(wall),
               K // 2, (K - 1) // 2, frac[-1]))
    print(line, flush=True)
    out.write(line + "\n")


if __name__ == "__main__":
    with open(sys.argv[1] if len(sys.argv) > 1 else "profiles/replica_round_cost.txt", "w") as out:
        measure(8, 16384, 32, capi.CALC_DENSE_GAUSSIAN, out)
        measure(4, 320, 2, capi.CALC_SKEWED_GAUSSIAN_2D, out)
