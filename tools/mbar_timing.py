"""Time of one mcmcpp_hip_evidence_mbar_device call next to one mcmcpp_hip_evidence_bridge_device call on the same chain (the
figures recorded in profiles/mbar_timing.txt):
    python tools/mbar_timing.py [K W D n repeats]
A dense-Gaussian ladder of K rungs, n stored steps of W walkers in device memory (iid draws from each rung's own Gaussian, made
by torch, as in tools/bridge_timing.py).  The two calls alternate; prints the wall time of every repeat -- a call returns when
its results are there -- the medians, the joint solve's passes, and both totals with their standard errors beside the closed
form.  For the split of a call into the fill of l and the passes, run it with one repeat under
`rocprofv3 --kernel-trace --stats`, in a run of its own."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch  # (before the library)
    from mcmcpp_amd import capi
    K, W, D, n, repeats = [int(v) for v in sys.argv[1:6]] if len(sys.argv) >= 6 else (8, 16384, 32, 256, 5)
    betas = np.array([0.8 ** k for k in range(K)])
    a = np.random.default_rng(1).standard_normal((D, D))
    P = a @ a.T / D + np.eye(D)
    s = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, np.stack([(b * P).ravel() for b in betas]), num_chains=K)
    chain = torch.empty((K, n, W, D), dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    to_target = torch.from_numpy(np.linalg.inv(np.linalg.cholesky(P))).cuda()  # P = L L': x = z L^-1 has precision P
    for k in range(K):
        chain[k].normal_(0.0, 1.0 / float(np.sqrt(betas[k])), generator=gen)
        chain[k] = chain[k] @ to_target
    torch.cuda.synchronize()
    s.evidence_bridge(chain), s.evidence_mbar(chain)  # (the first launches load the code objects)
    times = {"bridge": [], "mbar": []}
    got = {}
    for _ in range(repeats):
        for name, call in (("bridge", s.evidence_bridge), ("mbar", s.evidence_mbar)):
            t0 = time.perf_counter()
            got[name] = call(chain)
            times[name].append((time.perf_counter() - t0) * 1e3)
    bridge, mbar = got["bridge"], got["mbar"]
    print("K=%d W=%d D=%d n=%d: N = %d draws per rung, %.2f GB of stored steps, %.2f GB of log-posteriors"
          % (K, W, D, n, mbar["num_draws"], chain.numel() * 8 / 1e9, 8.0 * K * K * mbar["num_draws"] / 1e9))
    for name in ("bridge", "mbar"):
        print("evidence_%s_device, ms per call: " % name + " ".join("%.1f" % t for t in times[name]) + "   median %.1f" % float(np.median(times[name])))
    print("mbar passes: %d   converged: %d   bridge passes per pair: %s" % (mbar["passes"], mbar["converged"], " ".join(str(v) for v in bridge["passes"])))
    print("log_ratio bridge: " + " ".join("%.4f" % v for v in bridge["log_ratio"]) + "   analytic %.4f" % (0.5 * D * np.log(0.8)))
    print("log_ratio mbar:   " + " ".join("%.4f" % v for v in mbar["log_ratio"]))
    print("mcse bridge:      " + " ".join("%.5f" % v for v in bridge["mcse"]))
    print("mcse mbar:        " + " ".join("%.5f" % v for v in mbar["mcse"]))
    print("total bridge %.5f +- %.5f   mbar %.5f +- %.5f   analytic %.5f"
          % (bridge["log_ratio_total"], bridge["mcse_total"], mbar["log_ratio_total"], mbar["mcse_total"], 0.5 * D * (K - 1) * np.log(0.8)))
    print("ess mbar: " + " ".join("%.0f" % v for v in mbar["ess"]))


if __name__ == "__main__":
    main()
