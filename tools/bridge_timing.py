"""Time of one mcmcpp_hip_evidence_bridge_device call next to one mcmcpp_hip_evidence_ratios_device call on the same chain (the
figures recorded in DESIGN.md and profiles/bridge_timing.txt):
    python tools/bridge_timing.py [K W D n repeats]
A dense-Gaussian ladder of K rungs, n stored steps of W walkers in device memory (iid draws from each rung's own Gaussian, made
by torch, as in tools/evidence_timing.py).  The two calls alternate; prints the wall time of every repeat -- a call returns when
its results are there -- the medians, and the solver's passes per pair.  For the time of one bridge_pass_kernel launch next to
one evidence_weights_kernel launch, run it with one repeat under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
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
    s.evidence_ratios(chain), s.evidence_bridge(chain)  # (the first launches load the code objects)
    times = {"ratios": [], "bridge": []}
    for _ in range(repeats):
        for name, call in (("ratios", s.evidence_ratios), ("bridge", s.evidence_bridge)):
            t0 = time.perf_counter()
            got = call(chain)
            times[name].append((time.perf_counter() - t0) * 1e3)
            if name == "ratios":
                ratios = got
    print("K=%d W=%d D=%d n=%d: N = %d draws per rung, %.2f GB of stored steps" % (K, W, D, n, got["num_draws"], chain.numel() * 8 / 1e9))
    for name in ("ratios", "bridge"):
        print("evidence_%s_device, ms per call: " % name + " ".join("%.1f" % t for t in times[name]) + "   median %.1f" % float(np.median(times[name])))
    print("passes per pair: " + " ".join(str(v) for v in got["passes"]) + "   converged: " + " ".join(str(v) for v in got["converged"]))
    print("overlap: " + " ".join("%.4f" % v for v in got["overlap"]))
    print("log_ratio stepping stone: " + " ".join("%.4f" % v for v in ratios["log_ratio"][0]))
    print("log_ratio reverse:        " + " ".join("%.4f" % v for v in ratios["log_ratio"][1]))
    print("log_ratio bridge:         " + " ".join("%.4f" % v for v in got["log_ratio"]) + "   analytic %.4f" % (0.5 * D * np.log(0.8)))
    print("mcse bridge:              " + " ".join("%.4f" % v for v in got["mcse"]))


if __name__ == "__main__":
    main()
