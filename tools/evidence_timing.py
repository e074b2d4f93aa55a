"""Time of one mcmcpp_hip_evidence_ratios_device call (the figure recorded in DESIGN.md):
    python tools/evidence_timing.py [K W D n repeats]
A dense-Gaussian ladder of K rungs, n stored steps of W walkers in device memory (iid draws from each rung's own Gaussian, made
by torch: the call's time does not depend on where the draws come from).  Prints the wall time of every repeat -- the
call returns when its results are there -- and the median."""
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
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = s.evidence_ratios(chain)
        times.append((time.perf_counter() - t0) * 1e3)
    print("K=%d W=%d D=%d n=%d: N = %d draws per rung, %.2f GB of stored steps" % (K, W, D, n, got["num_draws"], chain.numel() * 8 / 1e9))
    print("ms per call: " + " ".join("%.1f" % t for t in times) + "   median %.1f" % float(np.median(times)))
    print("log_ratio (stepping stone): " + " ".join("%.4f" % v for v in got["log_ratio"][0]) + "   analytic %.4f" % (0.5 * D * np.log(0.8)))


if __name__ == "__main__":
    main()
