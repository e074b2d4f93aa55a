"""Time of one mcmcpp_hip_evidence_gaussian_device call and of its two own kernels, next to one mcmcpp_hip_evidence_bridge_device
call with K = 2 on the same draws (the figures recorded in DESIGN.md and profiles/gaussian_bridge_timing.txt):
    python tools/gaussian_bridge_timing.py [W D n repeats [out.txt [parent_library.so]]]
A dense-Gaussian target, n stored steps of W walkers in device memory (iid draws from the target, made by torch from a seed, as in
tools/bridge_timing.py); the Gaussian is fitted to a further block of as many steps.  Every repetition is two processes of their
own, one after the other: `... gaussian W D n` and `... bridge W D n`.  Each makes the draws, calls its entry point once to load
the code objects, then times one call -- wall time, a call returns when its results are there.  The first also prints the GPU time
of gaussian_rows_kernel and gaussian_log_q_kernel between the library's own events around their launches
(mcmcpp_hip_evidence_gaussian_last_timing), and the wall time of one mcmcpp_hip_calc_logp_device sweep over the N draws, of
which the call makes two.  With parent_library.so the bridge's process loads that build of the library (MCMCPP_HIP_LIB) -- the
commit before this call existed -- and this one otherwise.  The parent prints every repetition and the medians, and writes them to
out.txt where one is named."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_draws(W, D, n, torch):
    """the target's precision, and [2][n][W][D]: draws of the target and of the target flattened by 0.8"""
    a = np.random.default_rng(1).standard_normal((D, D))
    P = a @ a.T / D + np.eye(D)
    gen = torch.Generator(device="cuda").manual_seed(1)
    to_target = torch.from_numpy(np.linalg.inv(np.linalg.cholesky(P))).cuda()  # P = L L': x = z L^-1 has precision P
    chain = torch.empty((2, n, W, D), dtype=torch.float64, device="cuda")
    chain.normal_(0.0, 1.0, generator=gen)
    chain[0] = chain[0] @ to_target
    chain[1] = (chain[1] / float(np.sqrt(0.8))) @ to_target
    torch.cuda.synchronize()
    return P, chain, gen, to_target


def timed(call):
    call()  # (the first launches load the code objects)
    t0 = time.perf_counter()
    got = call()
    return (time.perf_counter() - t0) * 1e3, got


def gaussian(W, D, n):
    import torch  # (before the library)
    from mcmcpp_amd import capi
    P, chain, gen, to_target = make_draws(W, D, n, torch)
    s = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, P)
    head = torch.empty((n, W, D), dtype=torch.float64, device="cuda").normal_(0.0, 1.0, generator=gen) @ to_target
    torch.cuda.synchronize()
    m = capi.HipMoments(W, D)
    m.add_device_steps(head)
    _, mean, cov, _ = m.finish()
    m.close()
    del head
    chol = np.linalg.cholesky(cov)
    L = capi.lib()
    figures = np.zeros(3)
    passes = C.c_int64(0)
    draws = chain[0]

    def call():  # (through the C ABI: neither the proposals nor log q are asked for)
        rc = L.mcmcpp_hip_evidence_gaussian_device(s.h, 0, C.c_void_p(draws.data_ptr()), n, 1, capi._ptr(mean), capi._ptr(chol), 7, 0,
                                                   *([C.c_void_p(figures.ctypes.data + 8 * j) for j in range(3)] + [None, C.byref(passes)] + [None] * 5))
        assert rc == 0, L.mcmcpp_hip_last_error(s.h)

    wall, _ = timed(call)
    rows_ms, log_q_ms = C.c_double(0), C.c_double(0)
    L.mcmcpp_hip_evidence_gaussian_last_timing(C.byref(rows_ms), C.byref(log_q_ms))
    sweep, _ = timed(lambda: s.calc_logp_device(draws))
    truth = 0.5 * D * np.log(2.0 * np.pi) - 0.5 * np.linalg.slogdet(P)[1]
    print("RESULT %.3f %.3f %.3f %.3f %d %.6f %.6f %.6f %.6f" % (wall, rows_ms.value, log_q_ms.value, sweep, passes.value, figures[0], figures[1], figures[2], truth), flush=True)


def bridge(W, D, n):
    import torch  # (before the library)
    from mcmcpp_amd import capi
    P, chain, _, _ = make_draws(W, D, n, torch)
    ladder = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, np.stack([P.ravel(), (0.8 * P).ravel()]), num_chains=2)
    wall, got = timed(lambda: ladder.evidence_bridge(chain))
    print("RESULT %.3f %d %.6f" % (wall, got["passes"][0], got["log_ratio"][0]), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] in ("gaussian", "bridge"):
        return {"gaussian": gaussian, "bridge": bridge}[sys.argv[1]](*[int(v) for v in sys.argv[2:5]])
    W, D, n, repeats = [int(v) for v in sys.argv[1:5]] if len(sys.argv) >= 5 else (16384, 32, 256, 5)
    path = sys.argv[5] if len(sys.argv) > 5 else None
    parent = os.path.abspath(sys.argv[6]) if len(sys.argv) > 6 else None
    rows = {"gaussian": [], "bridge": []}
    for _ in range(repeats):
        for mode in ("gaussian", "bridge"):
            env = dict(os.environ)
            if mode == "bridge" and parent:
                env["MCMCPP_HIP_LIB"] = parent
            r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(W), str(D), str(n)], capture_output=True, text=True, timeout=600, env=env)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return 1
            rows[mode].append([float(v) for v in [line for line in r.stdout.split("\n") if line.startswith("RESULT")][0].split()[1:]])
    g, b = np.array(rows["gaussian"]), np.array(rows["bridge"])

    def row(name, v):
        return "%s: " % name + " ".join("%.2f" % t for t in v) + "   median %.2f" % np.median(v)

    lines = ["W=%d D=%d n=%d: N = %d draws, fp64 dense, one process per repetition and entry point, one warm-up call in front of the timed one" % (W, D, n, n * W),
             row("evidence_gaussian_device, wall ms per call", g[:, 0]),
             row("  gaussian_rows_kernel, GPU ms per call between events", g[:, 1]),
             row("  gaussian_log_q_kernel (proposals and draws), GPU ms per call between events", g[:, 2]),
             row("  one calc_logp_device sweep over the N draws, wall ms (the call makes two)", g[:, 3]),
             row("evidence_bridge_device K=2 (%s), wall ms per call" % ("the parent commit's library" if parent else "this build"), b[:, 0]),
             "passes: gaussian %d, bridge %d" % (g[0, 4], b[0, 1]),
             "log Z estimate %.6f   mcse %.6f   overlap %.6f   analytic %.6f" % tuple(g[0, 5:9])]
    print("\n".join(lines))
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
