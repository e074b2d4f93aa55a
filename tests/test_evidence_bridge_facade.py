"""ReplicaExchangeSampler::evidenceBridge (include/MCMCpp/ReplicaExchangeSampler.h) and examples/gaussian_evidence_bridge.cpp.
CPU: both programs compile and link against the facade with -Werror.  GPU: the example runs, its table parses, and the bridge
estimate of every pair is within four of its own standard errors of the analytic ratio (the run is seeded: one outcome);
and evidenceBridge of tests/cpp/evidence_bridge_facade.cpp equals, bit for bit, what the C entry point returns for the same
chains through a handle with the same ladder."""
import math
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests.test_histograms import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _programs():
    return (_compile(os.path.join(ROOT, "examples", "gaussian_evidence_bridge.cpp"), "gaussian_evidence_bridge"),
            _compile(os.path.join(ROOT, "tests", "cpp", "evidence_bridge_facade.cpp"), "evidence_bridge_facade"))


def test_programs_with_the_facade_compile_and_link():
    for exe in _programs():
        assert os.access(exe, os.X_OK)


@pytest.mark.gpu
def test_example_runs_and_the_bridge_is_within_four_mcse_of_the_analytic_ratio():
    exe = _programs()[0]
    steps = 200
    r = subprocess.run([exe, str(steps), "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = r.stdout.strip().split("\n")
    head = lines[0].split()
    assert int(head[0]) == steps + 1 and int(head[5]) == steps // 4  # (the initial placement is stored step 0)
    N = int(lines[0].split(",")[2].split()[0])
    assert N == (steps + 1 - steps // 5) * 256
    rows = [line.split() for line in lines[2:]]
    pairs = [row for row in rows if row[0] == "pair"]
    assert [row[1] for row in pairs] == ["0-1", "1-2"]
    for row in pairs:
        stone, reverse, bridge, mcse, overlap, passes, analytic = (float(v) for v in row[2:9])
        assert analytic == pytest.approx(2.0 * math.log(0.7), abs=1e-6)
        assert 0.0 < overlap <= 1.0 and mcse > 0 and 3 <= passes <= 1301
        assert abs(bridge - analytic) <= 4.0 * mcse + 1e-8 and row[9] == "yes"  # (nine decimals are printed)
        assert abs(stone - analytic) < 0.5 and abs(reverse - analytic) < 0.5
    total = [row for row in rows if row[0] == "total"][0]
    assert float(total[3]) == pytest.approx(sum(float(p[4]) for p in pairs), abs=1e-8) and float(total[5]) == pytest.approx(4.0 * math.log(0.7), abs=1e-6)


@pytest.mark.gpu
def test_evidence_bridge_equals_the_c_call_on_the_same_chains(tmp_path):
    exe = _programs()[1]
    out = tmp_path / "facade.bin"
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    v = np.fromfile(str(out), np.float64)
    K, n, W, D, burn, sl, draws = (int(x) for x in v[:7])
    assert (K, n, W, D) == (3, 121, 32, 4)
    at = 7
    P = v[at:at + K * D * D].reshape(K, D * D)
    at += K * D * D
    chains = v[at:at + K * n * W * D].reshape(K, n, W, D)
    at += chains.size
    got = {}
    for key in ("log_ratio", "mcse", "overlap", "passes", "converged"):
        got[key] = v[at:at + K - 1]
        at += K - 1
    for key in ("ess", "nonfinite"):
        got[key] = v[at:at + 2 * (K - 1)].reshape(2, K - 1)
        at += 2 * (K - 1)
    got["log_ratio_total"], got["mcse_total"] = v[at], v[at + 1]
    assert at + 2 == v.size
    s = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, P, num_chains=K)
    want = s.evidence_bridge(np.ascontiguousarray(chains[:, burn::sl]))
    assert want["num_draws"] == draws == len(range(burn, n, sl)) * W
    for key in ("log_ratio", "mcse", "overlap", "ess"):
        np.testing.assert_array_equal(got[key].view(np.uint64), want[key].view(np.uint64), err_msg=key)
    for key in ("log_ratio_total", "mcse_total"):
        assert np.float64(got[key]).view(np.uint64) == np.float64(want[key]).view(np.uint64), key
    for key in ("passes", "converged", "nonfinite"):
        np.testing.assert_array_equal(got[key].astype(np.int64), want[key])
    # the same through the call's own slice interval
    sliced = s.evidence_bridge(np.ascontiguousarray(chains[:, burn:]), slice_interval=sl)
    for key in ("log_ratio", "mcse", "overlap", "ess"):
        np.testing.assert_array_equal(sliced[key].view(np.uint64), want[key].view(np.uint64), err_msg=key)
    assert (want["converged"] == 1).all() and (want["overlap"] > 0).all() and (want["overlap"] <= 1).all() and np.isfinite(want["log_ratio"]).all()
