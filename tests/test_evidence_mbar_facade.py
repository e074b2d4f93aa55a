"""ReplicaExchangeSampler::evidenceMbar (include/MCMCpp/ReplicaExchangeSampler.h) and examples/gaussian_evidence_mbar.cpp.
CPU: both programs compile and link against the facade with -Werror.  GPU: the example runs and its table parses (no
statistical gate on the code's own chain); and evidenceMbar of tests/cpp/evidence_mbar_facade.cpp equals, bit for bit, what the
C entry point returns for the same chains through a handle with the same ladder."""
import math
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests.test_histograms import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = ("log_z", "cov", "log_ratio", "mcse", "ess")


def _programs():
    return (_compile(os.path.join(ROOT, "examples", "gaussian_evidence_mbar.cpp"), "gaussian_evidence_mbar"),
            _compile(os.path.join(ROOT, "tests", "cpp", "evidence_mbar_facade.cpp"), "evidence_mbar_facade"))


def _program():
    return _programs()[1]


def test_programs_with_the_facade_compile_and_link():
    for exe in _programs():
        assert os.access(exe, os.X_OK)


@pytest.mark.gpu
def test_example_runs_and_prints_both_totals_beside_the_closed_form():
    steps = 200
    r = subprocess.run([_programs()[0], str(steps), "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = r.stdout.strip().split("\n")
    head = lines[0].replace(",", "").split()
    assert int(head[0]) == steps + 1 and int(head[5]) == (steps + 1 - steps // 5) * 256 and 3 <= int(head[10]) <= 201 and int(head[-1]) == 1
    rows = [line.split() for line in lines[2:]]
    assert [row[1] for row in rows if row[0] == "pair"] == ["0-1", "1-2"]
    for row in rows:
        figures = [float(v) for v in row[-5:]]
        assert all(math.isfinite(v) for v in figures) and figures[1] > 0 and figures[3] > 0
        assert figures[4] == pytest.approx((4.0 if row[0] == "total" else 2.0) * math.log(0.7), abs=1e-6)
    total = [row for row in rows if row[0] == "total"][0]
    assert float(total[3]) == pytest.approx(sum(float(row[4]) for row in rows if row[0] == "pair"), abs=1e-8)  # log_z[0] is the sum of MBAR's ratios


@pytest.mark.gpu
def test_evidence_mbar_equals_the_c_call_on_the_same_chains(tmp_path):
    out = tmp_path / "facade.bin"
    r = subprocess.run([_program(), str(out)], capture_output=True, text=True, timeout=120)
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
    for key, shape in (("log_z", (K,)), ("cov", (K, K)), ("log_ratio", (K - 1,)), ("mcse", (K - 1,)), ("ess", (K,)), ("nonfinite", (K, K))):
        size = int(np.prod(shape))
        got[key] = v[at:at + size].reshape(shape)
        at += size
    got["log_ratio_total"], got["mcse_total"], got["passes"], got["converged"] = v[at:at + 4]
    assert at + 4 == v.size
    s = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, P, num_chains=K)
    want = s.evidence_mbar(np.ascontiguousarray(chains[:, burn::sl]))
    assert want["num_draws"] == draws == len(range(burn, n, sl)) * W
    for key in FLOATS:
        np.testing.assert_array_equal(got[key].view(np.uint64), want[key].view(np.uint64), err_msg=key)
    for key in ("log_ratio_total", "mcse_total"):
        assert np.float64(got[key]).view(np.uint64) == np.float64(want[key]).view(np.uint64), key
    np.testing.assert_array_equal(got["nonfinite"].astype(np.int64), want["nonfinite"])
    assert int(got["passes"]) == want["passes"] and int(got["converged"]) == want["converged"] == 1
    # the same through the call's own slice interval
    sliced = s.evidence_mbar(np.ascontiguousarray(chains[:, burn:]), slice_interval=sl)
    for key in FLOATS:
        np.testing.assert_array_equal(sliced[key].view(np.uint64), want[key].view(np.uint64), err_msg=key)
    assert np.isfinite(want["log_z"]).all() and np.isfinite(want["cov"]).all() and (want["mcse"] > 0).all()
