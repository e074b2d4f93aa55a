"""ReplicaExchangeSampler::evidenceRatios (include/MCMCpp/ReplicaExchangeSampler.h) and examples/gaussian_evidence.cpp.
CPU: both programs compile and link against the facade with -Werror.  GPU: the example runs, its table parses and the
invariants of the definition hold in it (max_u - log N <= lme <= max_u, 1 <= kish <= N); and evidenceRatios of
tests/cpp/evidence_facade.cpp equals, bit for bit, what the C entry point returns for the same chains through a handle with
the same ladder.  No statistical gate on the code's own chain."""
import math
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests.test_histograms import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _programs():
    return (_compile(os.path.join(ROOT, "examples", "gaussian_evidence.cpp"), "gaussian_evidence"),
            _compile(os.path.join(ROOT, "tests", "cpp", "evidence_facade.cpp"), "evidence_facade"))


def test_programs_with_the_facade_compile_and_link():
    for exe in _programs():
        assert os.access(exe, os.X_OK)


@pytest.mark.gpu
def test_example_runs_and_its_table_holds_the_invariants():
    exe = _programs()[0]
    steps = 200
    r = subprocess.run([exe, str(steps), "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    head = lines[0].split()
    assert int(head[0]) == steps + 1 and int(head[5]) == steps // 4  # (the initial placement is stored step 0)
    N = int(lines[0].split(",")[2].split()[0])
    assert N == (steps + 1 - steps // 5) * 256
    rows = [line.split() for line in lines[2:]]
    pairs = [row for row in rows if row[0] == "pair"]
    assert [(row[1], row[2]) for row in pairs] == [("0-1", "stepping-stone"), ("0-1", "reverse"), ("1-2", "stepping-stone"), ("1-2", "reverse")]
    slack = 1e-8  # (nine decimals are printed)
    for row in pairs:
        estimate, mcse, ess, kish, max_u, analytic = (float(v) for v in row[3:9])
        lme = estimate if row[2] == "stepping-stone" else -estimate
        assert max_u - math.log(N) - slack <= lme <= max_u + slack
        assert 1.0 <= kish <= N + 0.05 and mcse > 0 and ess > 0
        assert analytic == pytest.approx(2.0 * math.log(0.7), abs=1e-6)
    totals = [row for row in rows if row[0] == "total"]
    assert [row[1] for row in totals] == ["stepping-stone", "reverse"]
    for d, row in enumerate(totals):
        assert float(row[2]) == pytest.approx(sum(float(p[3]) for p in pairs[d::2]), abs=1e-8) and float(row[-1]) == pytest.approx(4.0 * math.log(0.7), abs=1e-6)


@pytest.mark.gpu
def test_evidence_ratios_equals_the_c_call_on_the_same_chains(tmp_path):
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
    pairs = 2 * (K - 1)
    got = {}
    for key in ("log_ratio", "mcse", "ess", "kish", "max_u", "nonfinite"):
        got[key] = v[at:at + pairs].reshape(2, K - 1)
        at += pairs
    got["log_ratio_total"], got["mcse_total"] = v[at:at + 2], v[at + 2:at + 4]
    assert at + 4 == v.size
    s = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, P, num_chains=K)
    want = s.evidence_ratios(np.ascontiguousarray(chains[:, burn::sl]))
    assert want["num_draws"] == draws == len(range(burn, n, sl)) * W
    for key in ("log_ratio", "mcse", "ess", "kish", "max_u", "log_ratio_total", "mcse_total"):
        np.testing.assert_array_equal(got[key].view(np.uint64), want[key].view(np.uint64), err_msg=key)
    np.testing.assert_array_equal(got["nonfinite"].astype(np.int64), want["nonfinite"])
    # the same through the call's own slice interval
    sliced = s.evidence_ratios(np.ascontiguousarray(chains[:, burn:]), slice_interval=sl)
    for key in ("log_ratio", "mcse", "ess", "kish", "max_u"):
        np.testing.assert_array_equal(sliced[key].view(np.uint64), want[key].view(np.uint64), err_msg=key)
    lme = np.stack([want["log_ratio"][0], -want["log_ratio"][1]])
    assert (want["max_u"] - math.log(draws) <= lme).all() and (lme <= want["max_u"]).all() and (1.0 <= want["kish"]).all() and (want["kish"] <= draws).all()
