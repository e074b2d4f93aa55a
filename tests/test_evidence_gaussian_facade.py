"""EnsembleSampler::gaussianBridgeEvidence (include/MCMCpp/Device/GaussianBridge.h) and examples/rosenbrock_evidence.cpp.
CPU: the example compiles and links against the facade with -Werror; the header-only Cholesky factor.  GPU: the example runs,
and the estimate it prints equals, bit for bit, what the Python wrapper returns for the same chain, mean, factor and seed."""
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests.test_histograms import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    return _compile(os.path.join(ROOT, "examples", "rosenbrock_evidence.cpp"), "rosenbrock_evidence")


def test_the_example_compiles_and_links():
    assert os.access(_example(), os.X_OK)


def _other_samplers():
    return _compile(os.path.join(ROOT, "tests", "cpp", "gaussian_bridge_facade.cpp"), "gaussian_bridge_facade")


def test_the_parallel_and_the_replica_exchange_sampler_reach_it_too():
    """ParallelEnsembleSampler::gaussianBridgeEvidence and ReplicaExchangeSampler::gaussianBridgeEvidence(rung, ...) are instantiated"""
    r = subprocess.run([_other_samplers()], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("compiled")


@pytest.mark.gpu
def test_the_other_samplers_on_the_gpu(tmp_path):
    """the parallel sampler follows the sequential trajectory, so its estimate is the example's at the same length, bit for bit;
    every rung of a ladder gives a finite estimate with a positive error from its own chain alone"""
    r = subprocess.run([_other_samplers(), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    got = {" ".join(line.split()[:-2]): [float(v) for v in line.split()[-2:]] for line in r.stdout.strip().split("\n")}
    e = subprocess.run([_example(), "200"], capture_output=True, text=True, timeout=120)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-2000:]
    printed = {line.rsplit(" ", 1)[0]: float(line.rsplit(" ", 1)[1]) for line in e.stdout.strip().split("\n")[1:5]}
    assert got["parallel"] == [printed["log Z estimate"], printed["mcse"]]
    for key in ("rung 0", "rung 1"):
        assert np.isfinite(got[key]).all() and got[key][1] > 0.0


def test_the_header_only_cholesky_factors_and_fails_cleanly(tmp_path):
    src = tmp_path / "chol.cpp"
    src.write_text('#include <cstdio>\n#include "Utility/Cholesky.h"\n'
                   'int main()\n{\n'
                   '    std::vector<double> a = {4.0, 9.0, 9.0, 2.0, 10.0, 9.0, -2.0, 1.0, 14.0}, l;\n'  # (what lies above the diagonal is not read)
                   '    if (!MCMC::Utility::choleskyLower(a, 3, l)) return 1;\n'
                   '    for (double v : l) std::printf("%.17g\\n", v);\n'
                   '    std::vector<double> bad = {1.0, 0.0, 2.0, 1.0};\n'  # [[1, 2], [2, 1]]: the second pivot is -3
                   '    std::vector<double> nan = {0.0 / 0.0};\n'
                   '    return (MCMC::Utility::choleskyLower(bad, 2, l) || MCMC::Utility::choleskyLower(nan, 1, l)) ? 2 : 0;\n}\n')
    exe = tmp_path / "chol"
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-div-by-zero", "-I", os.path.join(ROOT, "include", "MCMCpp"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0
    got = np.array([float(v) for v in r.stdout.split()]).reshape(3, 3)
    want = np.linalg.cholesky(np.array([[4.0, 2.0, -2.0], [2.0, 10.0, 1.0], [-2.0, 1.0, 14.0]]))
    assert np.allclose(got, want, rtol=1e-15, atol=0) and (got[np.triu_indices(3, 1)] == 0.0).all()


@pytest.mark.gpu
def test_the_example_prints_what_the_python_wrapper_returns(tmp_path):
    out = tmp_path / "evidence.bin"
    steps = 400
    r = subprocess.run([_example(), str(steps), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = r.stdout.strip().split("\n")
    printed = {line.rsplit(" ", 1)[0]: float(line.rsplit(" ", 1)[1]) for line in lines[1:5]}
    v = np.fromfile(str(out), np.float64)
    W, D, stored, burn, seed = (int(x) for x in v[:5])
    assert (W, D, stored, burn) == (64, 2, steps + 1, steps // 5)  # (the initial placement is stored step 0)
    mean, chol = v[8:8 + D], v[8 + D:8 + D + D * D].reshape(D, D)
    chain = v[8 + D + D * D:].reshape(stored, W, D)
    head = (stored - burn) // 2
    s = capi.HipSampler(W, D, capi.CALC_ROSENBROCK, np.array([1.0, 4.0, 1.0]))
    want = s.evidence_gaussian(np.ascontiguousarray(chain[burn + head:]), mean=mean, chol=chol, seed=seed)
    assert want["num_draws"] == (stored - burn - head) * W == int(lines[0].split(",")[2].split()[0])
    for key, at, name in (("log_evidence", 5, "log Z estimate"), ("mcse", 6, "mcse"), ("overlap", 7, "overlap")):
        assert np.float64(v[at]).view(np.uint64) == np.float64(want[key]).view(np.uint64), key
        assert printed[name] == float(want[key]), name  # (seventeen digits are printed)
    assert printed["log(pi / (c sqrt(b)))"] == pytest.approx(np.log(np.pi / 2.0), abs=1e-15)
    assert want["converged"] == 1 and 0.0 < want["overlap"] <= 2.0 and want["mcse"] > 0.0
    # the Gaussian is the fit of the first half behind the burn-in: the wrapper's own fit of the same steps
    fit = s.evidence_gaussian(np.ascontiguousarray(chain[burn:]), seed=seed)
    np.testing.assert_allclose(fit["mean"], mean, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(fit["chol"], chol, rtol=1e-10, atol=1e-14)
