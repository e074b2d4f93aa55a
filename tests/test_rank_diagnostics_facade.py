"""The facade class Analysis::RankDiagnostics (include/MCMCpp/Analysis/RankDiagnostics.h; an extension) and the example that
uses it.  CPU: both programs compile and link against include/MCMCpp with -Werror.  GPU: tests/cpp/rank_diagnostics_facade.cpp
with the chains in device memory, in pinned host memory, and in device memory with the device path switched off writes the same
bytes from all three; its figures are those of the C ABI (capi.rank_diagnostics, host and device forms, in a child process) and
of the restatement (tests/rank_restatement.py) on the chains it wrote; and the example runs."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import rank_restatement as rk
from tests.rank_device import DIAG_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "examples", "skewed_gaussian_rank_diagnostics.cpp")
FACADE = os.path.join(ROOT, "tests", "cpp", "rank_diagnostics_facade.cpp")


def _compile(src, out):
    from tests.test_histograms import _compile as compile_against_the_facade
    return compile_against_the_facade(src, out)


def test_programs_with_the_facade_class_compile_and_link():
    _compile(EXAMPLE, "skewed_gaussian_rank_diagnostics")
    _compile(FACADE, "rank_diagnostics_facade")


def _read_facade(raw):
    K, W, P, n, sl, split = struct.unpack_from("6i", raw, 0)
    off = [24]

    def take(count, dt=np.float64):
        a = np.frombuffer(raw, dt, count, off[0])
        off[0] += a.nbytes
        return a

    chains = take(K * n * W * P).reshape(K, n, W, P)
    got = {key: take(P, np.int64 if key.startswith("closed") else np.float64) for key in DIAG_KEYS}
    got["sequence_length"], got["num_sequences"] = (int(v) for v in take(2, np.int64))
    assert off[0] == len(raw)
    return chains, sl, split, got


@pytest.mark.gpu
def test_facade_class_on_device_pinned_and_downloaded_chains(tmp_path):
    exe = _compile(FACADE, "rank_diagnostics_facade")
    runs = {}
    for tag, env in (("device", dict(MCMCPP_CHAIN_MEMORY="device")), ("pinned", dict(MCMCPP_CHAIN_MEMORY="pinned")), ("heap", dict(MCMCPP_CHAIN_MEMORY="heap")),
                     ("downloaded", dict(MCMCPP_CHAIN_MEMORY="device", MCMCPP_DEVICE_ANALYSIS="0"))):
        outp = tmp_path / (tag + ".bin")
        e = {k: v for k, v in os.environ.items() if k not in ("MCMCPP_CHAIN_MEMORY", "MCMCPP_DEVICE_ANALYSIS")}
        r = subprocess.run([exe, str(outp)], capture_output=True, text=True, timeout=300, env=dict(e, **env))
        assert r.returncode == 0 and "rank_diagnostics_facade OK" in r.stdout, tag + r.stdout + r.stderr
        runs[tag] = (r.stdout, outp.read_bytes())
    assert runs["device"] == runs["pinned"] == runs["heap"] == runs["downloaded"]
    chains, sl, split, got = _read_facade(runs["device"][1])
    assert chains.shape == (3, 901, 64, 4) and sl == 2 and split == 1  # the initial positions and 900 steps
    # the C ABI on the same chains, in a child process under a time limit of its own
    np.save(tmp_path / "chains.npy", chains)
    out = str(tmp_path / "abi.npz")
    r = subprocess.run([sys.executable, "-m", "tests.rank_device", json.dumps(dict(chains_file=str(tmp_path / "chains.npy"), slice=sl, split=split)), out], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rank_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    abi = np.load(out)
    want = rk.rank_diagnostics(chains, True, 0, sl)
    for key in DIAG_KEYS:
        a = np.ascontiguousarray(got[key])
        for other, tag in ((abi["file/host_" + key], "C ABI, host form"), (abi["file/dev_" + key], "C ABI, device form"), (want[key], "restatement")):
            np.testing.assert_array_equal(a.view(np.uint64), np.ascontiguousarray(other).view(np.uint64), err_msg="%s: %s" % (tag, key))
    assert (got["sequence_length"], got["num_sequences"]) == (225, 3 * 2 * 64) == (want["sequence_length"], want["num_sequences"])
    assert int(abi["file/dev_sequence_length"]) == 225 and int(abi["file/host_num_sequences"]) == 384
    print("rank diagnostics of the facade's chains: rhat", got["rhat"], "bulk", got["ess_bulk"], "tail", got["ess_tail"])
    # (the chains start from a uniform cloud and keep their first steps: R-hat is near 1, not at it; measured 1.053 .. 1.056)
    N = 225 * 384
    assert (got["rhat"] > 0.9).all() and (got["rhat"] < 2.0).all() and (got["ess_bulk"] > 0).all() and (got["ess_bulk"] < N).all() and (got["ess_tail"] > 0).all()


@pytest.mark.gpu
def test_rank_diagnostics_example_runs():
    exe = _compile(EXAMPLE, "skewed_gaussian_rank_diagnostics")
    r = subprocess.run([exe, "1019"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1920 sequences of 408 steps" in r.stdout
    rows = [[float(v) for v in line.split(":")[1].split("|")] for line in r.stdout.split("\n") if line[:1] == "P" and line[1:2].isdigit()]
    assert len(rows) == 2
    for rhat, rank, folded, bulk, tail, q05, median, q95 in rows:
        assert rhat == max(rank, folded) and 0.9 < rhat < 2.0 and 0 < bulk < 2 * 1920 * 408 and 0 < tail < 2 * 1920 * 408 and q05 < median < q95
