"""The bridge estimate of the evidence ratios (mcmcpp_hip_evidence_bridge, HipSampler.evidence_bridge): Bennett's acceptance
ratio between neighbouring rungs, solved on the device, against the definition of include/mcmcpp_hip.h restated in numpy
(tests/bridge_restatement.py).

CPU: the restatement's root against g in long double at overlaps 0.99, 0.25 and 0.1; the edge rules; the layout of the whole
call; and what the estimator says of iid draws from the exact Gaussians of a ladder, where the ratio is known:
log(Z_p / Z_{p+1}) = (D / 2) log(beta_{p+1} / beta_p).

GPU (one child process, tests/bridge_device.py, under a time limit of its own): every output of the host-pointer and of the
device entry point -- passes and converged included -- equals the restatement on the log-posteriors the existing
calc_logp(pos, chain=) returned for the same draws, bit for bit.  A handle's walkers are even in number, so N = n W is even: the
tile boundary is taken at N = 1024 and N = 1026 (N = 1025 is reached by the host sum_tree of tests/test_bridge_plan.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import bridge_restatement as br
from tests import evidence_restatement as ev
from tests.bridge_device import KEYS, RATIO_KEYS
from tests.evidence_device import E_ARG, E_STATE, E_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS_BOUND = 1100 + 200 + 1

# ---- CPU: the restatement ------------------------------------------------------------------------------------------------


def _iid_pair(D, beta, N, seed):
    """u0, u1 of the pair exp(-|x|^2 / 2), exp(-beta |x|^2 / 2) from N iid draws of each"""
    rng = np.random.default_rng(seed)
    ra = (rng.standard_normal((N, D)) ** 2).sum(axis=1)
    rb = (rng.standard_normal((N, D)) ** 2).sum(axis=1) / beta
    return -0.5 * rb + 0.5 * beta * rb, -0.5 * beta * ra + 0.5 * ra


@pytest.mark.parametrize("name, D, beta", [("overlap_0.99", 8, 0.9), ("overlap_0.25", 32, 0.5), ("overlap_0.1", 8, 0.15)])
def test_restatement_root_against_long_double(name, D, beta):
    """g in long double changes sign, or is zero, between c* - delta and c* + delta, delta = 2^-39 max(1, |c*|)"""
    n, W = 256, 16
    u0, u1 = _iid_pair(D, beta, n * W, 7)
    got = br.pair(u0, u1, n, W)
    c = got["log_ratio"]
    delta = 2.0 ** -39 * max(1.0, abs(c))
    below, above = br.g_long_double(u0, u1, c - delta), br.g_long_double(u0, u1, c + delta)
    print("%s: c* = %.17g, overlap = %.4f, passes = %d, g(c* - delta) = %.3g, g(c* + delta) = %.3g" % (name, c, got["overlap"], got["passes"], below, above))
    assert abs(got["overlap"] - float(name.split("_")[1])) < 0.02
    assert below >= 0 >= above
    assert got["converged"] == 1 and 2 <= got["passes"] <= PASS_BOUND
    assert got["mcse"] > 0 and (got["ess"] >= 1.0).all() and (got["nonfinite"] == 0).all()


def test_edge_rules():
    n, W = 16, 32
    N = n * W
    u0, u1 = _iid_pair(4, 0.5, N, 3)
    base = br.pair(u0, u1, n, W)
    assert np.isfinite(base["log_ratio"]) and base["converged"] == 1
    # NaN or +inf in either direction: every figure of the pair is NaN, the counts stand
    for d in range(2):
        for bad in (np.nan, np.inf):
            v = [u0.copy(), u1.copy()]
            v[d][5] = bad
            v[d][6] = -np.inf
            got = br.pair(v[0], v[1], n, W)
            assert all(np.isnan(got[key]) for key in ("log_ratio", "mcse", "overlap")) and np.isnan(got["ess"]).all()
            assert got["passes"] == 0 and got["converged"] == 0 and got["nonfinite"].tolist() == [2 if d == 0 else 0, 2 if d == 1 else 0]
    # a u of -inf has h = 0 exactly and is counted
    v = u0.copy()
    v[[3, 100]] = -np.inf
    got = br.pair(v, u1, n, W)
    assert got["nonfinite"].tolist() == [2, 0] and got["h"][0][3] == 0.0 and got["h"][0][100] == 0.0 and np.isfinite(got["log_ratio"])
    # every u of one direction -inf: no mass is shared
    for d in range(2):
        v = [u0.copy(), u1.copy()]
        v[d][:] = -np.inf
        got = br.pair(v[0], v[1], n, W)
        assert got["overlap"] == 0.0 and np.isnan(got["log_ratio"]) and np.isnan(got["mcse"]) and np.isnan(got["ess"]).all()
        assert got["converged"] == 1 and got["passes"] <= PASS_BOUND and got["nonfinite"][d] == N
    # disjoint rungs: each rung's draws have no weight under the other at double precision
    got = br.pair(np.full(N, -2000.0), np.full(N, -3000.0), n, W)
    assert got["overlap"] == 0.0 and np.isnan(got["log_ratio"]) and got["passes"] == 2 and got["converged"] == 1
    # identical rungs: the root is +-0 and the overlap 1
    for zero in (0.0, -0.0):
        got = br.pair(np.full(N, zero), np.full(N, zero), n, W)
        assert got["log_ratio"] == 0.0 and got["overlap"] == 1.0 and got["mcse"] == 0.0 and got["passes"] == 2 and got["converged"] == 1
    # rungs that differ by a constant factor: u0 = 2 = -u1, the root is 2 and the overlap 1
    got = br.pair(np.full(N, 2.0), np.full(N, -2.0), n, W)
    assert abs(got["log_ratio"] - 2.0) <= 2.0 ** -39 * 2.0 and abs(got["overlap"] - 1.0) < 1e-9 and got["converged"] == 1


def test_whole_call_layout_and_totals():
    """pairs in ascending p; ess and nonfinite [2][K - 1]; a NaN in rung 1's draws reaches pairs 0 and 1 and nothing else"""
    K, n, W = 4, 8, 16
    rng = np.random.default_rng(3)
    own, lower, upper = (rng.standard_normal((K, n, W)) for _ in range(3))
    got = br.evidence_bridge(own, lower, upper)
    for p in range(K - 1):
        one = br.pair((lower[p + 1] - own[p + 1]).ravel(), (upper[p] - own[p]).ravel(), n, W)
        assert got["log_ratio"][p] == one["log_ratio"] and got["mcse"][p] == one["mcse"] and got["overlap"][p] == one["overlap"]
        assert (got["ess"][:, p] == one["ess"]).all() and got["passes"][p] == one["passes"]
    assert got["log_ratio_total"] == ((0.0 + got["log_ratio"][0]) + got["log_ratio"][1]) + got["log_ratio"][2]
    assert got["mcse_total"] == np.sqrt(((0.0 + got["mcse"][0] ** 2) + got["mcse"][1] ** 2) + got["mcse"][2] ** 2)
    assert got["num_draws"] == n * W
    own2 = own.copy()
    own2[1, 2, 3] = np.nan
    bad = br.evidence_bridge(own2, lower, upper)
    assert np.isnan(bad["log_ratio"][:2]).all() and bad["log_ratio"][2] == got["log_ratio"][2] and (bad["passes"][:2] == 0).all()
    assert bad["nonfinite"].tolist() == [[1, 0, 0], [0, 1, 0]] and np.isnan(bad["log_ratio_total"])


def test_known_answer_on_iid_gaussian_draws():
    """D = 8, beta = 0.5, N = 4096, numpy seed 7: |bridge - (D / 2) ln beta| <= 4 mcse.  With this seed the restatement gives
    c* = -2.77755 against -2.77259, mcse 0.0156: z = -0.32."""
    D, beta, n, W = 8, 0.5, 256, 16
    u0, u1 = _iid_pair(D, beta, n * W, 7)
    got = br.pair(u0, u1, n, W)
    truth = 0.5 * D * np.log(beta)
    print("bridge = %.6f, truth = %.6f, mcse = %.4g, z = %.2f, overlap = %.4f, ess = %s" % (got["log_ratio"], truth, got["mcse"], (got["log_ratio"] - truth) / got["mcse"],
                                                                                             got["overlap"], got["ess"]))
    assert abs(got["log_ratio"] - truth) <= 4.0 * got["mcse"]
    assert got["converged"] == 1 and 0.5 * n * W <= got["ess"].min() and got["ess"].max() <= 2.0 * n * W


def test_the_bridge_where_both_importance_directions_fail():
    """D = 64, beta = 0.25 (the issue's table): each importance direction is off by several units, the bridge by far less"""
    n, W = 256, 16
    u0, u1 = _iid_pair(64, 0.25, n * W, 7)
    truth = 32.0 * np.log(0.25)
    stone, reverse = ev.direction(u0, n, W)["log_ratio"], -ev.direction(u1, n, W)["log_ratio"]
    bridge = br.pair(u0, u1, n, W)["log_ratio"]
    print("truth %.3f stepping stone %.3f reverse %.3f bridge %.3f" % (truth, stone, reverse, bridge))
    assert abs(bridge - truth) < 0.5 * min(abs(stone - truth), abs(reverse - truth))


# ---- CPU: the interface ------------------------------------------------------------------------------------------------------


def test_entry_points_need_a_handle_and_are_declared_as_c99(tmp_path):
    capi.build_library()
    L = capi.lib()
    ten = [None] * 10
    assert L.mcmcpp_hip_evidence_bridge(None, None, 8, 1, *ten) == E_ARG
    assert L.mcmcpp_hip_evidence_bridge_device(None, None, 0, 8, 1, *ten) == E_ARG
    assert "mcmcpp_hip_evidence_bridge" in capi.EXPORTS and "mcmcpp_hip_evidence_bridge_device" in capi.EXPORTS
    assert L.mcmcpp_hip_abi_version() == 2
    src = tmp_path / "bridge.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int bridge(mcmcpp_hip_sampler* h, const void* const* steps, const void* dev, double* lr, int64_t* passes, int64_t* draws)\n'
                   '{\n'
                   '    int rc = mcmcpp_hip_evidence_bridge(h, steps, 100, 1, lr, 0, 0, 0, passes, 0, 0, 0, 0, draws);\n'
                   '    return rc ? rc : mcmcpp_hip_evidence_bridge_device(h, dev, 0, 100, 1, lr, 0, 0, 0, passes, 0, 0, 0, 0, draws);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "bridge.o")])


# ---- GPU: bits against the restatement --------------------------------------------------------------------------------------

DENSE3 = dict(dtype="f64", calc="dense", K=3, n=40, W=64, D=4, betas=[1.0, 0.5, 0.25], seed=2)
CASES = {
    "n32": dict(dtype="f64", calc="dense", K=2, n=4, W=8, D=2, betas=[1.0, 0.5]),  # a single short tile; the smallest n
    "n1024": dict(dtype="f64", calc="dense", K=2, n=16, W=64, D=2, betas=[1.0, 0.6]),  # one whole tile
    "n1026": dict(dtype="f64", calc="dense", K=2, n=19, W=54, D=2, betas=[1.0, 0.6]),  # a tile and one lane of the next
    "k3": DENSE3,  # N = 2560: two tiles and a half
    "three_slices": dict(dtype="f32", calc="rosen", K=2, n=2100, W=64, D=3, betas=[1.0, 0.7]),  # rows of 12 bytes; N = 134 400: 132 tiles
    "k16": dict(dtype="f64", calc="dense", K=16, n=8, W=8, D=2),  # 15 pairs; the direction-1 buffers take turns
    "iso": dict(dtype="f64", calc="iso", K=2, n=6, W=8, D=3),  # every u = 0
    # the uploads take several chunks of a size that does not divide n: a step is 2 KiB, 1 MiB holds 512; N = 83 200: two slices
    "k3_chunked": dict(DENSE3, n=1300, W=64, chunk_mb=1, device=False),
    "k3_one_chunk": dict(DENSE3, n=1300, W=64),
    "room": dict(DENSE3, place="room", host=False),  # rungs more than n steps apart
    "burn_slice3": dict(DENSE3, place="burn", burn=7, slice=3),  # behind a burn-in, every third step (14 used)
    "nan": dict(DENSE3, nan=1),
    "overflow": dict(dtype="f32", calc="dense", identity=1, K=2, n=6, W=10, D=4, betas=[1.0, 1e-4], overflow=1),
    "outside": dict(dtype="f32", calc="dense", identity=1, K=2, n=6, W=10, D=4, betas=[1.0, 1e-4], outside=1),
    "steep": dict(dtype="f64", calc="dense", identity=1, K=2, n=6, W=10, D=4, betas=[1.0, 1e-6]),
}
E2E = dict(dtype="f64", calc="dense", K=3, n=300, W=32, D=4, betas=[1.0, 0.7, 0.49], burn=50)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bridge") / "device.npz")
    spec = dict(cases=CASES, e2e=E2E, refusals=True)
    r = subprocess.run([sys.executable, "-m", "tests.bridge_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


_restated_cache = {}


def _restated(device, name, sl=1, first=0):
    key = (name, sl, first)
    if key not in _restated_cache:
        own, lower, upper = (device["%s/logp_%s" % (name, k)][:, first::sl] for k in ("own", "lower", "upper"))
        _restated_cache[key] = br.evidence_bridge(own, lower, upper)
    return _restated_cache[key]


def _assert_bits(got, want, what):
    a, b = np.asarray(got), np.asarray(want)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b, err_msg=what)


def _assert_all(device, prefix, want, what):
    for key in KEYS:
        _assert_bits(device["%s_%s" % (prefix, key)], want[key], "%s %s" % (what, key))
    assert device[prefix + "_num_draws"] == want["num_draws"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_restatement(name, device):
    spec = CASES[name]
    want = _restated(device, name, spec.get("slice", 1))
    assert want["num_draws"] == -(-spec["n"] // spec.get("slice", 1)) * spec["W"]
    for how in ("host", "dev"):
        if spec.get({"host": "host", "dev": "device"}[how], True):
            _assert_all(device, "%s/%s" % (name, how), want, "%s %s" % (name, how))


@pytest.mark.gpu
def test_the_shapes_are_what_they_are_chosen_for(device):
    assert [_restated(device, name)["num_draws"] for name in ("n32", "n1024", "n1026", "three_slices", "k3_one_chunk")] == [32, 1024, 1026, 134400, 83200]
    for name in ("n32", "n1024", "n1026", "k3", "three_slices", "k16", "k3_one_chunk"):
        want = _restated(device, name)
        assert (want["converged"] == 1).all() and (want["passes"] >= 3).all() and (want["passes"] <= PASS_BOUND).all(), name
        assert np.isfinite(want["log_ratio"]).all() and (want["overlap"] > 0).all() and (want["overlap"] <= 1).all() and (want["mcse"] > 0).all()


@pytest.mark.gpu
def test_forced_chunks_give_the_one_chunk_result(device):
    for key in KEYS:
        _assert_bits(device["k3_chunked/host_" + key], device["k3_one_chunk/host_" + key], key)
        _assert_bits(device["k3_chunked/host_" + key], device["k3_one_chunk/dev_" + key], key)


@pytest.mark.gpu
def test_identical_rungs_have_ratio_zero_and_overlap_one(device):
    for how in ("host", "dev"):
        assert device["iso/%s_log_ratio" % how].tolist() == [0.0] and device["iso/%s_overlap" % how].tolist() == [1.0]
        assert device["iso/%s_mcse" % how].tolist() == [0.0] and device["iso/%s_passes" % how].tolist() == [2] and device["iso/%s_log_ratio_total" % how] == 0.0


@pytest.mark.gpu
def test_a_nan_draw_reaches_its_two_pairs_alone(device):
    """rung 1's draws are direction 0 of pair 0 and direction 1 of pair 1: both pairs of K = 3"""
    for how in ("host", "dev"):
        for key in ("log_ratio", "mcse", "overlap", "ess"):
            assert np.isnan(device["nan/%s_%s" % (how, key)]).all()
        assert device["nan/%s_nonfinite" % how].tolist() == [[1, 0], [0, 1]] and (device["nan/%s_passes" % how] == 0).all()
        assert np.isfinite(device["k3/%s_log_ratio" % how]).all()


@pytest.mark.gpu
def test_an_overflowing_row_has_h_zero(device):
    spec = CASES["overflow"]
    n, W = spec["n"], spec["W"]
    own, lower = device["overflow/logp_own"], device["overflow/logp_lower"]
    assert lower[1, n // 3, 1] == -np.inf and np.isfinite(own[1, n // 3, 1])
    assert np.isfinite(np.delete(lower[1].ravel(), (n // 3) * W + 1)).all() and np.isfinite(own).all()
    for how in ("host", "dev"):
        assert device["overflow/%s_nonfinite" % how].tolist() == [[1], [0]]
        assert device["overflow/%s_converged" % how].tolist() == [1] and device["overflow/%s_passes" % how][0] <= PASS_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["outside", "steep"])
def test_no_shared_mass_gives_overlap_zero(device, name):
    spec = CASES[name]
    if name == "outside":  # the premise: every draw of rung 1 is outside rung 0's support, and inside its own
        assert (device["outside/logp_lower"][1] == -np.inf).all() and np.isfinite(device["outside/logp_own"]).all()
    for how in ("host", "dev"):
        assert device["%s/%s_overlap" % (name, how)].tolist() == [0.0]
        for key in ("log_ratio", "mcse", "ess"):
            assert np.isnan(device["%s/%s_%s" % (name, how, key)]).all()
        assert device["%s/%s_converged" % (name, how)].tolist() == [1]
        assert device["%s/%s_nonfinite" % (name, how)].tolist() == ([[spec["n"] * spec["W"]], [0]] if name == "outside" else [[0], [0]])


REFUSALS = [("de", E_UNSUPPORTED, "differential-evolution"), ("batch", E_UNSUPPORTED, "batch target"), ("sharded", E_UNSUPPORTED, "sharded"),
            ("communicator", E_UNSUPPORTED, "communicator"), ("owned", E_UNSUPPORTED, "caller-owned positions"),
            ("one_chain", E_ARG, "num_chains must be at least 2"), ("three_steps", E_ARG, "n >= 4"), ("three_used_steps", E_ARG, "n >= 4"),
            ("slice", E_ARG, "slice_interval >= 1"), ("null", E_ARG, "must not be NULL"), ("async", E_STATE, "asynchronous run is in progress")]


@pytest.mark.gpu
@pytest.mark.parametrize("tag, code, text", REFUSALS + [("null_step_host", E_ARG, "a step pointer is NULL"), ("stride_dev", E_ARG, "chain_stride_steps"),
                                                        ("host_pointer_dev", E_ARG, "not device memory"), ("past_the_end_dev", E_ARG, "end inside the allocation")])
def test_refusals_leave_the_outputs_untouched(device, tag, code, text):
    for t in ([tag] if tag.endswith(("_dev", "_host")) else [tag + "_dev", tag + "_host"]):
        message = str(device["refusals/%s_message" % t])
        assert device["refusals/%s_code" % t] == code and text in message, (t, message)
        assert ("evidence_bridge_device" in message) == t.endswith("_dev") and "evidence_bridge" in message
        assert device["refusals/%s_untouched" % t] == 1


@pytest.mark.gpu
def test_the_call_after_the_refusals_succeeds_without_set_state(device):
    _assert_all(device, "refusals/after", _restated(device, "refusals"), "after the refusals")
    assert device["refusals/all_null_code"] == 0


@pytest.mark.gpu
def test_end_to_end_on_a_tempered_run(device):
    """run_tempered(device=True), K = 3, dense, D = 4, W = 32, 300 stored steps: evidence_bridge on the tensor in place, whole and
    behind a burn-in, equals the restatement bit for bit; evidence_ratios on the same tensor still equals its own restatement.
    No statistical gate on the code's own chain."""
    assert device["e2e/state_untouched"] == 1 and device["e2e/accepted"].sum() > 0
    for prefix, first in (("e2e/dev", 0), ("e2e/burn", E2E["burn"])):
        want = _restated(device, "e2e", first=first)
        _assert_all(device, prefix, want, prefix)
        assert (want["converged"] == 1).all() and (want["overlap"] > 0.1).all() and (want["nonfinite"] == 0).all()
    own, lower, upper = (device["e2e/logp_" + key] for key in ("own", "lower", "upper"))
    ratios = ev.evidence_ratios(own, lower, upper)
    for key in RATIO_KEYS:
        _assert_bits(device["e2e/ratios_" + key], ratios[key], "evidence_ratios " + key)
