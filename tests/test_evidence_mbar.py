"""The multistate Bennett acceptance ratio (mcmcpp_hip_evidence_mbar, HipSampler.evidence_mbar): all K log-normalising constants
of a ladder in one joint solve on the device, with their covariance, against the definition of include/mcmcpp_hip.h restated in
numpy (tests/mbar_restatement.py).

CPU: for K = 2 the restatement's root is the bridge's (tests/bridge_restatement.py); a known answer on iid draws from the exact
Gaussians of a ladder, where log(Z_p / Z_q) = (D / 2) log(beta_q / beta_p); the spread of the total over 100 seeds against the
reported standard error; the invariances; the edge rules; the interface.

GPU (one child process, tests/mbar_device.py, under a time limit of its own): every output of the host-pointer and of the device
entry point -- passes and converged included -- equals the restatement on the log-posteriors the existing calc_logp(pos, chain=)
returned for the same draws, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import bridge_restatement as br
from tests import mbar_restatement as mr
from tests.evidence_device import E_ARG, E_STATE, E_UNSUPPORTED
from tests.mbar_device import BRIDGE_KEYS, KEYS
from tests.test_evidence_bridge import _iid_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = (1.0, 0.5, 0.25, 0.125)

# ---- CPU: the restatement ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("D, beta", [(8, 0.9), (32, 0.5), (8, 0.15)])
def test_two_rungs_have_the_root_of_the_bridge(D, beta):
    """For K = 2 and equal draw counts the equation S_0 = N is the bridge's S_0(c) = S_1(c).  Each solver stops within 2^-39 of
    the common root (its step rule, and one Newton step beyond): |log_ratio[0] - c*| <= 2^-36 max(1, |c*|) leaves a margin of 8."""
    n, W = 256, 16
    u0, u1 = _iid_pair(D, beta, n * W, 7)
    got = mr.mbar(mr.l_of_pair(u0, u1), n, W)
    bridge = br.pair(u0, u1, n, W)
    c = bridge["log_ratio"]
    print("D = %d, beta = %g: mbar %.17g, bridge %.17g, difference %.3g, passes %d against %d, mcse %.6g against %.6g"
          % (D, beta, got["log_ratio"][0], c, got["log_ratio"][0] - c, got["passes"], bridge["passes"], got["mcse"][0], bridge["mcse"]))
    assert abs(got["log_ratio"][0] - c) <= 2.0 ** -36 * max(1.0, abs(c))
    assert got["converged"] == 1 and got["passes"] <= mr.PASS_BOUND and got["log_ratio_total"] == got["log_z"][0] == got["log_ratio"][0]
    assert got["log_z"][1] == 0.0 and (got["cov"][1] == 0.0).all() and (got["cov"][:, 1] == 0.0).all() and got["mcse"][0] == got["mcse_total"] > 0


def test_known_answer_on_iid_gaussian_draws():
    """D = 8, beta = (1, 1/2, 1/4, 1/8), N = 4096 iid draws per rung, numpy seed 7: |total - 4 ln(1/8)| <= 4 mcse_total.  With this
    seed the restatement gives -8.29860 against -8.31777, mcse_total 0.0320: z = 0.60, in 8 passes."""
    n, W = 256, 16
    got = mr.mbar(mr.iid_ladder(8, LADDER, n * W, 7), n, W)
    truth = 4.0 * np.log(0.125)
    print("total = %.6f, truth = %.6f, mcse_total = %.4g, z = %.2f, passes = %d, ess = %s" % (got["log_ratio_total"], truth, got["mcse_total"],
                                                                                           (got["log_ratio_total"] - truth) / got["mcse_total"], got["passes"], got["ess"]))
    assert abs(got["log_ratio_total"] - truth) <= 4.0 * got["mcse_total"]
    assert got["converged"] == 1 and got["passes"] <= mr.PASS_BOUND


def _pairwise_total(l, n, W):
    """the bridge's total and mcse_total on the same draws: pair p from u0 on the draws of rung p + 1 and u1 on those of rung p"""
    K, N = l.shape[0], n * W
    total, squares = 0.0, 0.0
    for p in range(K - 1):
        own, other = slice(p * N, (p + 1) * N), slice((p + 1) * N, (p + 2) * N)
        got = br.pair(l[p, other] - l[p + 1, other], l[p + 1, own] - l[p, own], n, W)
        total, squares = total + got["log_ratio"], squares + got["mcse"] ** 2
    return total, np.sqrt(squares)


def test_the_reported_error_is_the_spread_over_seeds():
    """Same ladder, N = 1024, seeds 0 .. 99: the standard deviation of log_ratio_total over the seeds divided by the mean
    mcse_total lies in [0.8, 1.25] (the sd of an sd over 100 seeds is about 7 %).  The restatement gives 1.09; the pairwise
    bridge's total, printed and not asserted, has a spread well above its own mcse_total."""
    n, W = 64, 16
    totals, errors, pair_totals, pair_errors = [], [], [], []
    for seed in range(100):
        l = mr.iid_ladder(8, LADDER, n * W, seed)
        got = mr.mbar(l, n, W)
        assert got["converged"] == 1
        totals.append(got["log_ratio_total"])
        errors.append(got["mcse_total"])
        t, e = _pairwise_total(l, n, W)
        pair_totals.append(t)
        pair_errors.append(e)
    ratio = np.std(totals) / np.mean(errors)
    print("mbar: spread %.5f / mean mcse_total %.5f = %.3f; pairwise bridge: spread %.5f / mean mcse_total %.5f = %.3f"
          % (np.std(totals), np.mean(errors), ratio, np.std(pair_totals), np.mean(pair_errors), np.std(pair_totals) / np.mean(pair_errors)))
    assert 0.8 <= ratio <= 1.25


def test_invariances():
    """each within 2^-36 max(1, |zeta|)"""
    n, W = 32, 16
    N = n * W
    l = mr.iid_ladder(4, (1.0, 0.6, 0.3), N, 11)
    K = l.shape[0]
    base = mr.mbar(l, n, W)
    tol = 2.0 ** -36 * max(1.0, np.abs(base["log_z"]).max())
    # a constant c_k added to every l[k][.] moves zeta_k - zeta_{K-1} by c_k - c_{K-1}
    c = np.array([3.5, -120.25, 40.0])
    moved = mr.mbar(l + c.reshape(K, 1), n, W)
    assert moved["converged"] == 1 and np.abs((moved["log_z"] - base["log_z"]) - (c - c[-1])).max() <= 2.0 ** -36 * max(1.0, np.abs(moved["log_z"]).max())
    # the rungs in reverse order: log_ratio negated and reversed
    back = l[::-1].reshape(K, K, N)[:, ::-1].reshape(K, K * N)
    got = mr.mbar(back, n, W)
    assert got["converged"] == 1 and np.abs(got["log_ratio"] + base["log_ratio"][::-1]).max() <= tol
    assert np.abs(got["mcse"] - base["mcse"][::-1]).max() <= 1e-6 * base["mcse"].max()


def test_edge_rules():
    n, W = 16, 8
    N = n * W
    l = mr.iid_ladder(4, (1.0, 0.5, 0.25), N, 3)
    K = l.shape[0]
    base = mr.mbar(l, n, W)
    assert np.isfinite(base["log_z"]).all() and base["converged"] == 1 and (base["nonfinite"] == 0).all() and base["num_draws"] == N
    # NaN or +inf in one cell: everything is NaN, no pass is made, the counts stand
    for bad in (np.nan, np.inf):
        v = l.copy()
        v[2, N + 5] = bad  # a draw of rung 1 under chain 2
        v[0, 2 * N + 7] = -np.inf
        got = mr.mbar(v, n, W)
        for key in mr.FLOAT_KEYS:
            assert np.isnan(got[key]).all(), key
        assert got["passes"] == 0 and got["converged"] == 0
        assert got["nonfinite"].tolist() == [[0, 0, 0], [0, 0, 1], [1, 0, 0]]
    # -inf cells have weight 0, are counted, and the result stays finite
    v = l.copy()
    v[0, [N + 3, 2 * N + 100]] = -np.inf
    v[:, 9] = -np.inf  # a draw outside every rung's support: every weight +0
    got = mr.mbar(v, n, W)
    assert got["nonfinite"].tolist() == [[1, 1, 1], [1, 0, 0], [1, 0, 0]] and np.isfinite(got["log_z"]).all() and np.isfinite(got["cov"]).all()
    assert got["w"][0, N + 3] == 0.0 and got["w"][0, 2 * N + 100] == 0.0 and (got["w"][:, 9] == 0.0).all() and got["converged"] == 1
    # identical rungs: zeta = +0 exactly, mcse = 0, two passes
    for K2 in (2, 4):
        got = mr.mbar(np.zeros((K2, K2 * N)), n, W)
        assert (got["log_z"] == 0.0).all() and not np.signbit(got["log_z"]).any() and (got["mcse"] == 0.0).all() and got["mcse_total"] == 0.0
        assert got["passes"] == 2 and got["converged"] == 1 and (got["cov"] == 0.0).all()
    # disjoint rungs: no draw has weight under the other rung at double precision
    v = np.zeros((2, 2 * N))
    v[1, :N], v[0, N:] = -3000.0, -2000.0
    got = mr.mbar(v, n, W)
    for key in mr.FLOAT_KEYS:
        assert np.isnan(got[key]).all(), key
    assert got["converged"] == 1 and got["passes"] == 1 and (got["nonfinite"] == 0).all()


# ---- CPU: the interface ------------------------------------------------------------------------------------------------------


def test_entry_points_need_a_handle_and_are_declared_as_c99(tmp_path):
    capi.build_library()
    L = capi.lib()
    eleven = [None] * 11
    assert L.mcmcpp_hip_evidence_mbar(None, None, 8, 1, *eleven) == E_ARG
    assert L.mcmcpp_hip_evidence_mbar_device(None, None, 0, 8, 1, *eleven) == E_ARG
    assert "mcmcpp_hip_evidence_mbar" in capi.EXPORTS and "mcmcpp_hip_evidence_mbar_device" in capi.EXPORTS
    assert L.mcmcpp_hip_abi_version() == 2
    src = tmp_path / "mbar.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int mbar(mcmcpp_hip_sampler* h, const void* const* steps, const void* dev, double* log_z, double* cov, int64_t* passes, int64_t* draws)\n'
                   '{\n'
                   '    int rc = mcmcpp_hip_evidence_mbar(h, steps, 100, 1, log_z, cov, 0, 0, 0, 0, 0, 0, passes, 0, draws);\n'
                   '    return rc ? rc : mcmcpp_hip_evidence_mbar_device(h, dev, 0, 100, 1, log_z, cov, 0, 0, 0, 0, 0, 0, passes, 0, draws);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "mbar.o")])


# ---- GPU: bits against the restatement --------------------------------------------------------------------------------------

DENSE3 = dict(dtype="f64", calc="dense", K=3, n=40, W=64, D=4, betas=[1.0, 0.5, 0.25], seed=2)
CASES = {
    "kn64": dict(dtype="f64", calc="dense", K=2, n=4, W=8, D=2, betas=[1.0, 0.5]),  # one short tile; the smallest n
    "kn1024": dict(dtype="f64", calc="dense", K=2, n=16, W=32, D=2, betas=[1.0, 0.6]),  # exactly one tile; the rung boundary at lane 128's first term
    "kn1026": dict(dtype="f64", calc="dense", K=3, n=19, W=18, D=2, betas=[1.0, 0.6, 0.36]),  # a tile and one lane; N = 342: the rungs' trees do not align
    "k3": DENSE3,  # 7680 terms
    "three_slices": dict(dtype="f32", calc="rosen", K=2, n=1050, W=64, D=3, betas=[1.0, 0.7]),  # rows of 12 bytes; K N = 134 400: three slices
    "k16": dict(dtype="f64", calc="dense", K=16, n=8, W=8, D=2),  # 152 sums a pass, a solve of order 15
    "iso": dict(dtype="f64", calc="iso", K=2, n=6, W=8, D=3),  # identical rungs
    # the uploads take several chunks of a size that does not divide n: a step is 2 KiB, 1 MiB holds 512
    "k3_chunked": dict(DENSE3, n=1300, W=64, chunk_mb=1, device=False),
    "k3_one_chunk": dict(DENSE3, n=1300, W=64),
    "room": dict(DENSE3, place="room", host=False),  # rungs more than n steps apart
    "burn_slice3": dict(DENSE3, place="burn", burn=7, slice=3),  # behind a burn-in, every third step (14 used)
    "nan": dict(DENSE3, nan=1),
    "overflow": dict(dtype="f32", calc="dense", identity=1, K=2, n=6, W=10, D=4, betas=[1.0, 1e-4], overflow=1),
}
E2E = dict(dtype="f64", calc="dense", K=3, n=300, W=32, D=4, betas=[1.0, 0.7, 0.49], burn=50)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mbar") / "device.npz")
    spec = dict(cases=CASES, e2e=E2E, refusals=True)
    r = subprocess.run([sys.executable, "-m", "tests.mbar_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


_restated_cache = {}


def _restated(device, name, sl=1, first=0):
    key = (name, sl, first)
    if key not in _restated_cache:
        logp = device[name + "/logp"][:, :, first::sl]
        _restated_cache[key] = mr.mbar(mr.from_logp(logp), logp.shape[2], logp.shape[3])
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
    terms = {name: CASES[name]["K"] * _restated(device, name)["num_draws"] for name in ("kn64", "kn1024", "kn1026", "k3", "three_slices", "k16", "k3_one_chunk")}
    assert terms == dict(kn64=64, kn1024=1024, kn1026=1026, k3=7680, three_slices=134400, k16=1024, k3_one_chunk=249600)
    for name in terms:
        want = _restated(device, name)
        assert want["converged"] == 1 and 3 <= want["passes"] <= mr.PASS_BOUND, name
        assert np.isfinite(want["log_z"]).all() and np.isfinite(want["cov"]).all() and (want["mcse"] > 0).all() and (want["nonfinite"] == 0).all(), name


@pytest.mark.gpu
def test_forced_chunks_give_the_one_chunk_result(device):
    for key in KEYS:
        _assert_bits(device["k3_chunked/host_" + key], device["k3_one_chunk/host_" + key], key)
        _assert_bits(device["k3_chunked/host_" + key], device["k3_one_chunk/dev_" + key], key)


@pytest.mark.gpu
def test_identical_rungs_have_zeta_zero(device):
    for how in ("host", "dev"):
        assert device["iso/%s_log_z" % how].tolist() == [0.0, 0.0] and not np.signbit(device["iso/%s_log_z" % how]).any()
        assert device["iso/%s_mcse" % how].tolist() == [0.0] and device["iso/%s_passes" % how] == 2 and device["iso/%s_converged" % how] == 1
        assert device["iso/%s_log_ratio_total" % how] == 0.0 and device["iso/%s_mcse_total" % how] == 0.0


@pytest.mark.gpu
def test_a_nan_draw_reaches_everything(device):
    """the draw is one of rung 1: its log-posterior is NaN under every chain's parameters"""
    for how in ("host", "dev"):
        for key in mr.FLOAT_KEYS:
            assert np.isnan(device["nan/%s_%s" % (how, key)]).all(), key
        assert device["nan/%s_nonfinite" % how].tolist() == [[0, 0, 0], [1, 1, 1], [0, 0, 0]]
        assert device["nan/%s_passes" % how] == 0 and device["nan/%s_converged" % how] == 0
        assert np.isfinite(device["k3/%s_log_z" % how]).all()


@pytest.mark.gpu
def test_an_overflowing_row_has_weight_zero(device):
    spec = CASES["overflow"]
    n, W = spec["n"], spec["W"]
    logp = device["overflow/logp"]
    assert logp[0, 1, n // 3, 1] == -np.inf and np.isfinite(logp[1, 1, n // 3, 1]) and (~np.isfinite(logp)).sum() == 1
    for how in ("host", "dev"):
        assert device["overflow/%s_nonfinite" % how].tolist() == [[0, 0], [1, 0]]
        assert device["overflow/%s_converged" % how] == 1 and device["overflow/%s_passes" % how] <= mr.PASS_BOUND and np.isfinite(device["overflow/%s_log_z" % how]).all()


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
        assert ("evidence_mbar_device" in message) == t.endswith("_dev") and "evidence_mbar" in message
        assert device["refusals/%s_untouched" % t] == 1


@pytest.mark.gpu
def test_the_call_after_the_refusals_succeeds_without_set_state(device):
    _assert_all(device, "refusals/after", _restated(device, "refusals"), "after the refusals")
    assert device["refusals/all_null_code"] == 0


@pytest.mark.gpu
def test_end_to_end_on_a_tempered_run(device):
    """run_tempered(device=True), K = 3, dense, D = 4, W = 32, 300 stored steps: evidence_mbar on the tensor in place, whole and
    behind a burn-in, equals the restatement bit for bit; evidence_bridge on the same tensor still equals its own restatement.
    No statistical gate on the code's own chain."""
    assert device["e2e/state_untouched"] == 1 and device["e2e/accepted"].sum() > 0
    for prefix, first in (("e2e/dev", 0), ("e2e/burn", E2E["burn"])):
        want = _restated(device, "e2e", first=first)
        _assert_all(device, prefix, want, prefix)
        assert want["converged"] == 1 and (want["nonfinite"] == 0).all() and np.isfinite(want["cov"]).all()
    logp = device["e2e/logp"]
    K = logp.shape[0]
    own = np.stack([logp[k, k] for k in range(K)])
    lower = np.stack([logp[k - 1, k] if k > 0 else np.zeros_like(logp[0, 0]) for k in range(K)])
    upper = np.stack([logp[k + 1, k] if k + 1 < K else np.zeros_like(logp[0, 0]) for k in range(K)])
    bridge = br.evidence_bridge(own, lower, upper)
    for key in BRIDGE_KEYS:
        _assert_bits(device["e2e/bridge_" + key], bridge[key], "evidence_bridge " + key)
