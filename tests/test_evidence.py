"""Evidence from a ladder (mcmcpp_hip_evidence_ratios, HipSampler.evidence_ratios): the ratios of normalising constants between
neighbouring rungs by importance weights in both directions, on the device, against the definition of include/mcmcpp_hip.h
restated in numpy (tests/evidence_restatement.py).

CPU: the restatement itself against a long-double log-sum-exp on synthetic log-posteriors; the rules for -inf, NaN, +inf, all
-inf and constant weights; and what the estimator says of iid draws from the exact Gaussians of a ladder, where the ratio is
known: log(Z_p / Z_{p+1}) = (D / 2) log(beta_{p+1} / beta_p).

GPU (one child process, tests/evidence_device.py, under a time limit of its own): every output of the host-pointer and of the
device entry point equals the restatement on the log-posteriors the existing calc_logp(pos, chain=) returned for the same
draws, bit for bit.

Measured on the CPU (test_restatement_against_long_double prints them), in units of 2^-52 max(1, |lme|): |lme - long double| is
3.1 (one slice, lme = -0.86), 0.33 (three slices, one draw with nearly all the weight, lme = 32.2) and 1.8 (61 slices,
N = 65 600).  The bar is LME_UNITS = 8: two and a half times the worst.  It does not grow with N: the fixed summation shape
keeps every partial sum short, and the error of S1 enters the logarithm relative to S1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import evidence_restatement as ev
from tests.evidence_device import E_ARG, E_STATE, E_UNSUPPORTED, KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LME_UNITS = 8


def _lme_bar(lme):
    return LME_UNITS * 2.0 ** -52 * max(1.0, abs(float(lme)))

# ---- CPU: the restatement ------------------------------------------------------------------------------------------------


def _synthetic(name):
    rng = np.random.default_rng(11)
    n, W = {"one_slice": (16, 32), "three_slices": (40, 64), "61_slices": (1025, 64)}[name]
    u = rng.standard_normal(n * W) * 2.0 - 3.0
    if name == "three_slices":
        u[7] = 40.0  # one draw carries nearly all the weight
    return u, n, W


@pytest.mark.parametrize("name", ["one_slice", "three_slices", "61_slices"])
def test_restatement_against_long_double(name):
    u, n, W = _synthetic(name)
    got = ev.direction(u, n, W)
    want = ev.log_mean_exp_long_double(u)
    err = abs(np.longdouble(got["log_ratio"]) - want)
    print("%s: lme = %.17g, |lme - long double| = %.3g = %.2f units" % (name, got["log_ratio"], float(err), float(err) / _lme_bar(got["log_ratio"]) * LME_UNITS))
    assert err <= _lme_bar(got["log_ratio"])
    e = np.exp(u.astype(np.longdouble) - u.max())
    kish = e.sum() ** 2 / (e * e).sum()
    assert abs(got["kish"] - kish) <= 1e-13 * kish
    assert got["max_u"] == u.max() and got["nonfinite"] == 0
    # the invariants of the definition
    assert got["max_u"] - np.log(n * W) <= got["log_ratio"] <= got["max_u"] and 1.0 <= got["kish"] <= n * W
    assert got["mcse"] > 0 and 1.0 <= got["ess"]


def test_nonfinite_rules():
    u, n, W = _synthetic("one_slice")
    base = ev.direction(u, n, W)
    # -inf: weight exactly 0, counted, the estimate is that of the other draws over all N
    v = u.copy()
    v[[3, 100]] = -np.inf
    got = ev.direction(v, n, W)
    assert got["nonfinite"] == 2 and got["weights"][3] == 0.0 and got["weights"][100] == 0.0
    want = ev.log_mean_exp_long_double(np.delete(u, [3, 100])) + np.log(np.longdouble(n * W - 2) / (n * W))
    assert abs(np.longdouble(got["log_ratio"]) - want) <= _lme_bar(got["log_ratio"])
    # NaN or +inf: every figure of the (d, p) is NaN, the count stands
    for bad in (np.nan, np.inf):
        v = u.copy()
        v[5] = bad
        v[6] = -np.inf
        got = ev.direction(v, n, W)
        assert got["nonfinite"] == 2 and all(np.isnan(got[key]) for key in ev.KEYS)
    # all -inf
    got = ev.direction(np.full(n * W, -np.inf), n, W)
    assert got["log_ratio"] == -np.inf and got["max_u"] == -np.inf and got["nonfinite"] == n * W
    assert all(np.isnan(got[key]) for key in ("mcse", "ess", "kish"))
    # constant weights: lme = u exactly, kish = N, mcse = 0
    for c in (0.0, -0.0, 1.25, -700.5):
        got = ev.direction(np.full(n * W, c), n, W)
        assert got["log_ratio"] == c and got["kish"] == n * W and got["mcse"] == 0.0 and got["max_u"] == c
    assert not np.signbit(ev.max_u(np.array([-0.0, 0.0, -1.0]))) and np.signbit(ev.max_u(np.array([-0.0, -0.0, -1.0])))
    assert base["nonfinite"] == 0


def test_whole_call_layout_and_totals():
    """[2][K - 1], d-major; the reverse direction negated; a NaN in rung 1's draws reaches exactly (0, 0) and (1, 1)"""
    K, n, W = 4, 8, 16
    rng = np.random.default_rng(3)
    own, lower, upper = (rng.standard_normal((K, n, W)) for _ in range(3))
    got = ev.evidence_ratios(own, lower, upper)
    for p in range(K - 1):
        d0 = ev.direction((lower[p + 1] - own[p + 1]).ravel(), n, W)
        d1 = ev.direction((upper[p] - own[p]).ravel(), n, W)
        assert got["log_ratio"][0, p] == d0["log_ratio"] and got["log_ratio"][1, p] == -d1["log_ratio"]
        assert got["mcse"][0, p] == d0["mcse"] and got["ess"][1, p] == d1["ess"] and got["kish"][1, p] == d1["kish"]
    assert got["log_ratio_total"][0] == ((0.0 + got["log_ratio"][0, 0]) + got["log_ratio"][0, 1]) + got["log_ratio"][0, 2]
    assert got["mcse_total"][1] == np.sqrt(((0.0 + got["mcse"][1, 0] ** 2) + got["mcse"][1, 1] ** 2) + got["mcse"][1, 2] ** 2)
    assert got["num_draws"] == n * W
    own2 = own.copy()
    own2[1, 2, 3] = np.nan
    bad = ev.evidence_ratios(own2, lower, upper)
    touched = np.zeros((2, K - 1), bool)
    touched[0, 0] = touched[1, 1] = True
    for key in ev.KEYS:
        assert np.isnan(bad[key][touched]).all()
        np.testing.assert_array_equal(bad[key][~touched], got[key][~touched])
    assert bad["nonfinite"][touched].tolist() == [1, 1] and np.isnan(bad["log_ratio_total"]).all()


# ---- CPU: what it says ------------------------------------------------------------------------------------------------------

SEEDS = (0, 1, 2, 3)


def _exact_ladder(betas, seed, D=4, n=400, W=16):
    """iid draws from the Gaussians N(0, 1 / beta_k) of a ladder and their log-posteriors -beta |x|^2 / 2, in numpy"""
    rng = np.random.default_rng(seed)
    K = len(betas)
    x = rng.standard_normal((K, n, W, D)) / np.sqrt(np.array(betas)).reshape(K, 1, 1, 1)
    r2 = (x * x).sum(axis=-1)
    own = np.stack([-0.5 * betas[k] * r2[k] for k in range(K)])
    lower = np.stack([-0.5 * betas[max(k - 1, 0)] * r2[k] for k in range(K)])
    upper = np.stack([-0.5 * betas[min(k + 1, K - 1)] * r2[k] for k in range(K)])
    return ev.evidence_ratios(own, lower, upper)


@pytest.mark.parametrize("seed", SEEDS)
def test_what_the_stepping_stone_direction_says(seed):
    """The ladder (1, 0.5, 0.25) at D = 4, n = 400, W = 16: log(Z_p / Z_{p+1}) = 2 log 0.5.  The stepping-stone direction must be
    within 4 mcse.  With the restatement's own ess (the draws are iid: it is near N) the |z| of the seeds fixed here are, pair 0
    and pair 1: seed 0: 0.54, 1.30; seed 1: 0.98, 0.74; seed 2: 0.84, 0.37; seed 3: 0.33, 0.94
    (ess 5840 .. 6548 of N = 6400; Kish's size 3569 .. 3639, and 386 .. 1632 in the reverse direction)."""
    got = _exact_ladder((1.0, 0.5, 0.25), seed)
    truth = 2.0 * np.log(0.5)
    N = 400 * 16
    for p in range(2):
        z = (got["log_ratio"][0, p] - truth) / got["mcse"][0, p]
        print("seed %d pair %d: z = %.3f, mcse = %.4f, ess = %.0f, kish = %.0f, reverse kish = %.0f" % (seed, p, z, got["mcse"][0, p], got["ess"][0, p], got["kish"][0, p], got["kish"][1, p]))
        assert abs(z) <= 4.0
        assert 0.5 * N <= got["ess"][0, p] <= 2.0 * N
        # the reverse direction has infinite weight variance at ratio 0.5 (E w^2 diverges): finite, and few draws carry it: far
        # below N, and below the stepping-stone direction's own 0.56 N
        assert np.isfinite(got["log_ratio"][1, p]) and np.isfinite(got["mcse"][1, p]) and got["kish"][1, p] < N / 3
    assert abs(got["log_ratio_total"][0] - 2.0 * truth) <= 4.0 * got["mcse_total"][0]


@pytest.mark.parametrize("seed", SEEDS)
def test_what_the_reverse_direction_says_where_its_variance_is_finite(seed):
    """The ladder (1, 0.7, 0.49): ratio 0.7 > 0.5, so E w^2 is finite in the reverse direction too.  Its |z| for the seeds fixed
    here, the largest over pairs and directions: seed 0: 1.59; seed 1: 1.45; seed 2: 1.03; seed 3: 1.43."""
    got = _exact_ladder((1.0, 0.7, 0.49), seed)
    truth = 2.0 * np.log(0.7)
    for p in range(2):
        for d in range(2):
            z = (got["log_ratio"][d, p] - truth) / got["mcse"][d, p]
            print("seed %d pair %d direction %d: z = %.3f" % (seed, p, d, z))
            assert abs(z) <= 4.0


# ---- CPU: the interface ------------------------------------------------------------------------------------------------------


def test_entry_points_need_a_handle_and_are_declared_as_c99(tmp_path):
    capi.build_library()
    L = capi.lib()
    nine = [None] * 9
    assert L.mcmcpp_hip_evidence_ratios(None, None, 8, 1, *nine) == E_ARG
    assert L.mcmcpp_hip_evidence_ratios_device(None, None, 0, 8, 1, *nine) == E_ARG
    assert "mcmcpp_hip_evidence_ratios" in capi.EXPORTS and "mcmcpp_hip_evidence_ratios_device" in capi.EXPORTS
    src = tmp_path / "evidence.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int ratios(mcmcpp_hip_sampler* h, const void* const* steps, const void* dev, double* lr, int64_t* draws)\n'
                   '{\n'
                   '    int rc = mcmcpp_hip_evidence_ratios(h, steps, 100, 1, lr, 0, 0, 0, 0, 0, 0, 0, draws);\n'
                   '    return rc ? rc : mcmcpp_hip_evidence_ratios_device(h, dev, 0, 100, 1, lr, 0, 0, 0, 0, 0, 0, 0, draws);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "evidence.o")])
    text = open(os.path.join(ROOT, "mcmcpp_amd", "csrc", "evidence.hip")).read()
    assert "MCMCPP_HIP_EVIDENCE_CHUNK_MB" in text and "MCMCPP_HIP_EVIDENCE_CHUNK_MB" in open(os.path.join(ROOT, "include", "mcmcpp_hip.h")).read()


# ---- GPU: bits against the restatement --------------------------------------------------------------------------------------

DENSE3 = dict(dtype="f64", calc="dense", K=3, n=40, W=64, D=4, betas=[1.0, 0.5, 0.25], seed=2)
CASES = {
    "k2_tiny": dict(dtype="f64", calc="dense", K=2, n=4, W=6, D=2, betas=[1.0, 0.5]),  # one slice; the smallest n
    "k3_three_slices": DENSE3,  # N = 2560: two full slices and a short one
    "k2_61_slices": dict(dtype="f32", calc="rosen", K=2, n=1025, W=64, D=3, betas=[1.0, 0.7]),  # rows of 12 bytes; N = 65 600
    "k16": dict(dtype="f64", calc="dense", K=16, n=8, W=8, D=2),  # 15 pairs; every rung but the ends in two pairs
    "iso": dict(dtype="f64", calc="iso", K=2, n=6, W=8, D=3),  # every u = 0
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
    out = str(tmp_path_factory.mktemp("evidence") / "device.npz")
    spec = dict(cases=CASES, e2e=E2E, refusals=True)
    r = subprocess.run([sys.executable, "-m", "tests.evidence_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def _restated(device, name, sl=1):
    own, lower, upper = (device["%s/logp_%s" % (name, key)][:, ::sl] for key in ("own", "lower", "upper"))
    return ev.evidence_ratios(own, lower, upper)


def _assert_bits(got, want, what):
    a, b = np.asarray(got), np.asarray(want)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b, err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_restatement(name, device):
    spec = CASES[name]
    want = _restated(device, name, spec.get("slice", 1))
    for how in ("host", "dev"):
        if not spec.get({"host": "host", "dev": "device"}[how], True):
            continue
        for key in KEYS:
            _assert_bits(device["%s/%s_%s" % (name, how, key)], want[key], "%s %s %s" % (name, how, key))
        assert device["%s/%s_num_draws" % (name, how)] == want["num_draws"]


@pytest.mark.gpu
def test_forced_chunks_give_the_one_chunk_result(device):
    for key in KEYS:
        _assert_bits(device["k3_chunked/host_" + key], device["k3_one_chunk/host_" + key], key)
        _assert_bits(device["k3_chunked/host_" + key], device["k3_one_chunk/dev_" + key], key)


@pytest.mark.gpu
def test_iso_gaussian_rungs_have_ratio_zero(device):
    N = 6 * 8
    assert (device["iso/logp_own"] == device["iso/logp_upper"])[0].all() and (device["iso/logp_own"] == device["iso/logp_lower"])[1].all()
    for how in ("host", "dev"):
        assert (device["iso/%s_log_ratio" % how] == 0.0).all() and (device["iso/%s_kish" % how] == N).all() and (device["iso/%s_mcse" % how] == 0.0).all()
        assert (device["iso/%s_max_u" % how] == 0.0).all() and (device["iso/%s_log_ratio_total" % how] == 0.0).all()


@pytest.mark.gpu
def test_a_nan_draw_reaches_its_two_pairs_alone(device):
    touched = np.zeros((2, 2), bool)
    touched[0, 0] = touched[1, 1] = True  # rung 1's draws: direction 0 of pair 0, direction 1 of pair 1
    for how in ("host", "dev"):
        for key in ("log_ratio", "mcse", "ess", "kish", "max_u"):
            got = device["nan/%s_%s" % (how, key)]
            assert np.isnan(got[touched]).all() and np.isfinite(got[~touched]).all()
            _assert_bits(got[~touched], device["k3_three_slices/%s_%s" % (how, key)][~touched], key)
        assert device["nan/%s_nonfinite" % how].tolist() == [[1, 0], [0, 1]]


@pytest.mark.gpu
def test_an_overflowing_row_has_weight_zero(device):
    spec = CASES["overflow"]
    n, W = spec["n"], spec["W"]
    # the premise, from the calc_logp values: the row overflows under rung 0's matrix and not under rung 1's
    own, lower = device["overflow/logp_own"], device["overflow/logp_lower"]
    assert lower[1, n // 3, 1] == -np.inf and np.isfinite(own[1, n // 3, 1])
    assert np.isfinite(np.delete(lower[1].ravel(), (n // 3) * W + 1)).all() and np.isfinite(own).all()
    for how in ("host", "dev"):
        assert device["overflow/%s_nonfinite" % how].tolist() == [[1], [0]]
        assert np.isfinite(device["overflow/%s_log_ratio" % how]).all()


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
        assert ("evidence_ratios_device" in message) == t.endswith("_dev") and "evidence_ratios" in message
        assert device["refusals/%s_untouched" % t] == 1


@pytest.mark.gpu
def test_the_call_after_the_refusals_succeeds_without_set_state(device):
    want = _restated(device, "refusals")
    for key in KEYS:
        _assert_bits(device["refusals/after_" + key], want[key], key)


@pytest.mark.gpu
def test_end_to_end_on_a_tempered_run(device):
    """run_tempered(device=True), K = 3, dense, D = 4, W = 32, 300 stored steps: the host-pointer entry, the device entry and the
    restatement give equal bits, on the whole tensor and on a view behind a burn-in; the invariants of the definition hold.  No
    statistical gate on the code's own chain."""
    own, lower, upper = (device["e2e/logp_" + key] for key in ("own", "lower", "upper"))
    assert device["e2e/state_untouched"] == 1 and device["e2e/accepted"].sum() > 0
    for tag, first in (("all", 0), ("burn", E2E["burn"])):
        want = ev.evidence_ratios(own[:, first:], lower[:, first:], upper[:, first:])
        N = (E2E["n"] - first) * E2E["W"]
        for how in ("dev", "host"):
            for key in KEYS:
                _assert_bits(device["e2e/%s_%s_%s" % (tag, how, key)], want[key], "%s %s %s" % (tag, how, key))
            assert device["e2e/%s_%s_num_draws" % (tag, how)] == N
        lme = np.stack([want["log_ratio"][0], -want["log_ratio"][1]])
        assert (want["max_u"] - np.log(N) <= lme).all() and (lme <= want["max_u"]).all()
        assert (1.0 <= want["kish"]).all() and (want["kish"] <= N).all() and (want["nonfinite"] == 0).all()
