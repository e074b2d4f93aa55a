"""The evidence of one chain's target by a bridge to a fitted Gaussian (mcmcpp_hip_evidence_gaussian,
HipSampler.evidence_gaussian), against the definition of include/mcmcpp_hip.h restated in numpy
(tests/gaussian_bridge_restatement.py).

CPU: what the estimator says of iid draws from targets whose normalising constant is known -- the project's Rosenbrock target at
D = 2, Z = pi / (c sqrt(b)), and a dense Gaussian at D = 8 --; the edge rules; the C99 prototypes.

GPU (one child process, tests/gaussian_bridge_device.py, under a time limit of its own): every output of the host-pointer and of
the device entry point -- the proposals and log q included -- equals the restatement on the log-posteriors the existing
calc_logp(pos, chain=) returned for the same draws and for the returned proposals, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import gaussian_bridge_restatement as gb
from tests.gaussian_bridge_device import E_ARG, E_STATE, E_UNSUPPORTED, KEYS, make_draws, make_gaussian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS_BOUND = 1100 + 200 + 1

# ---- CPU: known answers on the restatement ---------------------------------------------------------------------------------


def _fit_and_bridge(logp, draws, n, W, seed):
    """fit on the first half of the iid draws [2 n W][D], bridge on the second half against as many proposals"""
    N = n * W
    mean, L = gb.fit(draws[:N])
    y = draws[N:2 * N]
    x = gb.proposals(mean, L, N, seed, 0, np.float64)
    return gb.evidence_gaussian(logp(x), logp(y), x, y, mean, L, n, W)


def test_known_answer_rosenbrock():
    """(a, b, c) = (1, 4, 1), 8192 iid draws, numpy seed 3: |estimate - log(pi / (c sqrt(b)))| <= 4 mcse and overlap > 0.5.  With this
    seed the restatement gives 0.4590 against 0.4516, mcse 0.0140, overlap 0.699: z = 0.53."""
    a, b, c = 1.0, 4.0, 1.0
    n, W = 256, 16
    rng = np.random.default_rng(3)
    x0 = a + rng.standard_normal(2 * n * W) / np.sqrt(2.0 * c)
    x1 = x0 * x0 + rng.standard_normal(2 * n * W) / np.sqrt(2.0 * c * b)
    got = _fit_and_bridge(lambda v: -c * (b * (v[:, 1] - v[:, 0] ** 2) ** 2 + (a - v[:, 0]) ** 2), np.stack([x0, x1], axis=1), n, W, 1)
    truth = np.log(np.pi / (c * np.sqrt(b)))
    z = (got["log_evidence"] - truth) / got["mcse"]
    print("rosenbrock: estimate %.6f truth %.6f mcse %.4g z %.2f overlap %.4f passes %d" % (got["log_evidence"], truth, got["mcse"], z, got["overlap"], got["passes"]))
    assert abs(got["log_evidence"] - truth) <= 4.0 * got["mcse"] and got["overlap"] > 0.5
    assert got["converged"] == 1 and (got["nonfinite"] == 0).all()


def test_known_answer_dense_gaussian():
    """D = 8, precision P, 8192 iid draws, numpy seed 3: |estimate - ((D / 2) log 2 pi - (1 / 2) log det P)| <= 4 mcse and overlap > 0.95.
    With this seed the restatement gives 4.91766 against 4.91764, mcse 0.00087, overlap 0.998: z = 0.02."""
    D, n, W = 8, 256, 16
    rng = np.random.default_rng(3)
    A = rng.standard_normal((D, D))
    P = A @ A.T / D + np.eye(D)
    draws = np.linalg.solve(np.linalg.cholesky(P).T, rng.standard_normal((D, 2 * n * W))).T
    got = _fit_and_bridge(lambda v: -0.5 * np.einsum("ni,ij,nj->n", v, P, v), draws, n, W, 1)
    truth = 0.5 * D * np.log(2.0 * np.pi) - 0.5 * np.linalg.slogdet(P)[1]
    z = (got["log_evidence"] - truth) / got["mcse"]
    print("dense: estimate %.6f truth %.6f mcse %.4g z %.2f overlap %.4f passes %d" % (got["log_evidence"], truth, got["mcse"], z, got["overlap"], got["passes"]))
    assert abs(got["log_evidence"] - truth) <= 4.0 * got["mcse"] and got["overlap"] > 0.95
    assert got["converged"] == 1 and (got["nonfinite"] == 0).all()


# ---- CPU: the edges --------------------------------------------------------------------------------------------------------


def _small(seed=2, D=3, n=8, W=8):
    rng = np.random.default_rng(seed)
    N = n * W
    mean = rng.standard_normal(D)
    L = np.tril(rng.standard_normal((D, D))) * 0.2 + np.eye(D)
    y = rng.standard_normal((N, D)) + mean
    x = gb.proposals(mean, L, N, 4, 1, np.float64)
    return mean, L, x, y, n, W


def test_a_nan_draw_makes_every_figure_nan():
    mean, L, x, y, n, W = _small()
    logp = lambda v: -0.5 * (v * v).sum(axis=1)
    y[5, 1] = np.nan
    got = gb.evidence_gaussian(logp(x), logp(y), x, y, mean, L, n, W)
    assert all(np.isnan(got[key]) for key in ("log_evidence", "mcse", "overlap")) and np.isnan(got["ess"]).all()
    assert got["passes"] == 0 and got["converged"] == 0 and got["nonfinite"].tolist() == [0, 1]
    assert np.isnan(got["log_q"][1, 5]) and np.isfinite(np.delete(got["log_q"][1], 5)).all()


def test_a_proposal_outside_the_support_is_counted_and_has_h_zero():
    mean, L, x, y, n, W = _small()
    lp_x, lp_y = -0.5 * (x * x).sum(axis=1), -0.5 * (y * y).sum(axis=1)
    lp_x[[3, 17]] = -np.inf
    got = gb.evidence_gaussian(lp_x, lp_y, x, y, mean, L, n, W)
    assert got["nonfinite"].tolist() == [2, 0] and got["h"][0][3] == 0.0 and got["h"][0][17] == 0.0
    assert np.isfinite(got["log_evidence"]) and got["converged"] == 1 and 0.0 < got["overlap"] <= 1.0


def test_an_exactly_gaussian_target_with_its_own_mean_and_factor_has_overlap_one():
    """logp = log q + 3: u0 = 3 and u1 = -3 up to rounding, so c* = 3 and the overlap is 1 within 1e-9"""
    mean, L, x, y, n, W = _small()
    got = gb.evidence_gaussian(gb.log_q(x, mean, L) + 3.0, gb.log_q(y, mean, L) + 3.0, x, y, mean, L, n, W)
    assert abs(got["overlap"] - 1.0) < 1e-9 and abs(got["log_evidence"] - 3.0) < 1e-9 and got["converged"] == 1


def test_the_proposals_are_the_gaussians():
    """the restated proposals have the Gaussian's mean and covariance (N = 20000, D = 3: standard errors of 1 / sqrt(N))"""
    rng = np.random.default_rng(8)
    mean = rng.standard_normal(3)
    L = np.tril(rng.standard_normal((3, 3))) * 0.3 + np.eye(3)
    x = gb.proposals(mean, L, 20000, 1, 2, np.float64)
    assert np.abs(x.mean(axis=0) - mean).max() < 5.0 * np.sqrt((L @ L.T).max() / 20000)
    assert np.abs(np.cov(x.T) - L @ L.T).max() < 0.06
    # a later chunk of proposals is the same stream further on
    assert (gb.proposals(mean, L, 5, 1, 2, np.float32, first=100) == x[100:105].astype(np.float32)).all()


# ---- CPU: the interface ------------------------------------------------------------------------------------------------------


def test_entry_points_need_a_handle_and_are_declared_as_c99(tmp_path):
    capi.build_library()
    L = capi.lib()
    tail = [None, None, 0, 0] + [None] * 10
    assert L.mcmcpp_hip_evidence_gaussian(None, 0, None, 8, 1, *tail) == E_ARG
    assert L.mcmcpp_hip_evidence_gaussian_device(None, 0, None, 8, 1, *tail) == E_ARG
    assert "mcmcpp_hip_evidence_gaussian" in capi.EXPORTS and "mcmcpp_hip_evidence_gaussian_device" in capi.EXPORTS
    assert L.mcmcpp_hip_abi_version() == 2
    src = tmp_path / "gaussian.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int gaussian(mcmcpp_hip_sampler* h, const void* const* steps, const void* dev, const double* mean, const double* chol, double* lz, int64_t* passes,\n'
                   '             void* proposals, double* log_q)\n'
                   '{\n'
                   '    int rc = mcmcpp_hip_evidence_gaussian(h, 0, steps, 100, 1, mean, chol, 1u, 2u, lz, 0, 0, 0, passes, 0, 0, 0, proposals, log_q);\n'
                   '    return rc ? rc : mcmcpp_hip_evidence_gaussian_device(h, 0, dev, 100, 1, mean, chol, 1u, 2u, lz, 0, 0, 0, passes, 0, 0, 0, proposals, log_q);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "gaussian.o")])


# ---- GPU: bits against the restatement --------------------------------------------------------------------------------------

DENSE = dict(dtype="f64", calc="dense", K=1, n=40, W=64, D=4, betas=[1.0], seed=2)
TRIO = dict(dtype="f64", calc="dense", K=1, n=6, W=512, D=4, betas=[1.0], device=False)
CASES = {
    "n32": dict(dtype="f64", calc="dense", K=1, n=4, W=8, D=2, betas=[1.0]),  # a single short tile; the smallest n
    "n1024": dict(dtype="f64", calc="dense", K=1, n=16, W=64, D=2, betas=[1.0]),  # one whole tile
    "n1026": dict(dtype="f64", calc="dense", K=1, n=19, W=54, D=2, betas=[1.0]),  # a tile and one lane of the next
    "d1": dict(dtype="f64", calc="iso", K=1, n=5, W=6, D=1),
    "d3_f32": dict(dtype="f32", calc="rosen", K=1, n=40, W=8, D=3, betas=[1.0]),  # rows of 12 bytes; more than one block of rows
    "d17": dict(dtype="f64", calc="dense", K=1, n=5, W=36, D=17, betas=[1.0]),  # 128 rows a block: two blocks, the second short
    "d64": dict(dtype="f64", calc="dense", K=1, n=4, W=130, D=64, betas=[1.0]),  # the widest, a full factor; 64 rows a block
    "k3_chain2": dict(dtype="f64", calc="dense", K=3, chain=2, n=6, W=16, D=4, betas=[1.0, 0.5, 0.25]),
    "burn_slice3": dict(DENSE, place="burn", burn=7, slice=3),  # behind a burn-in, every third step (14 used)
    "room": dict(DENSE, place="room", host=False),
    # the uploads and the proposals take several chunks of a size that does not divide n: a step is 2 KiB, 1 MiB holds 512
    "chunked": dict(DENSE, n=1300, chunk_mb=1),
    "one_chunk": dict(DENSE, n=1300),
    "dense_trio": TRIO,
    "de_trio": dict(TRIO, handle="de"),
    "batch_trio": dict(TRIO, handle="batch"),
    "nan": dict(DENSE, nan=1, K=2, chain=1, betas=[1.0, 0.5]),
    # an fp32 identity target and a Gaussian 10^19 wide: the quadratic form of many a proposal overflows
    "overflow": dict(dtype="f32", calc="dense", identity=1, K=1, n=6, W=10, D=4, betas=[1.0], scale=1.0e19),
}
E2E = dict(dtype="f64", calc="dense", K=1, n=600, W=32, D=4, betas=[1.0], burn=100)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gaussian_bridge") / "device.npz")
    spec = dict(cases=CASES, e2e=E2E, refusals=True)
    r = subprocess.run([sys.executable, "-m", "tests.gaussian_bridge_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


_restated_cache = {}


def _restated(device, name, spec, y, mean, chol, seed, stream):
    if name not in _restated_cache:
        T = np.float32 if spec["dtype"] == "f32" else np.float64
        n, W = y.shape[0], y.shape[1]
        x = gb.proposals(mean, chol, n * W, seed, stream, T)
        want = gb.evidence_gaussian(device[name + "/logp_proposals"], device[name + "/logp_draws"], x, y, mean, chol, n, W)
        want["proposals"] = x
        _restated_cache[name] = want
    return _restated_cache[name]


def _restated_case(device, name):
    spec = CASES[name]
    mean, chol = make_gaussian(spec)
    return _restated(device, name, spec, make_draws(spec)[::spec.get("slice", 1)], mean, chol, spec.get("pseed", 9), spec.get("pstream", 4))


def _assert_bits(got, want, what):
    a, b = np.asarray(got), np.asarray(want)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    word = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    if a.dtype.kind == "f":  # (a NaN is a NaN: IEEE 754 leaves the sign and the payload of an operation's NaN open)
        a, b = np.where(np.isnan(a), a.dtype.type(np.nan), a), np.where(np.isnan(b), b.dtype.type(np.nan), b)
    np.testing.assert_array_equal(a.view(word) if a.dtype.kind == "f" else a, b.view(word) if b.dtype.kind == "f" else b, err_msg=what)


def _assert_all(device, prefix, want, what):
    for key in KEYS:
        _assert_bits(device["%s_%s" % (prefix, key)], want[key], "%s %s" % (what, key))
    assert device[prefix + "_num_draws"] == want["num_draws"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_restatement(name, device):
    spec = CASES[name]
    want = _restated_case(device, name)
    assert want["num_draws"] == -(-spec["n"] // spec.get("slice", 1)) * spec["W"]
    for how in ("host", "dev"):
        if spec.get({"host": "host", "dev": "device"}[how], True):
            # the proposals the calculator saw are the restated ones: the log-posteriors the restatement took are of these rows
            _assert_all(device, "%s/%s" % (name, how), want, "%s %s" % (name, how))


@pytest.mark.gpu
def test_the_shapes_are_what_they_are_chosen_for(device):
    assert [_restated_case(device, name)["num_draws"] for name in ("n32", "n1024", "n1026", "d1", "d3_f32", "d17", "d64", "one_chunk")] == \
        [32, 1024, 1026, 30, 320, 180, 520, 83200]
    for name in ("n32", "n1024", "n1026", "d1", "d3_f32", "d17", "d64", "k3_chain2", "one_chunk", "dense_trio"):
        want = _restated_case(device, name)
        assert want["converged"] == 1 and 3 <= want["passes"] <= PASS_BOUND, name
        # (the overlap is S_0 / N + S_1 / N, two means of sigmas: 1 for identical densities in expectation, at most 2 in a sample)
        assert np.isfinite(want["log_evidence"]) and 0 < want["overlap"] <= 2 and want["mcse"] > 0 and (want["nonfinite"] == 0).all(), name


@pytest.mark.gpu
def test_forced_chunks_give_the_one_chunk_result(device):
    for key in KEYS:
        for how in ("host", "dev"):
            _assert_bits(device["chunked/%s_%s" % (how, key)], device["one_chunk/host_" + key], key)


@pytest.mark.gpu
def test_de_and_batch_handles_give_the_dense_handles_bits(device):
    """their calculators return the dense target's bits (the batch callback is the dense handle's calc_logp_device)"""
    for other in ("de_trio", "batch_trio"):
        for key in KEYS:
            _assert_bits(device["%s/host_%s" % (other, key)], device["dense_trio/host_" + key], "%s %s" % (other, key))


@pytest.mark.gpu
def test_a_nan_draw_on_the_device(device):
    for how in ("host", "dev"):
        for key in ("log_evidence", "mcse", "overlap", "ess"):
            assert np.isnan(device["nan/%s_%s" % (how, key)]).all()
        assert device["nan/%s_nonfinite" % how].tolist() == [0, 1] and device["nan/%s_passes" % how] == 0 and device["nan/%s_converged" % how] == 0


@pytest.mark.gpu
def test_proposals_that_overflow_are_counted_and_have_h_zero(device):
    lp = device["overflow/logp_proposals"]
    N = lp.size
    assert 0 < (lp == -np.inf).sum() < N and not np.isnan(lp).any() and np.isfinite(device["overflow/logp_draws"]).all()
    want = _restated_case(device, "overflow")
    for how in ("host", "dev"):
        assert device["overflow/%s_nonfinite" % how].tolist() == [int((lp == -np.inf).sum()), 0]
        assert device["overflow/%s_passes" % how] <= PASS_BOUND
    assert (want["h"][0][lp == -np.inf] == 0.0).all()  # (the solver ran: no u is NaN or +inf, so the final pass's h are there)


REFUSALS = [("d65", E_UNSUPPORTED, "64 at the most"), ("sharded", E_UNSUPPORTED, "sharded"), ("communicator", E_UNSUPPORTED, "communicator"),
            ("owned", E_UNSUPPORTED, "caller-owned positions"), ("three_steps", E_ARG, "n >= 4"), ("three_used_steps", E_ARG, "n >= 4"),
            ("slice", E_ARG, "slice_interval >= 1"), ("null", E_ARG, "must not be NULL"), ("null_mean", E_ARG, "mean and chol must not be NULL"),
            ("null_chol", E_ARG, "mean and chol must not be NULL"), ("chain", E_ARG, "chain 1 outside 0..0"), ("mean", E_ARG, "mean[2] is not finite"),
            ("factor", E_ARG, "chol[3][1] is not finite"), ("diagonal", E_ARG, "chol[1][1] is not a positive normal number"),
            ("batch_chain", E_ARG, "chain 1 outside 0..0"), ("de_chain", E_ARG, "chain 1 outside 0..0"), ("async", E_STATE, "asynchronous run is in progress")]


@pytest.mark.gpu
@pytest.mark.parametrize("tag, code, text", REFUSALS + [("null_step_host", E_ARG, "a step pointer is NULL"), ("host_pointer_dev", E_ARG, "not device memory"),
                                                        ("past_the_end_dev", E_ARG, "end inside the allocation")])
def test_refusals_leave_the_outputs_untouched(device, tag, code, text):
    for t in ([tag] if tag.endswith(("_dev", "_host")) else [tag + "_dev", tag + "_host"]):
        message = str(device["refusals/%s_message" % t])
        assert device["refusals/%s_code" % t] == code and text in message, (t, message)
        assert ("evidence_gaussian_device" in message) == t.endswith("_dev") and "evidence_gaussian" in message
        assert device["refusals/%s_untouched" % t] == 1


@pytest.mark.gpu
def test_the_call_after_the_refusals_succeeds_without_set_state(device):
    spec = dict(dtype="f64", calc="dense", K=1, n=6, W=10, D=4, betas=[1.0])
    mean, chol = make_gaussian(spec)
    _assert_all(device, "refusals/after", _restated(device, "refusals", spec, make_draws(spec), mean, chol, 5, 0), "after the refusals")
    assert device["refusals/all_null_code"] == 0


@pytest.mark.gpu
def test_end_to_end_on_a_device_run(device):
    """run_device of a dense D = 4, W = 32 handle, 600 stored steps, burn-in 100: the Python wrapper fits on the first half behind
    the burn-in and bridges on the second, in place; given the mean and factor it reports, it equals the restatement bit for bit,
    and so does the host entry point on the download.  Walker state and counters are unchanged.  No statistical gate on the code's
    own chain."""
    assert device["e2e/state_untouched"] == 1
    n, burn = E2E["n"], E2E["burn"]
    head = (n - burn) // 2
    mean, chol = device["e2e/mean"], device["e2e/chol"]
    _assert_bits(mean, device["e2e/fit_mean"], "the fitted mean")
    _assert_bits(chol, np.linalg.cholesky(device["e2e/fit_cov"]), "the fitted factor")
    want = _restated(device, "e2e", E2E, device["e2e/steps"][burn + head:], mean, chol, 21, 0)
    assert want["num_draws"] == (n - burn - head) * E2E["W"]
    _assert_all(device, "e2e/dev", want, "e2e dev")
    _assert_all(device, "e2e/host", want, "e2e host")
    assert want["converged"] == 1 and (want["nonfinite"] == 0).all()
