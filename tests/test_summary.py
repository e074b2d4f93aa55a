"""The posterior summary with its Monte Carlo standard errors (mcmcpp_amd/csrc/summary.hip; an extension: Vehtari, Gelman,
Simpson, Carpenter and Buerkner 2021, section 4).

CPU: the restatement (tests/summary_restatement.py: the definition of include/mcmcpp_hip.h in numpy) on cases whose answer is
known; the statistical case the standard errors exist for; every argument error the entry points check before they open a
device; the header, the exports, the example and the facade.
GPU: one child process (tests/summary_device.py, under a time limit of its own) runs every case through the host-pointer and
the device entry points; every output is compared bit for bit with the restatement, and mean, ess and the quantiles with the
existing entry points on the same input."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import rank_restatement as rk
from tests import summary_restatement as sr
from tests.rank_device import make_draws
from tests.summary_device import DEFAULT_PROBS, KEYS, case_arguments
from tests.test_beta_quantile import reference_quantile
from tests.test_rank_plan import B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIXTEEN = [0.001, 0.01, 0.025, 0.05, 0.1, 0.2, 0.25, 0.4, 0.5, 0.6, 0.75, 0.8, 0.9, 0.95, 0.975, 0.999]


def _case(dtype, K, n, W, P, split=1, **more):
    return dict(dtype=dtype, K=K, n=n, W=W, P=P, split=split, seed=K + n + W + P, **more)


# The draws of a parameter are S = K H W L.  B = 2048 draws make a block of a sort pass, and 2048 window starts a block of the
# HDI reduction: hdi_m = m asks for floor(hdi_prob S) = m.
CASES = {
    # fewer draws than a wavefront; one draw short of a block, a block, one more; three blocks and a ragged fourth
    "s32": _case("f64", 1, 16, 2, 1, one_chain_3d=True, place="exact"),
    "sBm1_16probs_m1": _case("f32", 1, 89, 23, 3, 0, probs=SIXTEEN, hdi_m=1),                  # one window short of a block of the reduction
    "sB_1prob_mSm1": _case("f64", 1, 64, 32, 1, probs=[0.5], hdi_m=B - 1),                     # one window
    "sBp1_0probs": _case("f64", 3, 683, 1, 1, 0, probs=[]),
    "s3B17_f32_w2047": _case("f32", 1, 101, 61, 3, 0, hdi_m=3 * B + 17 - (B - 1)),             # B - 1, B and B + 1 windows
    "s3B17_f64_w2048": _case("f64", 1, 101, 61, 3, 0, hdi_m=3 * B + 17 - B),
    "s3B17_f64_w2049": _case("f64", 1, 101, 61, 1, 0, hdi_m=3 * B + 17 - (B + 1), probs=[0.3]),
    "no_hdi": _case("f64", 2, 40, 8, 2, hdi=0.0),
    # all draws equal; two values only (an interval inside one run of equal draws)
    "equal": _case("f64", 2, 20, 8, 2, mode="equal"),
    "two": _case("f32", 2, 140, 16, 2, mode="two", hdi=0.3),
    # -0 and +0, infinities (widths that are NaN or infinite), subnormals, both signs
    "special_f64": _case("f64", 2, 80, 16, 3, mode="special"),
    "special_f32": _case("f32", 2, 80, 16, 3, mode="special", hdi=0.5),
    # tiles of the parameters: 3 MB hold two of the five, 1 MB one, the default all.  With more tiles than one the sorted keys
    # are kept (2.3 MB here); where MCMCPP_HIP_SUMMARY_KEEP_MB = 1 does not allow that, every tile is sorted a second time
    "tiles_default": _case("f64", 2, 300, 96, 5),
    "tiles_3mb": _case("f64", 2, 300, 96, 5, work_mb=3, chunk_mb=1),
    "tiles_1mb": _case("f64", 2, 300, 96, 5, work_mb=1),
    "tiles_3mb_resort": _case("f64", 2, 300, 96, 5, work_mb=3, keep_mb=1),
    "tiles_1mb_resort": _case("f64", 2, 300, 96, 5, work_mb=1, keep_mb=1),
    # split with an odd number of steps behind a burn-in, chains further apart than their steps
    "odd_burn_k3": _case("f64", 3, 45, 8, 2, place="burn", burn=15, max_lag=7),
    # slice_interval 3 on the device against pre-sliced, scattered host pointers
    "scattered_slice3": _case("f32", 2, 100, 12, 4, slice=3, scattered=True),
    # chain[:, 3:] of a contiguous tensor of 16 stored steps at slice_interval 2: 13 stored steps, 7 used, HL = 6 (the middle
    # one in no sequence), chains 16 steps apart.  The ESS calls inside get a request that no public check has seen
    "odd7_slice2_tail_f64": _case("f64", 2, 13, 3, 2, place="tail", burn=3, slice=2),
    "odd7_slice2_tail_f32": _case("f32", 2, 13, 3, 2, place="tail", burn=3, slice=2),
}
assert len({CASES[n]["seed"] for n in CASES if n.startswith("tiles_")}) == 1 and 57600 * 5 * 8 > 1 << 20

_WANT = {}


def _draw_count(spec):
    return rk.draws(make_draws(spec), bool(spec["split"]), spec.get("slice", 1))[..., 0].size


def _want(name):
    if name not in _WANT:
        spec = CASES[name]
        probs, hdi = case_arguments(spec, _draw_count(spec))
        _WANT[name] = sr.posterior_summary(make_draws(spec), probs, hdi, bool(spec["split"]), spec.get("max_lag", 0), spec.get("slice", 1))
    return _WANT[name]


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

def test_the_cases_have_the_sizes_they_are_for():
    sizes = {name: _draw_count(CASES[name]) for name in CASES}
    assert sizes["s32"] == 32 and sizes["sBm1_16probs_m1"] == B - 1 and sizes["sB_1prob_mSm1"] == B and sizes["sBp1_0probs"] == B + 1
    assert sizes["s3B17_f32_w2047"] == sizes["s3B17_f64_w2048"] == sizes["s3B17_f64_w2049"] == 3 * B + 17 and sizes["tiles_default"] == 57600
    assert sizes["odd7_slice2_tail_f64"] == sizes["odd7_slice2_tail_f32"] == 2 * 6 * 3  # 7 used steps of 13: two halves of 3
    windows = {}
    for name, spec in CASES.items():
        probs, hdi = case_arguments(spec, sizes[name])
        assert len(probs) <= 16
        if hdi:
            m = int(math.floor(np.float64(hdi) * np.float64(sizes[name])))
            assert 1 <= m <= sizes[name] - 1 and ("hdi_m" not in spec or m == spec["hdi_m"])
            windows[name] = sizes[name] - m
    assert windows["sBm1_16probs_m1"] == B - 2 and windows["sB_1prob_mSm1"] == 1
    assert [windows["s3B17_f%s" % s] for s in ("32_w2047", "64_w2048", "64_w2049")] == [B - 1, B, B + 1]
    assert sorted({len(case_arguments(s, 100)[0]) for s in CASES.values()}) == [0, 1, 3, 16]


def test_restatement_on_known_answers():
    # all draws equal: sd = 0, no standard error, the interval is the value at window 0
    d = _want("equal")
    assert (d["mean"] == 2.5).all() and (d["sd"] == 0).all() and (d["quantile"] == 2.5).all()
    assert np.isnan(d["mcse_mean"]).all() and np.isnan(d["mcse_sd"]).all() and np.isnan(d["mcse_quantile"]).all() and np.isnan(d["ess_quantile"]).all()
    assert (d["rank_lower"] == -1).all() and (d["rank_upper"] == -1).all()
    assert (d["hdi_lower"] == 2.5).all() and (d["hdi_upper"] == 2.5).all() and (d["hdi_start"] == 0).all()
    # two values, -1.5 and 3.0: every quantile is one of them; 30 % of the draws fit inside the run of -1.5, from window 0
    d = _want("two")
    x = make_draws(CASES["two"])
    assert np.isin(d["quantile"][:, [0, 2]], (-1.5, 3.0)).all() and (d["quantile"][:, 0] == -1.5).all() and (d["quantile"][:, 2] == 3.0).all()
    assert (d["hdi_lower"] == -1.5).all() and (d["hdi_upper"] == -1.5).all() and (d["hdi_start"] == 0).all()
    assert np.isfinite(d["mcse_mean"]).all() and np.isfinite(d["mcse_sd"]).all()
    for p in range(2):  # sd is numpy's pooled standard deviation with one degree of freedom removed
        assert abs(d["sd"][p] - x[..., p].astype(np.float64).std(ddof=1)) < 1e-12
        low = d["quantile"][p] == -1.5
        assert np.isin(d["mcse_quantile"][p][low], (0.0, 2.25)).all()  # half of 0 or of 4.5
        assert np.isnan(d["mcse_quantile"][p][~low]).all() and (d["rank_lower"][p][~low] == -1).all()  # every draw is <= 3.0: a constant indicator has no ess
    # equal widths: the lowest window wins
    xs = np.arange(20.0)
    assert sr.hdi_of(xs, 0.5) == (0.0, 10.0, 0)
    xs = np.array([0.0, 2.0, 3.0, 5.0, 6.0, 8.0])  # m = 2: widths 3, 3, 3, 3
    assert sr.hdi_of(xs, 0.4) == (0.0, 3.0, 0)
    xs = np.array([0.0, 2.0, 4.0, 5.0, 6.0, 9.0])  # m = 2: widths 4, 3, 2, 4
    assert sr.hdi_of(xs, 0.4) == (4.0, 6.0, 2)
    # infinite draws: inf - inf is NaN and is skipped; a width of +inf is a width
    xs = np.array([-np.inf, -np.inf, -np.inf, 1.0, 2.0, 4.0, 5.0, np.inf])  # m = 2: NaN, inf, inf, 3, 3, inf
    assert sr.hdi_of(xs, 0.25) == (1.0, 4.0, 3)
    xs = np.array([-np.inf, -np.inf, -np.inf, np.inf, np.inf])  # m = 2: NaN, inf, inf
    assert sr.hdi_of(xs, 0.4) == (-np.inf, np.inf, 1)
    # every width NaN
    lo, hi, i = sr.hdi_of(np.full(6, np.inf), 0.5)
    assert np.isnan(lo) and np.isnan(hi) and i == -1
    d = sr.posterior_summary(np.full((2, 4, 3, 1), -np.inf), (0.5,), 0.5)
    assert np.isnan(d["hdi_lower"]).all() and np.isnan(d["hdi_upper"]).all() and (d["quantile"] == -np.inf).all()
    # the special draws: -0 sorts below +0, the infinities make some widths NaN, and an interval is still found
    d = _want("special_f64")
    assert (d["hdi_start"] >= 0).all() and not np.isnan(d["hdi_lower"]).any() and not np.isnan(d["hdi_upper"]).any()
    # a NaN draw has no place in the order
    with pytest.raises(ValueError):
        sr.posterior_summary(np.array([[[[1.0]], [[np.nan]], [[2.0]], [[0.5]]]]), split=False)


def test_mcse_ranks_at_the_ends():
    S = 1000
    assert sr.mcse_ranks(np.nan, 0.5, S) == (-1, -1)
    lo, hi = sr.mcse_ranks(0.0, 0.5, S)  # Beta(1, 1): u = 0.1587, 0.8413
    assert (lo, hi) == (157, 841)
    lo, hi = sr.mcse_ranks(1e9, 0.0001, S)  # u S below 1: the lowest rank
    assert lo == 0 and 0 <= hi < 3
    lo, hi = sr.mcse_ranks(1e9, 0.9999, S)
    assert hi == S - 1 and lo >= S - 3


def test_the_standard_errors_are_what_theory_says():
    """Four chains of 32 walkers and 400 steps (S = 51 200): parameter 0 iid N(0, 1); parameter 1 an AR(1) with rho = 0.9 per
    walker, started from N(0, 1).  Theory: mcse_mean sqrt(S) / sd = 1 and sqrt((1 + rho) / (1 - rho)) = 4.36; the median's
    standard error is sqrt(pi / 2) = 1.2533 that of the mean; mcse_sd sqrt(2 S) / sd = 1; the 94 % interval of a normal is +-1.881.
    Measured here with default_rng(7): 0.995 and 4.20; 1.262; 0.994; (-1.851, 1.889); every u S at least 0.0187 from an integer."""
    rng = np.random.default_rng(7)
    K, n, W, rho = 4, 400, 32, 0.9
    x = np.empty((K, n, W, 2))
    x[..., 0] = rng.standard_normal((K, n, W))
    x[:, 0, :, 1] = rng.standard_normal((K, W))
    eps = rng.standard_normal((K, n, W)) * np.sqrt(1.0 - rho * rho)
    for t in range(1, n):
        x[:, t, :, 1] = rho * x[:, t - 1, :, 1] + eps[:, t]
    d = sr.posterior_summary(x)
    S = d["sequence_length"] * d["num_sequences"]
    assert S == 51200
    mean_ratio = d["mcse_mean"] * np.sqrt(S) / d["sd"]
    median_ratio = d["mcse_quantile"][0, 1] * np.sqrt(S) / d["sd"][0]
    sd_ratio = d["mcse_sd"][0] * np.sqrt(2 * S) / d["sd"][0]
    print("mcse_mean sqrt(S)/sd", mean_ratio, "median", median_ratio, "sd", sd_ratio, "hdi", d["hdi_lower"][0], d["hdi_upper"][0])
    ar = math.sqrt((1 + rho) / (1 - rho))
    assert 0.9 < mean_ratio[0] < 1.1 and 0.9 * 1.2533 < median_ratio < 1.1 * 1.2533 and 0.9 < sd_ratio < 1.1
    assert 0.75 * ar <= mean_ratio[1] <= 1.35 * ar
    assert abs(d["hdi_lower"][0] + 1.881) < 0.1 and abs(d["hdi_upper"][0] - 1.881) < 0.1
    # the ranks are those of the 50-digit inverse, exactly
    margin = 1.0
    for p in range(2):
        for j, prob in enumerate(DEFAULT_PROBS):
            ess = d["ess_quantile"][p, j]
            a, b = ess * np.float64(prob) + 1.0, ess * (1.0 - np.float64(prob)) + 1.0
            with mp.workdps(50):
                u_lo, u_hi = reference_quantile(sr.LOWER_TAIL, a, b) * S, reference_quantile(sr.UPPER_TAIL, a, b) * S
                lo, hi = max(int(mp.floor(u_lo)), 1) - 1, min(int(mp.ceil(u_hi)), S) - 1
                margin = min(margin, float(min(u_lo - mp.floor(u_lo), mp.ceil(u_lo) - u_lo, u_hi - mp.floor(u_hi), mp.ceil(u_hi) - u_hi)))
            assert (d["rank_lower"][p, j], d["rank_upper"][p, j]) == (lo, hi), (p, prob)
    print("the nearest u S lies %.3g from an integer" % margin)


# ---- CPU: the boundary --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.lib()


def _call(L, dtype=capi.F64, steps="good", K=2, n_steps=4, W=3, P=2, split=1, device_path=False, slice_interval=1, stride=0, max_lag=0, probs=(0.05, 0.5, 0.95),
          n_probs=None, hdi=0.5):
    x = np.arange(48, dtype=np.float64).reshape(2, 4, 3, 2)
    addresses = [x[k, s].ctypes.data for k in range(2) for s in range(4)] * 2
    if steps == "null_step":
        addresses[7] = None
    ptrs = (C.c_void_p * len(addresses))(*addresses)
    outs = [np.full(4096, 777.0) for _ in range(9)] + [np.full(4096, 777, np.int64) for _ in range(2)] + [np.full(4096, 777.0) for _ in range(2)]
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    pr = None if probs is None else np.array(probs, dtype=np.float64)
    lead = [split, max_lag, None if pr is None else capi._ptr(pr), (0 if pr is None else pr.size) if n_probs is None else n_probs, hdi]
    args = lead + [capi._ptr(a) for a in outs + shape]
    if device_path:
        rc = L.mcmcpp_hip_posterior_summary_device(dtype, -1, None if steps is None else C.c_void_p(x.ctypes.data), K, stride, n_steps, slice_interval, W, P, *args)
    else:
        rc = L.mcmcpp_hip_posterior_summary(dtype, -1, None if steps is None else ptrs, K, n_steps, W, P, *args)
    untouched = all((a == 777).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6
    return rc, (L.mcmcpp_hip_posterior_summary_last_error() or b"").decode(), untouched


@pytest.mark.parametrize("kw,msg", [
    # what mcmcpp_hip_rank_diagnostics refuses, in its words
    (dict(dtype=7), "dtype"),
    (dict(K=0), "num_chains"),
    (dict(K=1025, device_path=True), "num_chains"),
    (dict(P=0), "num_params"),
    (dict(P=1025, device_path=True), "num_params"),
    (dict(W=0), "num_walkers"),
    (dict(W=2 ** 30, P=2, device_path=True), "2^31"),
    (dict(device_path=True, slice_interval=0), "slice_interval"),
    (dict(device_path=True, stride=3), "chain_stride_steps"),
    (dict(steps=None), "NULL"),
    (dict(steps=None, device_path=True), "NULL"),
    (dict(steps="null_step"), "NULL"),
    (dict(n_steps=3), "L >= 2"),
    (dict(device_path=True, slice_interval=2), "L >= 2"),
    (dict(K=1, W=1, split=0), "M >= 2"),
    (dict(max_lag=-1), "max_lag"),
    (dict(K=1024, W=2 ** 20, P=1, n_steps=4, split=0, device_path=True), "2^31 - 1 draws"),
    (dict(K=1, W=2 ** 29, P=1, n_steps=4, split=0, device_path=True), "2^31 - 1 draws"),
    (dict(K=512, W=2 ** 20, P=1024, n_steps=2, split=0, device_path=True), "too many draws in all"),
    # its own arguments (S = 2 x 2 x 3 x 2 = 24 draws)
    (dict(n_probs=-1), "n_probs"),
    (dict(n_probs=17, probs=[0.5] * 17), "n_probs"),
    (dict(probs=None, n_probs=2), "probs must not be NULL"),
    (dict(probs=[0.5, 0.0]), "0 < prob < 1"),
    (dict(probs=[1.0]), "0 < prob < 1"),
    (dict(probs=[0.2, 0.4, float("nan")], device_path=True), "0 < prob < 1"),
    (dict(hdi=-0.1), "hdi_prob"),
    (dict(hdi=1.0), "hdi_prob"),
    (dict(hdi=float("nan"), device_path=True), "hdi_prob"),
    (dict(hdi=0.04), "floor(hdi_prob S)"),          # floor(0.96) = 0
    (dict(hdi=0.04, device_path=True), "floor(hdi_prob S)"),
], ids=lambda v: "_".join("%s=%s" % (k, "..." if k == "probs" and v[k] and len(v[k]) > 4 else v[k]) for k in v) if isinstance(v, dict) else None)
def test_argument_errors_come_before_the_device(lib, kw, msg):
    rc, text, untouched = _call(lib, **kw)
    assert rc == 1 and msg in text and "posterior_summary" in text, (rc, text)
    assert untouched


def test_the_ends_of_the_hdi_range_pass_the_check(lib):
    """m = 1 (hdi_prob = 1 / 24 rounded up) and m = S - 1 = 23 are accepted: the call gets as far as opening a device, which this
    machine may not have; whatever it then says, it is not the argument check"""
    for hdi in (0.0417, 0.96, 0.0):
        rc, text, _ = _call(lib, hdi=hdi)
        assert rc == 0 or ("hdi_prob" not in text and "n_probs" not in text and rc != 1), (rc, text)


def test_python_functions_check_their_arguments():
    x = np.zeros((2, 8, 3, 2))
    with pytest.raises(ValueError):
        capi.posterior_summary(x, slice_interval=0)
    with pytest.raises(ValueError):
        capi.posterior_summary(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        capi.posterior_summary(x, chain_stride_steps=9)  # belongs to device memory
    with pytest.raises(ValueError):
        capi.posterior_summary(x, max_lag=-1)
    for kw, word in ((dict(probs=(0.5, 1.5)), "0 < prob < 1"), (dict(hdi_prob=1.0), "hdi_prob"), (dict(probs=[0.5] * 17), "n_probs")):
        with pytest.raises(capi.HipError) as e:  # the library's own message comes through
            capi.posterior_summary(x, **kw)
        assert e.value.code == 1 and word in str(e.value)
    with pytest.raises(capi.HipError) as e:
        capi.posterior_summary(x[:, :3])
    assert "L >= 2" in str(e.value)


def test_exports_are_declared_and_the_header_is_c99(tmp_path):
    with open(os.path.join(ROOT, "include", "mcmcpp_hip.h")) as fh:
        header = fh.read()
    for name in ("mcmcpp_hip_posterior_summary", "mcmcpp_hip_posterior_summary_device", "mcmcpp_hip_posterior_summary_last_error", "mcmcpp_hip_beta_quantile"):
        assert name + "(" in header and name in capi.EXPORTS
    assert "#define MCMCPP_HIP_ABI_VERSION 2" in header
    src = tmp_path / "hdr.c"
    src.write_text('#include "mcmcpp_hip.h"\nint main(void) { double r[3], q[3] = {0.05, 0.5, 0.95}; int64_t l, m, u[3]; const void* s[4] = {0, 0, 0, 0};\n'
                   'int a = mcmcpp_hip_posterior_summary(MCMCPP_HIP_F64, -1, s, 1, 4, 2, 1, 1, 0, q, 3, 0.94, r, r, r, r, r, r, r, r, r, u, u, r, r, &l, &m);\n'
                   'int b = mcmcpp_hip_posterior_summary_device(MCMCPP_HIP_F32, -1, 0, 1, 0, 4, 1, 2, 1, 1, 8, 0, 0, 0.0, r, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &l, &m);\n'
                   'return a + b + (mcmcpp_hip_posterior_summary_last_error() == 0) + (mcmcpp_hip_beta_quantile(0.5, 2.0, 2.0) > 0.4); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "hdr.o")])


def test_the_example_and_the_facade_driver_compile():
    from tests.test_histograms import _compile
    _compile(os.path.join(ROOT, "examples", "skewed_gaussian_summary.cpp"), "skewed_gaussian_summary")
    _compile(os.path.join(ROOT, "tests", "cpp", "posterior_summary_facade.cpp"), "posterior_summary_facade")


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """every case, the sampler's chains and the failures, in one child process"""
    out = str(tmp_path_factory.mktemp("summary_device") / "device.npz")
    spec = dict(cases=CASES, sampler=True, errors=True)
    r = subprocess.run([sys.executable, "-m", "tests.summary_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "summary_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def _assert_same_bits(got, want, what):
    """equal bit for bit, a NaN equal to any NaN (the sign of a NaN that inf - inf makes is the processor's)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype != np.float64:
        np.testing.assert_array_equal(got, want, err_msg=what)
        return
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what + " (NaN)")
    np.testing.assert_array_equal(np.where(nan, 0.0, got).view(np.uint64), np.where(nan, 0.0, want).view(np.uint64), err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_summary_equals_restatement_and_the_entry_points(name, device):
    spec, want = CASES[name], _want(name)
    for prefix in ("host_", "dev_"):
        for key in KEYS:
            _assert_same_bits(device["%s/%s%s" % (name, prefix, key)], want[key], prefix + key)
        assert list(device["%s/%sshape" % (name, prefix)]) == [want["sequence_length"], want["num_sequences"]]
        # mean and ess are the ESS entry point's on the same input
        _assert_same_bits(device["%s/%smean" % (name, prefix)], device[name + "/ess_mean"], prefix + "mean of the ESS call")
        _assert_same_bits(device["%s/%sess_mean" % (name, prefix)], device[name + "/ess_ess"], prefix + "ess of the ESS call")
        if want["quantile"].size:  # and the quantiles capi.quantiles' (which rounds once to the chain's type)
            q = device[name + "/quantiles"]
            with np.errstate(over="ignore"):
                np.testing.assert_array_equal(q, device["%s/%squantile" % (name, prefix)].astype(q.dtype))
    if spec.get("hdi") == 0.0:
        assert np.isnan(device[name + "/dev_hdi_lower"]).all()
    if spec.get("mode") == "equal":
        assert (device[name + "/dev_hdi_lower"] == 2.5).all() and (device[name + "/dev_sd"] == 0).all() and (device[name + "/dev_rank_lower"] == -1).all()


@pytest.mark.gpu
def test_the_tile_and_the_chunks_change_no_bit(device):
    for prefix in ("host_", "dev_"):
        for key in KEYS:
            a = device["tiles_default/%s%s" % (prefix, key)]
            for other in ("tiles_3mb", "tiles_1mb", "tiles_3mb_resort", "tiles_1mb_resort"):
                _assert_same_bits(device["%s/%s%s" % (other, prefix, key)], a, other + key)


@pytest.mark.gpu
def test_summary_of_chains_the_sampler_wrote(device):
    """Three chains of one handle, 900 stored steps of which 800 are summarised: about three draws in four repeat the one before,
    so the sorted draws are runs of equal values and the windows of the interval tie."""
    chain = device["sampler/chain"]
    assert chain.shape == (3, 900, 64, 4)
    want = sr.posterior_summary(chain[:, 100:])
    for key in KEYS:
        _assert_same_bits(device["sampler/dev_" + key], want[key], key)
        _assert_same_bits(device["sampler/host_" + key], want[key], "host form " + key)
    print("sd", want["sd"], "mcse_mean", want["mcse_mean"], "ess_quantile", want["ess_quantile"][0], "hdi", want["hdi_lower"], want["hdi_upper"])
    assert np.isfinite(want["mcse_quantile"]).all() and (want["ess_quantile"] > 100).all() and (want["rank_lower"] < want["rank_upper"]).all()


@pytest.mark.gpu
def test_failures_are_clean_and_the_next_call_succeeds(device):
    want = sr.posterior_summary(device["errors/steps"])
    for name, word in (("nan_draw", "NaN"), ("host_pointer", "not device memory"), ("nan_draw_host", "NaN")):
        assert device["errors/%s_code" % name] == 1 and word in str(device["errors/%s_message" % name]), (name, str(device["errors/%s_message" % name]))
        assert device["errors/%s_untouched" % name] == 1, name
    for name in ("nan_draw", "host_pointer"):
        for key in KEYS:
            _assert_same_bits(device["errors/after_%s_%s" % (name, key)], want[key], name + " then " + key)


def _read_facade(raw):
    K, W, P, n, sl, Q = np.frombuffer(raw, np.int32, 6, 0)
    off = [24]

    def take(count, dt=np.float64):
        a = np.frombuffer(raw, dt, count, off[0])
        off[0] += a.nbytes
        return a

    probs, hdi = take(Q), take(1)[0]
    chains = take(K * n * W * P).reshape(K, n, W, P)
    got = {}
    for key in KEYS:
        table = "quantile" in key or key.startswith("rank_")
        got[key] = take(P * Q if table else P, np.int64 if key.startswith("rank_") else np.float64).reshape((P, Q) if table else (P,))
    got["sequence_length"], got["num_sequences"] = (int(v) for v in take(2, np.int64))
    assert off[0] == len(raw)
    return chains, int(sl), probs, hdi, got


@pytest.mark.gpu
def test_facade_class_on_device_and_host_chains(tmp_path):
    from tests.test_histograms import _compile
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "posterior_summary_facade.cpp"), "posterior_summary_facade")
    runs = {}
    for tag, env in (("device", dict(MCMCPP_CHAIN_MEMORY="device")), ("heap", dict(MCMCPP_CHAIN_MEMORY="heap")),
                     ("downloaded", dict(MCMCPP_CHAIN_MEMORY="device", MCMCPP_DEVICE_ANALYSIS="0"))):
        outp = tmp_path / (tag + ".bin")
        e = {k: v for k, v in os.environ.items() if k not in ("MCMCPP_CHAIN_MEMORY", "MCMCPP_DEVICE_ANALYSIS")}
        r = subprocess.run([exe, str(outp)], capture_output=True, text=True, timeout=300, env=dict(e, **env))
        assert r.returncode == 0 and "posterior_summary_facade OK" in r.stdout, tag + r.stdout + r.stderr
        runs[tag] = (r.stdout, outp.read_bytes())
    assert runs["device"] == runs["heap"] == runs["downloaded"]
    chains, sl, probs, hdi, got = _read_facade(runs["device"][1])
    assert chains.shape == (3, 901, 64, 4) and sl == 2 and list(probs) == [0.1, 0.5] and hdi == 0.8
    want = sr.posterior_summary(chains, probs, hdi, True, 0, sl)
    for key in KEYS:
        _assert_same_bits(got[key], want[key], "facade " + key)
    assert (got["sequence_length"], got["num_sequences"]) == (225, 3 * 2 * 64) == (want["sequence_length"], want["num_sequences"])
    table = runs["device"][0].split("\n")
    assert table[0].startswith("param |") and "mcse_mean" in table[0] and "q0.1" in table[0] and "hdi 0.8" in table[0] and sum(l.startswith("P") for l in table) == 4


@pytest.mark.gpu
def test_summary_example_runs():
    from tests.test_histograms import _compile
    exe = _compile(os.path.join(ROOT, "examples", "skewed_gaussian_summary.cpp"), "skewed_gaussian_summary")
    r = subprocess.run([exe, "1019"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1920 sequences of 408 steps" in r.stdout and "mcse_mean" in r.stdout and "R-hat | bulk-ESS | tail-ESS" in r.stdout
    rows = [line for line in r.stdout.split("\n") if line[:1] == "P" and line[1:2].isdigit()]
    assert len(rows) == 4  # two rows of the table, two of the diagnostics
    for row in rows[:2]:
        cells = [[float(v) for v in cell.split()] for cell in row.split("|")[1:]]
        (mean, mcse_mean), (sd, mcse_sd) = cells[0], cells[1]
        q05, q50, q95 = (c[0] for c in cells[2:5])
        lower, upper = cells[5]
        assert 0 < mcse_mean < sd and 0 < mcse_sd < sd and q05 < q50 < q95 and lower < mean < upper and lower < q50 < upper
