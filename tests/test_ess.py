"""The effective sample size across chains and walkers (mcmcpp_amd/csrc/ess.hip; an extension: the multi-sequence estimator that
goes with the split R-hat of tests/test_rhat.py).

CPU: the restatement (tests/ess_restatement.py: the definition of include/mcmcpp_hip.h in numpy) against a long-double direct
computation; what the estimator says about AR(1) series, iid draws, an alternating series, a constant column and a chain that
is shifted; every argument error the entry points check before they open a device; the header, the two knobs, and the programs
that use the facade class compile and link; and which rounds of the plan (mcmcpp_amd/csrc/ess_plan.hpp) every GPU case takes.
GPU: one child process (tests/ess_device.py, under a time limit of its own) runs every case through the host-pointer and the
device entry points; every output is compared bit for bit with the restatement."""
import ctypes as C
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import ess_restatement as er
from tests import rhat_restatement as rr
from tests.ess_device import KEYS, make_series
from tests.rhat_device import reshaped
from tests.test_ess_plan import B, build_driver, rounds_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

# The restatement against long double.  autocov is measured relative to the lag-0 autocovariance (gamma_t itself passes
# through zero) and rho absolutely (|rho| <= 1); tau and ess relatively.  Measured worst differences over these five shapes:
# autocov 5.7e-13, rho 1.5e-12, tau 6.8e-12, ess 6.8e-12 (all at the 1e6 offset: the sequence means are formed to 1e-16 of 1e6,
# and every e_s carries that error into its products); without the offset all four are below 2.3e-15.  The bars are those with
# two to three orders of magnitude of margin, for |mean| / sd <= 1e7.
BARS = dict(autocov=1e-10, rho=1e-9, tau=1e-9, ess=1e-9)

RESTATEMENT_SHAPES = {
    "ar_k2": dict(dtype="f64", K=2, n=400, W=8, P=3, seed=1, ar=[0.0, 0.5, 0.9]),
    "ar_k3_1e6": dict(dtype="f64", K=3, n=300, W=6, P=2, seed=2, offset=1e6, ar=0.5),
    "ar_f32_50": dict(dtype="f32", K=2, n=200, W=10, P=3, seed=3, offset=50.0, ar=0.7),
    "k1_n7": dict(dtype="f64", K=1, n=7, W=4, P=1, seed=4),
    "whole_capped": dict(dtype="f64", K=2, n=150, W=5, P=2, seed=5, ar=0.8, split=0, max_lag=40),
}


@pytest.mark.parametrize("name", list(RESTATEMENT_SHAPES))
def test_restatement_against_long_double(name):
    spec = RESTATEMENT_SHAPES[name]
    x = make_series(spec)
    kw = dict(split=bool(spec.get("split", 1)), max_lag=spec.get("max_lag", 0), n_functions=1000)
    got, want = er.effective_sample_size(x, **kw), er.direct_long_double(x, **kw)
    L = got["sequence_length"]
    cap = L - 1 if not kw["max_lag"] else min(kw["max_lag"], L - 1)
    assert np.isfinite(got["rho"][:, :cap + 1]).all() and np.isnan(got["rho"][:, cap + 1:]).all() and np.isnan(got["autocov"][:, cap + 1:]).all()
    g, w = got["autocov"][:, :cap + 1].astype(np.longdouble), want["autocov"]
    errs = dict(autocov=np.max(np.abs(g - w) / np.abs(w[:, :1])), rho=np.max(np.abs(got["rho"][:, :cap + 1] - want["rho"])),
                tau=np.max(np.abs(got["tau"] - want["tau"]) / want["tau"]), ess=np.max(np.abs(got["ess"] - want["ess"]) / want["ess"]))
    # the window decisions: no closing pair within the bar of zero, so both computations stop at the same pair
    closing = want["closing"][want["closed"] == 1]
    print("%s closing pairs: %s" % (name, closing))
    assert (np.abs(closing) > 100 * BARS["rho"]).all()
    np.testing.assert_array_equal(got["lags_used"], want["lags_used"])
    np.testing.assert_array_equal(got["closed"], want["closed"])
    for key, err in errs.items():
        print("%s %s: %.3g" % (name, key, float(err)))
        assert err <= BARS[key], key
    base = rr.gelman_rubin(x, kw["split"])
    for key in ("rhat", "mean", "within", "between"):
        np.testing.assert_array_equal(got[key], base[key])
    assert (got["sequence_length"], got["num_sequences"]) == (base["sequence_length"], base["num_sequences"])


def test_no_value_depends_on_when_the_windows_are_walked():
    x = make_series(RESTATEMENT_SHAPES["ar_k2"])
    a, b = er.effective_sample_size(x, n_functions=7), er.effective_sample_size(x, n_functions=7, first_lags=2)
    for key in KEYS:
        np.testing.assert_array_equal(a[key], b[key])
    assert a["lags_used"].max() > 16  # (more than the first lags of b: its rounds had to double)


def _ar1(K, n, W, phis, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((K, n, W, len(phis)))
    for p, phi in enumerate(phis):
        z = rng.standard_normal((K, n, W))
        x[:, 0, :, p] = z[:, 0] / math.sqrt(1.0 - phi * phi)
        for s in range(1, n):
            x[:, s, :, p] = phi * x[:, s - 1, :, p] + z[:, s]
    return x


def test_what_the_estimator_says():
    phis = (0.0, 0.5, 0.9)
    x = _ar1(2, 2000, 16, phis, seed=7)
    a = er.effective_sample_size(x)
    N = 2 * 2 * 16 * 1000
    assert a["sequence_length"] == 1000 and a["num_sequences"] == 64
    print("AR(1) tau:", a["tau"], "lags used:", a["lags_used"])
    for p, phi in enumerate(phis):
        assert abs(a["tau"][p] / ((1 + phi) / (1 - phi)) - 1) < 0.15
    np.testing.assert_array_equal(a["ess"], N / a["tau"])
    assert 0.8 * N < a["ess"][0] < 1.25 * N  # iid draws
    assert (a["closed"] == 1).all()
    base = rr.gelman_rubin(x)
    for key in ("rhat", "mean", "within", "between"):
        np.testing.assert_array_equal(a[key], base[key])
    # one chain shifted by 5 in one parameter: its ess falls, the others keep their bits
    shifted = x.copy()
    shifted[1, :, :, 1] += 5.0
    b = er.effective_sample_size(shifted)
    assert b["ess"][1] < 0.05 * a["ess"][1] and b["closed"][1] == 0
    for key in ("ess", "tau", "lags_used", "closed"):
        np.testing.assert_array_equal(b[key][[0, 2]], a[key][[0, 2]])
    # an alternating series lands on the floor 1 / log10(N)
    alt = make_series(dict(dtype="f64", K=2, n=200, W=4, P=2, seed=8, alternating=True))
    c = er.effective_sample_size(alt)
    assert c["tau"][0] == 1.0 / math.log10(2 * 2 * 4 * 100) and c["ess"][0] == 1600 / c["tau"][0] and c["tau"][1] > c["tau"][0]
    # a constant column: NaN, the other parameters finite
    const = make_series(dict(dtype="f64", K=2, n=20, W=4, P=3, seed=22, constant=True))
    d = er.effective_sample_size(const, n_functions=3)
    assert np.isnan(d["ess"][2]) and np.isnan(d["tau"][2]) and np.isfinite(d["ess"][:2]).all() and np.isfinite(d["tau"][:2]).all()
    assert d["rho"][2, 0] == 1.0 and np.isnan(d["rho"][2, 1:]).all() and d["closed"][2] == 1 and d["lags_used"][2] == 2
    # L = 2: one pair, nothing to close
    e = er.effective_sample_size(x[:, :4])
    assert e["sequence_length"] == 2 and (e["closed"] == 0).all() and (e["lags_used"] == 2).all()


# ---- CPU: the boundary --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.lib()


def _call(L, dtype=capi.F64, steps="good", K=2, n_steps=4, W=3, P=2, split=1, device_path=False, slice_interval=1, stride=0, max_lag=0, n_functions=2):
    """mcmcpp_hip_effective_sample_size(_device) on two chains of four steps of 3 x 2, with one argument made bad; (code, message,
    untouched)"""
    x = np.arange(48, dtype=np.float64).reshape(2, 4, 3, 2)
    addresses = [x[k, s].ctypes.data for k in range(2) for s in range(4)] * 2  # (more than any call here reads)
    if steps == "null_step":
        addresses[7] = None
    ptrs = (C.c_void_p * len(addresses))(*addresses)
    outs = [np.full(4096, 777.0), np.full(4096, 777.0), np.full(4096, 777, np.int64), np.full(4096, 777, np.int64)] + [np.full(4096, 777.0) for _ in range(6)]
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    args = [capi._ptr(a) for a in outs + shape]
    if device_path:
        rc = L.mcmcpp_hip_effective_sample_size_device(dtype, -1, None if steps is None else C.c_void_p(x.ctypes.data), K, stride, n_steps, slice_interval, W, P, split,
                                                       max_lag, n_functions, *args)
    else:
        rc = L.mcmcpp_hip_effective_sample_size(dtype, -1, None if steps is None else ptrs, K, n_steps, W, P, split, max_lag, n_functions, *args)
    untouched = all((a == 777).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6
    return rc, (L.mcmcpp_hip_effective_sample_size_last_error() or b"").decode(), untouched


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype=7), "dtype"),
    (dict(dtype=-1, device_path=True), "dtype"),
    (dict(K=0), "num_chains"),
    (dict(K=1025), "num_chains"),
    (dict(K=1025, device_path=True), "num_chains"),
    (dict(P=0), "num_params"),
    (dict(P=1025), "num_params"),
    (dict(P=1025, device_path=True), "num_params"),
    (dict(W=0), "num_walkers"),
    (dict(W=-2, device_path=True), "num_walkers"),
    (dict(W=2 ** 21, P=1024), "2^31"),
    (dict(W=2 ** 30, P=2, device_path=True), "2^31"),
    (dict(device_path=True, slice_interval=0), "slice_interval"),
    (dict(device_path=True, slice_interval=-3), "slice_interval"),
    (dict(device_path=True, stride=3), "chain_stride_steps"),       # below n_steps = 4
    (dict(device_path=True, stride=-1), "chain_stride_steps"),
    (dict(steps=None), "NULL"),
    (dict(steps=None, device_path=True), "NULL"),
    (dict(steps="null_step"), "NULL"),
    (dict(n_steps=3), "L >= 2"),                                     # split: L = 1
    (dict(n_steps=1, split=0), "L >= 2"),
    (dict(n_steps=0), "L >= 2"),
    (dict(n_steps=-4, device_path=True), "L >= 2"),
    (dict(device_path=True, slice_interval=2), "L >= 2"),           # every second of four steps: n = 2, L = 1
    (dict(K=1, W=1, split=0), "M >= 2"),
    (dict(K=1, W=1, split=0, device_path=True), "M >= 2"),
    (dict(max_lag=-1), "max_lag"),
    (dict(max_lag=-1, device_path=True), "max_lag"),
    (dict(n_functions=-1), "n_functions"),
    (dict(n_functions=-7, device_path=True), "n_functions"),
], ids=lambda v: "_".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_argument_errors_come_before_the_device(lib, kw, msg):
    rc, text, untouched = _call(lib, **kw)
    assert rc == 1 and msg in text and "effective_sample_size" in text, (rc, text)
    assert untouched


def test_python_function_checks_its_arguments():
    x = np.zeros((2, 8, 3, 2))
    with pytest.raises(ValueError):
        capi.effective_sample_size(x, slice_interval=0)
    with pytest.raises(ValueError):
        capi.effective_sample_size(x, max_lag=-1)
    with pytest.raises(ValueError):
        capi.effective_sample_size(x, n_functions=-1)
    with pytest.raises(ValueError):
        capi.effective_sample_size(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        capi.effective_sample_size(x, chain_stride_steps=9)  # belongs to device memory
    with pytest.raises(ValueError):
        capi.effective_sample_size([[x[0, 0], x[0, 1]], [x[1, 0]]])  # chains of different lengths
    with pytest.raises(capi.HipError) as e:  # the library's own message comes through
        capi.effective_sample_size(x[:, :3])
    assert e.value.code == 1 and "L >= 2" in str(e.value)
    with pytest.raises(capi.HipError) as e:
        capi.effective_sample_size([[x[0, 0, :1, :1]] * 8], split=False)  # a list of one chain of one walker
    assert e.value.code == 1 and "M >= 2" in str(e.value)


def test_exports_and_knobs_are_declared(tmp_path):
    with open(os.path.join(ROOT, "include", "mcmcpp_hip.h")) as fh:
        header = fh.read()
    for name in ("mcmcpp_hip_effective_sample_size", "mcmcpp_hip_effective_sample_size_device", "mcmcpp_hip_effective_sample_size_last_error"):
        assert name + "(" in header and name in capi.EXPORTS
    assert "#define MCMCPP_HIP_ABI_VERSION 2" in header
    for doc in ("include/mcmcpp_hip.h", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as fh:
            text = fh.read()
        assert "MCMCPP_HIP_ESS_FIRST_LAGS" in text and "MCMCPP_HIP_ESS_WORK_MB" in text, doc
    # the header compiles as C99 with the new declarations in use
    src = tmp_path / "hdr.c"
    src.write_text('#include "mcmcpp_hip.h"\nint main(void) { double r[1]; int64_t l, m, u[1]; const void* s[4] = {0, 0, 0, 0};\n'
                   'int a = mcmcpp_hip_effective_sample_size(MCMCPP_HIP_F64, -1, s, 1, 4, 2, 1, 1, 0, 0, r, r, u, u, 0, 0, 0, 0, 0, 0, &l, &m);\n'
                   'int b = mcmcpp_hip_effective_sample_size_device(MCMCPP_HIP_F32, -1, 0, 1, 0, 4, 1, 2, 1, 1, 8, 1, r, 0, 0, 0, r, r, 0, 0, 0, 0, &l, &m);\n'
                   'return a + b + (mcmcpp_hip_effective_sample_size_last_error() == 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "hdr.o")])


def _compile(src, out):
    from tests.test_histograms import _compile as compile_against_the_facade
    return compile_against_the_facade(src, out)


def test_programs_with_the_facade_class_compile_and_link():
    _compile(os.path.join(ROOT, "examples", "skewed_gaussian_ess.cpp"), "skewed_gaussian_ess")
    _compile(os.path.join(ROOT, "tests", "cpp", "effective_sample_size_facade.cpp"), "effective_sample_size_facade")


# ---- the GPU cases, and the rounds they take ------------------------------------------------------------------------------

def _case(dtype, K, n, W, P, split=1, **more):
    return dict(dtype=dtype, K=K, n=n, W=W, P=P, split=split, seed=K + n + W + P, **more)


CASES = {}
# smallest and odd: L = 2 (n = 4, 5) and 3 (n = 7) split, cap 1 and 2; L = n unsplit; one chain as a 3-d tensor
for _n in (4, 5, 7):
    for _split in (1, 0):
        for _dt in ("f64", "f32"):
            CASES["n%d_%s_%s" % (_n, "split" if _split else "whole", _dt)] = _case(_dt, 1, _n, 4, 1, _split, one_chain_3d=True, place="exact", nf=8)
# every lag of an unsplit ramp plus noise, at L - 1 = B - 1, B, B + 1, 2 B, 2 B + 1: the last lag block holds one lag, all, ...
for _L in (B, B + 1, B + 2, 2 * B + 1, 2 * B + 2):
    CASES["ramp_L%d" % _L] = _case("f64" if _L % 2 else "f32", 2, _L, 5, 2, 0, ramp=0.25, nf=_L)
CASES.update({
    # max_lag below, at and above a block edge, on AR(1) series whose windows reach it
    "max_lag31": _case("f64", 2, 200, 6, 2, 0, ar=0.95, max_lag=B - 1, nf=40),
    "max_lag32": _case("f64", 2, 200, 6, 2, 0, ar=0.95, max_lag=B, nf=40),
    "max_lag33": _case("f64", 2, 200, 6, 2, 0, ar=0.95, max_lag=B + 1, nf=40),
    "max_lag_past": _case("f32", 2, 60, 6, 2, ar=0.5, max_lag=1000, nf=40),     # above L - 1 = 29
    # the row shapes of tests/test_rhat.py
    "row120_f32": _case("f32", 2, 50, 10, 3, nf=25),                      # a row of 120 bytes
    "step48_f64": _case("f64", 2, 21, 6, 1, nf=4),                        # read one step (48 bytes) into its allocation
    "base8_f64": _case("f64", 2, 33, 4, 2, place="base8", host=False),    # a base that is only 8-byte aligned
    "ragged257_f64": _case("f64", 2, 40, 257, 1, 0, ar=0.6),              # a ragged last wavefront, five workgroups
    "ragged257_f32": _case("f32", 1, 40, 257, 1, nf=3),
    "pieces_f32": _case("f32", 3, 30, 300, 4, ar=0.4),
    # the sum over m in two slices
    "m1200": _case("f64", 2, 40, 300, 2, ar=[0.3, 0.8], nf=6),
    # several rounds: one block first and 1 MB of lagged products (8192 series: 16 lags fit, so one block a round) against the
    # defaults on the same samples; sequences of 300 steps with a time near 12, so that some windows close and some reach the cap
    "rounds_knobs": _case("f64", 2, 600, 128, 16, ar=0.85, first_lags=B, work_mb=1),
    "rounds_default": _case("f64", 2, 600, 128, 16, ar=0.85),
    "rounds_first1": _case("f64", 2, 600, 128, 16, ar=0.85, first_lags=1, device=False),
    # host steps that are not contiguous in memory; slice_interval 3 on the device against pre-sliced host pointers
    "scattered_slice3": _case("f32", 2, 100, 12, 4, slice=3, scattered=True, ar=0.5, nf=5),
    "slice3_whole": _case("f64", 3, 50, 5, 3, 0, slice=3, scattered=True),
    # chains behind a burn-in of 15 steps in a [K][n_saved][W][P] array; 16 chains 0.3 apart
    "burn_k3": _case("f64", 3, 45, 16, 3, place="burn", burn=15, ar=0.5),
    "k16_apart": _case("f64", 16, 64, 64, 4, chain_shift=0.3, nf=32),
    # one inf and one NaN sample; a constant column; the alternating series
    "nonfinite": _case("f64", 2, 40, 8, 3, nonfinite=True, nf=4),
    "nonfinite_f32": _case("f32", 2, 40, 8, 3, 0, nonfinite=True),
    "constant": _case("f64", 2, 20, 4, 3, constant=True, nf=4),
    "alternating": _case("f64", 2, 200, 4, 2, alternating=True, nf=4),
})
assert CASES["rounds_knobs"]["seed"] == CASES["rounds_default"]["seed"] == CASES["rounds_first1"]["seed"]

_WANT = {}


def _want(name):
    """what the restatement says about the case's samples, computed once"""
    if name not in _WANT:
        spec = CASES[name]
        x = reshaped(spec, make_series(spec))
        _WANT[name] = er.effective_sample_size(x, bool(spec["split"]), spec.get("max_lag", 0), spec.get("nf", 0), spec.get("slice", 1))
    return _WANT[name]


def _rounds(exe, name, device_path):
    """(rounds, lag blocks, elements of a lane) of a case, by the plan: the windows are decided once the closing pair of every
    parameter is known (lags_used + 2 lags), or the pairs up to kmax (lags_used)"""
    spec, want = CASES[name], _want(name)
    K, W, P = spec["K"], spec["W"], spec["P"]
    decided = int(max(want["lags_used"] + 2 * want["closed"]))
    L, M = want["sequence_length"], want["num_sequences"]
    rows = rounds_of(exe, L=L, max_lag=spec.get("max_lag", 0), n_functions=spec.get("nf", 0), series=M * P, E=W * P, zs=K * (2 if spec["split"] else 1), decided=decided,
                     first_lags=spec.get("first_lags"), work_mb=spec.get("work_mb"))
    for first, lags, blocks, gx, gy, gz in rows:
        assert gx == -(-W * P // 64) and gy == -(-blocks // 4) and gz == K * (2 if spec["split"] else 1)
    return len(rows), sum(r[2] for r in rows), 1


# the rounds the named cases must take: (rounds, lag blocks in all, elements of a lane); the same on every device
ROUNDS = {
    "n4_split_f64": (1, 1, 1), "ramp_L32": (1, 1, 1), "ramp_L33": (1, 2, 1), "ramp_L34": (1, 2, 1), "ramp_L65": (1, 3, 1), "ramp_L66": (1, 3, 1),
    "max_lag31": (1, 1, 1), "max_lag32": (1, 2, 1), "max_lag33": (1, 2, 1), "m1200": (1, 1, 1), "k16_apart": (1, 1, 1),
}


def test_the_cases_take_their_rounds():
    exe = build_driver()
    for name, want in ROUNDS.items():
        assert _rounds(exe, name, True) == want, name
    knobs, default, first1 = (_rounds(exe, n, True) for n in ("rounds_knobs", "rounds_default", "rounds_first1"))
    print("rounds_knobs", knobs, "rounds_default", default, "rounds_first1", first1, "lags used", _want("rounds_default")["lags_used"].max())
    assert knobs == (10, 10, 1)    # one block a round
    assert default == (3, 10, 1)   # 64 lags, 128, and the 128 that hold the last 108
    assert first1 == (4, 10, 1)    # 32, 64, 128, 96
    closed = _want("rounds_default")["closed"]
    assert 0 < closed.sum() < closed.size and _want("rounds_default")["lags_used"].max() == 300


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """every case, the sampler's chains and the failures, in one child process"""
    out = str(tmp_path_factory.mktemp("ess_device") / "device.npz")
    spec = dict(cases=CASES, sampler=True, errors=True)
    r = subprocess.run([sys.executable, "-m", "tests.ess_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ess_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_restatement(name, device):
    spec, want = CASES[name], _want(name)
    prefixes = [p for p, on in (("host_", spec.get("host", True)), ("dev_", spec.get("device", True))) if on]
    assert prefixes
    for prefix in prefixes:
        for key in KEYS:
            np.testing.assert_array_equal(device["%s/%s%s" % (name, prefix, key)], want[key], err_msg=prefix + key)
        assert list(device["%s/%sshape" % (name, prefix)]) == [want["sequence_length"], want["num_sequences"]]
    L = want["sequence_length"]
    if name.startswith("ramp_L"):
        assert spec["nf"] == L and np.isfinite(want["rho"]).all() and np.isfinite(want["autocov"]).all()  # every lag 0 .. L - 1
    if name.startswith("max_lag3"):
        assert (want["closed"] == 0).all() and (want["lags_used"] == 2 * ((spec["max_lag"] - 1) // 2 + 1)).all()  # the windows reach the cap
        assert np.isfinite(want["rho"][:, :spec["max_lag"] + 1]).all() and np.isnan(want["rho"][:, spec["max_lag"] + 1:]).all()
    if name == "max_lag_past":
        assert np.isfinite(want["rho"][:, :L]).all() and np.isnan(want["rho"][:, L:]).all() and L == 30
    if name == "m1200":
        assert want["num_sequences"] == 1200 and rr.num_slices(1200) == 2
    if spec.get("nonfinite"):
        assert np.isnan(want["ess"][[0, -1]]).all() and np.isfinite(want["ess"][1])
    if spec.get("constant"):
        assert np.isnan(want["ess"][-1]) and np.isfinite(want["ess"][:-1]).all()
    if spec.get("alternating"):
        assert want["tau"][0] == 1.0 / math.log10(want["num_sequences"] * L)
    if name == "k16_apart":
        narrow = int(np.argmin(want["within"]))
        assert want["closed"][narrow] == 0 and want["lags_used"][narrow] == 32 and want["between"][narrow] > 3 * want["within"][narrow]  # varplus is mostly between


@pytest.mark.gpu
def test_the_knobs_change_no_bit(device):
    for key in KEYS:
        np.testing.assert_array_equal(device["rounds_knobs/host_" + key], device["rounds_default/host_" + key], err_msg=key)
        np.testing.assert_array_equal(device["rounds_knobs/dev_" + key], device["rounds_default/dev_" + key], err_msg=key)
        np.testing.assert_array_equal(device["rounds_first1/host_" + key], device["rounds_default/dev_" + key], err_msg=key)


@pytest.mark.gpu
def test_ess_of_chains_the_sampler_wrote(device):
    """Three chains of one handle, 900 stored steps, read whole and behind a burn-in of 100 (a view of the tensor)."""
    chain = device["sampler/chain"]
    assert chain.shape == (3, 900, 64, 4)
    for tag, x in (("all", chain), ("burn", chain[:, 100:])):
        want = er.effective_sample_size(x, n_functions=8)
        for key in KEYS:
            np.testing.assert_array_equal(device["sampler/%s_%s" % (tag, key)], want[key], err_msg=tag + key)
        L, N = want["sequence_length"], want["sequence_length"] * want["num_sequences"]
        tau, ess = device["sampler/%s_tau" % tag], device["sampler/%s_ess" % tag]
        print("%s: tau %s ess %s of N = %d, lags used %s" % (tag, tau, ess, N, device["sampler/%s_lags_used" % tag]))
        assert np.isfinite(tau).all() and np.isfinite(ess).all() and (tau > 1).all() and (tau < L / 2).all() and (ess < N).all()


@pytest.mark.gpu
def test_failures_are_clean_and_the_next_call_succeeds(device):
    for name, word in (("host_pointer", "not device memory"), ("past_the_end", "allocation")):
        assert device["errors/%s_code" % name] == 1 and word in str(device["errors/%s_message" % name]), (name, str(device["errors/%s_message" % name]))
        assert device["errors/%s_untouched" % name] == 1, name
    want = er.effective_sample_size(device["errors/steps"], n_functions=4)
    for key in KEYS:
        np.testing.assert_array_equal(device["errors/after_" + key], want[key], err_msg=key)


def _read_facade(raw):
    K, W, P, n, sl, split = struct.unpack_from("6i", raw, 0)
    off = [24]

    def take(count, dt=np.float64):
        a = np.frombuffer(raw, dt, count, off[0])
        off[0] += a.nbytes
        return a

    chains = take(K * n * W * P).reshape(K, n, W, P)
    got = dict(ess=take(P), tau=take(P), lags_used=take(P, np.int64), closed=take(P, np.int64), rhat=take(P), mean=take(P), within=take(P), between=take(P))
    got["sequence_length"], got["num_sequences"] = (int(v) for v in take(2, np.int64))
    assert off[0] == len(raw)
    return chains, sl, split, got


@pytest.mark.gpu
def test_facade_class_on_device_pinned_and_downloaded_chains(tmp_path):
    """tests/cpp/effective_sample_size_facade.cpp with the chains in device memory, in pinned host memory, and in device memory
    with the device path switched off: the same bytes from all three, and the restatement's values for the chains it wrote"""
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "effective_sample_size_facade.cpp"), "effective_sample_size_facade")
    runs = {}
    for tag, env in (("device", dict(MCMCPP_CHAIN_MEMORY="device")), ("pinned", dict(MCMCPP_CHAIN_MEMORY="pinned")),
                     ("downloaded", dict(MCMCPP_CHAIN_MEMORY="device", MCMCPP_DEVICE_ANALYSIS="0"))):
        outp = tmp_path / (tag + ".bin")
        e = {k: v for k, v in os.environ.items() if k not in ("MCMCPP_CHAIN_MEMORY", "MCMCPP_DEVICE_ANALYSIS")}
        r = subprocess.run([exe, str(outp)], capture_output=True, text=True, timeout=300, env=dict(e, **env))
        assert r.returncode == 0 and "effective_sample_size_facade OK" in r.stdout, tag + r.stdout + r.stderr
        runs[tag] = (r.stdout, outp.read_bytes())
    assert runs["device"] == runs["pinned"] == runs["downloaded"]
    chains, sl, split, got = _read_facade(runs["device"][1])
    assert chains.shape == (3, 901, 64, 4) and sl == 2 and split == 1  # the initial positions and 900 steps
    want = er.effective_sample_size(chains, True, 0, 0, sl)
    for key in ("ess", "tau", "lags_used", "closed", "rhat", "mean", "within", "between"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert (got["sequence_length"], got["num_sequences"]) == (225, 3 * 2 * 64) == (want["sequence_length"], want["num_sequences"])
    print("ESS of the facade's chains:", got["ess"], "tau", got["tau"])
    assert (got["ess"] > 100).all() and (got["ess"] < 225 * 384).all()


@pytest.mark.gpu
def test_ess_example_runs():
    exe = _compile(os.path.join(ROOT, "examples", "skewed_gaussian_ess.cpp"), "skewed_gaussian_ess")
    r = subprocess.run([exe, "1019"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1920 sequences of 408 steps" in r.stdout
    rows = [[float(v) for v in line.split(":")[1].split("|")] for line in r.stdout.split("\n") if line[:1] == "P" and line[1:2].isdigit()]
    assert len(rows) == 2
    for rhat, ess, tau, lags, closed, mean, err in rows:
        assert 0.9 < rhat < 2.0 and 1 < tau < 204 and 0 < ess < 1920 * 408 and lags >= 2 and err > 0
