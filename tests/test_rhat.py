"""The Gelman-Rubin split R-hat across chains and walkers (mcmcpp_amd/csrc/rhat.hip; an extension, the reference has no such
class).

CPU: the restatement (tests/rhat_restatement.py: the definition of include/mcmcpp_hip.h in numpy) against a long-double two-pass
computation; what R-hat says about chains that agree, one that is shifted, and a constant column; every argument error the
entry points check before they open a device; the header, the chunk knob, and the programs that use the facade class compile
and link; and which launch path of the plan (mcmcpp_amd/csrc/rhat_plan.hpp) every GPU case takes.
GPU: one child process (tests/rhat_device.py, under a time limit of its own) runs every case through the host-pointer and the
device entry points; every output is compared bit for bit with the restatement."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import rhat_restatement as rr
from tests.rhat_device import KEYS, make_steps, reshaped
from tests.test_rhat_plan import build_driver, plan_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

# rtol of the restatement against long double.  Measured worst relative differences over these six shapes: between 4.1e-11 (at
# the 1e6 offset: the sequence means are formed to 1e-16 of 1e6 and between is the variance of means a few 1e-2 apart), rhat
# 2.9e-13, within 8.7e-15, mean 6.2e-16; the bars are those with two to three orders of magnitude of margin, for |mean| / sd <= 1e7.
BARS = dict(mean=1e-12, within=1e-10, rhat=1e-10, between=1e-8, chain_mean=1e-12, chain_within=1e-10, sequence_mean=1e-12)

RESTATEMENT_SHAPES = {
    "k1_n7": dict(dtype="f64", K=1, n=7, W=4, P=1, seed=1),
    "k3_n2051_1e6": dict(dtype="f64", K=3, n=2051, W=6, P=2, seed=2, offset=1e6),          # two slices per sequence
    "k2_n4_f32": dict(dtype="f32", K=2, n=4, W=10, P=3, seed=3),
    "k1_n140001_1e3": dict(dtype="f64", K=1, n=140001, W=4, P=1, seed=4, offset=1e3),      # 61 slices per sequence
    "k2_n3000_f32_50": dict(dtype="f32", K=2, n=3000, W=40, P=5, seed=5, offset=50.0),
    "k16_apart": dict(dtype="f64", K=16, n=64, W=64, P=4, seed=6, chain_shift=0.3),        # the chains' means 0.3 apart
}


@pytest.mark.parametrize("name", list(RESTATEMENT_SHAPES))
def test_restatement_against_long_double(name):
    x = make_steps(RESTATEMENT_SHAPES[name])
    got, want = rr.gelman_rubin(x), rr.two_pass_long_double(x)
    for key, rtol in BARS.items():
        err = np.max(np.abs(got[key].astype(np.longdouble) - want[key]) / np.abs(want[key]))
        print("%s %s: %.3g" % (name, key, float(err)))
        np.testing.assert_allclose(got[key].astype(np.longdouble), want[key], rtol=rtol, atol=0, err_msg=key)
    scale = want["sequence_m2"].max(axis=0)  # (a sum of squares has no relative bar of its own where it is tiny)
    np.testing.assert_allclose(got["sequence_m2"].astype(np.longdouble), want["sequence_m2"], rtol=0, atol=float(1e-10 * scale.max()))
    assert got["sequence_length"] == x.shape[1] // 2 and got["num_sequences"] == 2 * x.shape[0] * x.shape[2]
    if name == "k16_apart":
        narrow = int(np.argmin(want["within"]))
        assert got["rhat"][narrow] > 2.0  # chains 0.3 apart, sd 0.2 to 4: far from converged in the narrow parameter
    if name == "k1_n140001_1e3":
        assert rr.num_slices(got["sequence_length"]) == 61 and rr.slice_len(got["sequence_length"]) == 1152


def test_restatement_unsplit_and_sliced():
    x = make_steps(dict(dtype="f64", K=2, n=31, W=5, P=2, seed=9))
    got, want = rr.gelman_rubin(x, split=False, slice_interval=3), rr.two_pass_long_double(x[:, ::3], split=False)
    assert got["sequence_length"] == 11 and got["num_sequences"] == 10
    for key in ("rhat", "mean", "within", "between", "chain_mean", "chain_within"):
        np.testing.assert_allclose(got[key].astype(np.longdouble), want[key], rtol=1e-12, atol=0)
    odd = rr.gelman_rubin(x)  # n = 31: L = 15, the middle step belongs to no sequence
    np.testing.assert_array_equal(odd["sequence_mean"][:5], rr.gelman_rubin(x[:1, :15], split=False)["sequence_mean"])
    np.testing.assert_array_equal(odd["sequence_mean"][5:10], rr.gelman_rubin(x[:1, 16:], split=False)["sequence_mean"])


def test_what_rhat_says():
    same = make_steps(dict(dtype="f64", K=4, n=400, W=8, P=3, seed=21))
    a = rr.gelman_rubin(same)
    assert (a["rhat"] < 1.1).all() and (a["rhat"] > 0.9).all()  # chains of one distribution
    shifted = same.copy()
    shifted[2, :, :, 1] += 5.0
    b = rr.gelman_rubin(shifted)
    assert b["rhat"][1] > a["rhat"][1] + 0.2 and b["rhat"][1] > 1.2
    np.testing.assert_array_equal(b["rhat"][[0, 2]], a["rhat"][[0, 2]])  # the other parameters are untouched
    assert int(np.argmax(np.abs(b["chain_mean"][:, 1] - np.median(b["chain_mean"][:, 1])))) == 2  # chain_mean shows which
    np.testing.assert_allclose(b["chain_mean"][2, 1] - a["chain_mean"][2, 1], 5.0, rtol=1e-12)
    constant = make_steps(dict(dtype="f64", K=2, n=20, W=4, P=3, seed=22, constant=True))
    c = rr.gelman_rubin(constant)
    assert c["within"][2] == 0 and c["between"][2] == 0 and np.isnan(c["rhat"][2]) and np.isfinite(c["rhat"][:2]).all()


# ---- CPU: the boundary --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.lib()


def _call(L, dtype=capi.F64, steps="good", K=2, n_steps=4, W=3, P=2, split=1, device_path=False, slice_interval=1, stride=0):
    """mcmcpp_hip_gelman_rubin(_device) on two chains of four steps of 3 x 2, with one argument made bad; (code, message, untouched)"""
    x = np.arange(48, dtype=np.float64).reshape(2, 4, 3, 2)
    addresses = [x[k, s].ctypes.data for k in range(2) for s in range(4)] * 2  # (more than any call here reads)
    if steps == "null_step":
        addresses[7] = None
    ptrs = (C.c_void_p * len(addresses))(*addresses)
    outs = [np.full(4096, 777.0) for _ in range(8)]
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    args = [capi._ptr(a) for a in outs + shape]
    if device_path:
        rc = L.mcmcpp_hip_gelman_rubin_device(dtype, -1, None if steps is None else C.c_void_p(x.ctypes.data), K, stride, n_steps, slice_interval, W, P, split, *args)
    else:
        rc = L.mcmcpp_hip_gelman_rubin(dtype, -1, None if steps is None else ptrs, K, n_steps, W, P, split, *args)
    untouched = all((a == 777.0).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6
    return rc, (L.mcmcpp_hip_gelman_rubin_last_error() or b"").decode(), untouched


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype=7), "dtype"),
    (dict(dtype=-1, device_path=True), "dtype"),
    (dict(K=0), "num_chains"),
    (dict(K=1025), "num_chains"),
    (dict(K=1025, device_path=True), "num_chains"),
    (dict(P=0), "num_params"),
    (dict(P=1025), "num_params"),
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
], ids=lambda v: "_".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_argument_errors_come_before_the_device(lib, kw, msg):
    rc, text, untouched = _call(lib, **kw)
    assert rc == 1 and msg in text, (rc, text)
    assert untouched


def test_python_function_checks_its_arguments():
    x = np.zeros((2, 8, 3, 2))
    with pytest.raises(ValueError):
        capi.gelman_rubin(x, slice_interval=0)
    with pytest.raises(ValueError):
        capi.gelman_rubin(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        capi.gelman_rubin(x, chain_stride_steps=9)  # belongs to device memory
    with pytest.raises(ValueError):
        capi.gelman_rubin([[x[0, 0], x[0, 1]], [x[1, 0]]])  # chains of different lengths
    with pytest.raises(capi.HipError) as e:  # the library's own message comes through
        capi.gelman_rubin(x[:, :3])
    assert e.value.code == 1 and "L >= 2" in str(e.value)
    with pytest.raises(capi.HipError) as e:
        capi.gelman_rubin([[x[0, 0, :1, :1]] * 8], split=False)  # a list of one chain of one walker
    assert e.value.code == 1 and "M >= 2" in str(e.value)


def test_exports_and_chunk_knob_are_declared(tmp_path):
    with open(os.path.join(ROOT, "include", "mcmcpp_hip.h")) as fh:
        header = fh.read()
    for name in ("mcmcpp_hip_gelman_rubin", "mcmcpp_hip_gelman_rubin_device", "mcmcpp_hip_gelman_rubin_last_error"):
        assert name + "(" in header and name in capi.EXPORTS
    assert "#define MCMCPP_HIP_ABI_VERSION 2" in header
    for doc in ("include/mcmcpp_hip.h", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as fh:
            assert "MCMCPP_HIP_RHAT_CHUNK_MB" in fh.read(), doc
    # the header compiles as C99 with the new declarations in use
    src = tmp_path / "hdr.c"
    src.write_text('#include "mcmcpp_hip.h"\nint main(void) { double r[1]; int64_t l, m; const void* s[4] = {0, 0, 0, 0};\n'
                   'int a = mcmcpp_hip_gelman_rubin(MCMCPP_HIP_F64, -1, s, 1, 4, 2, 1, 1, r, 0, 0, 0, 0, 0, 0, 0, &l, &m);\n'
                   'int b = mcmcpp_hip_gelman_rubin_device(MCMCPP_HIP_F32, -1, 0, 1, 0, 4, 1, 2, 1, 1, r, 0, 0, 0, 0, 0, 0, 0, &l, &m);\n'
                   'return a + b + (mcmcpp_hip_gelman_rubin_last_error() == 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "hdr.o")])


def _compile(src, out):
    from tests.test_histograms import _compile as compile_against_the_facade
    return compile_against_the_facade(src, out)


def test_programs_with_the_facade_class_compile_and_link():
    _compile(os.path.join(ROOT, "examples", "skewed_gaussian_rhat.cpp"), "skewed_gaussian_rhat")
    _compile(os.path.join(ROOT, "tests", "cpp", "gelman_rubin_facade.cpp"), "gelman_rubin_facade")


# ---- the GPU cases, and the launch paths they take ----------------------------------------------------------------------

def _case(dtype, K, n, W, P, split=1, **more):
    return dict(dtype=dtype, K=K, n=n, W=W, P=P, split=split, seed=K + n + W + P, **more)


CASES = {}
# smallest and odd: L = 2 (n = 4, 5) and 3 (n = 7) split, L = n unsplit; one chain as a 3-d tensor
for _n in (4, 5, 7):
    for _split in (1, 0):
        for _dt in ("f64", "f32"):
            CASES["n%d_%s_%s" % (_n, "split" if _split else "whole", _dt)] = _case(_dt, 1, _n, 4, 1, _split, one_chain_3d=True, place="exact")
CASES.update({
    # load paths
    "row120_f32": _case("f32", 2, 50, 10, 3),                             # a row of 120 bytes: no whole number of 16-byte pieces
    "step48_f64": _case("f64", 2, 21, 6, 1),                              # read one step (48 bytes) into its allocation
    "base8_f64": _case("f64", 2, 33, 4, 2, place="base8", host=False),    # 64-byte rows from a base that is only 8-byte aligned
    "ragged257_f64": _case("f64", 2, 40, 257, 1, 0),                      # a ragged last wavefront and block
    "ragged257_f32": _case("f32", 1, 40, 257, 1),
    "pieces_f32": _case("f32", 3, 30, 300, 4),                            # 16-byte pieces of four, two blocks, the last ragged
    # slices
    "L1024": _case("f64", 1, 2049, 4, 2),                                 # one slice; the middle step dropped
    "L1025": _case("f64", 2, 1025, 4, 2, 0, offset=1e4),                  # two slices, the second of one step
    "slices61": _case("f64", 1, 140001, 4, 1, offset=1e3),                # L = 70000: 61 slices of 1152
    "own": _case("f32", 1, 2101, 65541, 1, place="exact", chunk_mb=300, offset=3.0),   # lanes own whole sequences; two chunks
    "own_reshaped": _case("f32", 1, 2101, 65541, 1, place="exact", offset=3.0, view=[1, 14707, 9363, 1]),  # one block a slice
    # planned as for a device of one CU (MCMCPP_HIP_RHAT_PLAN_CUS), lanes own whole sequences of small shapes too: with 16-byte
    # pieces of both types, and carried over chunks of 256 steps
    "own_pieces_f64": _case("f64", 2, 2101, 64, 8, plan_cus=1, chunk_mb=1),
    "own_pieces_f32": _case("f32", 3, 2055, 200, 4, 0, plan_cus=1, offset=50.0),
    # the host path in forced chunks of 1 MB = 256 steps: boundaries inside slices and beside the dropped middle step
    "chunked": _case("f64", 2, 2101, 64, 8, chunk_mb=1, device=False),
    "one_chunk": _case("f64", 2, 2101, 64, 8),
    # host steps that are not contiguous in memory; slice_interval 3 on the device against pre-sliced host pointers
    "scattered_slice3": _case("f32", 2, 100, 12, 4, slice=3, scattered=True),
    "slice3_whole": _case("f64", 3, 50, 5, 3, 0, slice=3, scattered=True),
    # chains behind a burn-in of 15 steps in a [K][n_saved][W][P] array; 16 chains 0.3 apart
    "burn_k3": _case("f64", 3, 45, 16, 3, place="burn", burn=15),
    "k16_apart": _case("f64", 16, 64, 64, 4, chain_shift=0.3),
    # one inf and one NaN sample; a constant column
    "nonfinite": _case("f64", 2, 40, 8, 3, nonfinite=True),
    "nonfinite_f32": _case("f32", 2, 40, 8, 3, 0, nonfinite=True),
    "constant": _case("f64", 2, 20, 4, 3, constant=True),
})
assert CASES["own"]["seed"] == CASES["own_reshaped"]["seed"] and CASES["chunked"]["seed"] == CASES["one_chunk"]["seed"] == CASES["own_pieces_f64"]["seed"]

_WANT = {}


def _want(name):
    """what the restatement says about the case's samples, computed once"""
    if name not in _WANT:
        spec = CASES[name]
        x = reshaped(spec, make_steps(spec))
        _WANT[name] = rr.gelman_rubin(x, bool(spec["split"]), spec.get("slice", 1))
    return _WANT[name]


def _path(exe, name, cus, device_path):
    """(lanes own whole sequences, slices, elements of a lane) of a case's series launches, by the plan"""
    spec = CASES[name]
    K, n, W, P = spec.get("view", [spec["K"], spec["n"], spec["W"], spec["P"]])
    n = -(-n // spec.get("slice", 1))
    H, L = (2, n // 2) if spec["split"] else (1, n)
    eb = 4 if spec["dtype"] == "f32" else 8
    base = 8 if spec.get("place") == "base8" else (W * P * eb if device_path and spec.get("place", "room") == "room" else 0)
    p = plan_of(exe, E=W * P, elem_bytes=eb, base=base, L=L, zs=K * H if device_path else H, cus=spec.get("plan_cus", cus))
    return p["own"], p["slices"], p["vec"]


# which paths the named cases must take on the device path of 256 CUs: (own, slices, vec)
PATHS = {
    "n4_split_f64": (1, 1, 2), "n5_split_f32": (1, 1, 4),
    "row120_f32": (1, 1, 1), "step48_f64": (1, 1, 2), "base8_f64": (1, 1, 1), "ragged257_f64": (1, 1, 1), "pieces_f32": (1, 1, 4),
    "L1024": (1, 1, 2), "L1025": (0, 2, 2), "slices61": (0, 61, 2),
    "own": (1, 2, 1), "own_reshaped": (0, 8, 1), "one_chunk": (0, 2, 2), "own_pieces_f64": (1, 2, 2), "own_pieces_f32": (1, 3, 4),
}


def test_the_cases_take_their_paths_on_256_cus():
    exe = build_driver()
    for name, want in PATHS.items():
        assert _path(exe, name, 256, True) == want, name
    assert _path(exe, "own", 256, False) == (1, 2, 1)          # the host path of the large case too: state carried by a lane that owns
    assert _path(exe, "chunked", 256, False) == (0, 2, 2)      # and in slots per slice
    assert _path(exe, "slices61", 256, False)[:2] == (0, 61) and _path(exe, "own_pieces_f64", 256, False) == (1, 2, 2)
    seen = {_path(exe, name, 256, dev) for name in CASES for dev in (True, False)}
    assert {(own, min(s, 2), v > 1) for own, s, v in seen} >= {(1, 1, False), (1, 1, True), (1, 2, False), (1, 2, True), (0, 2, False), (0, 2, True)}


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """every case, the sampler's chains and the failures, in one child process"""
    out = str(tmp_path_factory.mktemp("rhat_device") / "device.npz")
    spec = dict(cases=CASES, sampler=True, errors=True)
    r = subprocess.run([sys.executable, "-m", "tests.rhat_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rhat_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
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
    if spec.get("nonfinite"):
        assert np.isnan(want["rhat"][[0, -1]]).all() and np.isfinite(want["rhat"][1])
        assert np.isinf(want["sequence_mean"]).any() or np.isnan(want["sequence_mean"]).any()
    if spec.get("constant"):
        assert np.isnan(want["rhat"][-1]) and want["within"][-1] == 0
    if name == "k16_apart":
        assert want["rhat"][int(np.argmin(want["within"]))] > 2.0


@pytest.mark.gpu
def test_forced_chunks_give_the_one_chunk_result(device):
    a = CASES["chunked"]
    assert a["n"] * a["W"] * a["P"] * 8 > 8 * 2 ** 20 and a["chunk_mb"] == 1 and "chunk_mb" not in CASES["one_chunk"]  # 8.6 MB a chain, in chunks of 1 MB
    for key in KEYS:
        np.testing.assert_array_equal(device["chunked/host_" + key], device["one_chunk/host_" + key], err_msg=key)
        # and where a lane owns its sequences and carries totals and the open slice from chunk to chunk (the same samples)
        np.testing.assert_array_equal(device["own_pieces_f64/host_" + key], device["one_chunk/host_" + key], err_msg=key)


@pytest.mark.gpu
def test_the_cases_take_their_paths_on_this_device(device):
    exe = build_driver()
    cus = int(device["cus"])
    seen = {_path(exe, name, cus, dev) for name in CASES for dev in (True, False)}
    assert {(own, min(s, 2), v > 1) for own, s, v in seen} >= {(1, 1, False), (1, 1, True), (1, 2, False), (1, 2, True), (0, 2, False), (0, 2, True)}


@pytest.mark.gpu
def test_rhat_of_chains_the_sampler_wrote(device):
    """Three chains of one handle, 900 stored steps, read whole and behind a burn-in of 100 (a view of the tensor).  With walkers
    as sequences R-hat^2 is about (L - 1) / L + 2 tau / L, tau the integrated autocorrelation time of a walker (a few tens of
    steps for the stretch move on 64 x 4): sequences of L = 400 steps put a converged sampler near 1.06, well inside 1.2, where
    sequences of 100 steps (first tried here: 1.23 to 1.26) are too short for that bound whatever computes them."""
    chain = device["sampler/chain"]
    assert chain.shape == (3, 900, 64, 4) and len(np.unique(chain[:, :, :, 0])) > 1000
    for tag, x in (("all", chain), ("burn", chain[:, 100:])):
        want = rr.gelman_rubin(x)
        for key in KEYS:
            np.testing.assert_array_equal(device["sampler/%s_%s" % (tag, key)], want[key], err_msg=tag + key)
    print("R-hat behind the burn-in:", device["sampler/burn_rhat"])
    assert (device["sampler/burn_rhat"] < 1.2).all() and (device["sampler/burn_rhat"] > 0.9).all()


@pytest.mark.gpu
def test_failures_are_clean_and_the_next_call_succeeds(device):
    for name, word in (("host_pointer", "not device memory"), ("past_the_end", "allocation")):
        assert device["errors/%s_code" % name] == 1 and word in str(device["errors/%s_message" % name]), (name, str(device["errors/%s_message" % name]))
        assert device["errors/%s_untouched" % name] == 1, name
    want = rr.gelman_rubin(device["errors/steps"])
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
    got = dict(rhat=take(P), mean=take(P), within=take(P), between=take(P), chain_mean=take(K * P).reshape(K, P), chain_within=take(K * P).reshape(K, P))
    got["sequence_length"], got["num_sequences"] = (int(v) for v in take(2, np.int64))
    assert off[0] == len(raw)
    return chains, sl, split, got


@pytest.mark.gpu
def test_facade_class_on_device_pinned_and_downloaded_chains(tmp_path):
    """tests/cpp/gelman_rubin_facade.cpp with the chains in device memory, in pinned host memory, and in device memory with the
    device path switched off: the same bytes from all three, and the restatement's values for the chains the program wrote"""
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "gelman_rubin_facade.cpp"), "gelman_rubin_facade")
    runs = {}
    for tag, env in (("device", dict(MCMCPP_CHAIN_MEMORY="device")), ("pinned", dict(MCMCPP_CHAIN_MEMORY="pinned")),
                     ("downloaded", dict(MCMCPP_CHAIN_MEMORY="device", MCMCPP_DEVICE_ANALYSIS="0"))):
        outp = tmp_path / (tag + ".bin")
        e = {k: v for k, v in os.environ.items() if k not in ("MCMCPP_CHAIN_MEMORY", "MCMCPP_DEVICE_ANALYSIS")}
        r = subprocess.run([exe, str(outp)], capture_output=True, text=True, timeout=300, env=dict(e, **env))
        assert r.returncode == 0 and "gelman_rubin_facade OK" in r.stdout, tag + r.stdout + r.stderr
        runs[tag] = (r.stdout, outp.read_bytes())
    assert runs["device"] == runs["pinned"] == runs["downloaded"]
    chains, sl, split, got = _read_facade(runs["device"][1])
    assert chains.shape == (3, 901, 64, 4) and sl == 2 and split == 1  # the initial positions and 900 steps
    assert not np.array_equal(chains[0], chains[1]) and not np.array_equal(chains[1], chains[2])
    want = rr.gelman_rubin(chains, True, sl)
    for key in ("rhat", "mean", "within", "between", "chain_mean", "chain_within"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert (got["sequence_length"], got["num_sequences"]) == (225, 3 * 2 * 64) == (want["sequence_length"], want["num_sequences"])
    print("R-hat of the facade's chains:", got["rhat"])
    assert (got["rhat"] < 1.2).all()  # sequences of 225 every-second steps of three samplers that have converged


@pytest.mark.gpu
def test_rhat_example_runs():
    exe = _compile(os.path.join(ROOT, "examples", "skewed_gaussian_rhat.cpp"), "skewed_gaussian_rhat")
    r = subprocess.run([exe, "1019"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1920 sequences of 408 steps" in r.stdout and r.stdout.count(" | ") >= 10
    rhat = [float(line.split(":")[1].split("|")[0]) for line in r.stdout.split("\n") if line[:1] == "P" and line[1:2].isdigit()]
    assert len(rhat) == 2 and all(0.9 < v < 2.0 for v in rhat)
