"""Normal scores, rank-normalised split R-hat, bulk-ESS and tail-ESS (mcmcpp_amd/csrc/rank.hip; an extension: Vehtari, Gelman,
Simpson, Carpenter and Buerkner 2021).

CPU: the restatement (tests/rank_restatement.py: the definition of include/mcmcpp_hip.h in numpy) on cases whose answer is known;
the statistical case the estimators exist for (one chain of another scale: the raw R-hat misses it, the folded one does not);
every argument error the entry points check before they open a device; the header and the exports.
GPU: one child process (tests/rank_device.py, under a time limit of its own) runs every case through the host-pointer and the
device entry points; scores, order statistics and every diagnostic are compared bit for bit with the restatement, and the
diagnostics with the existing entry points run on the scores and the indicator chains."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import rank_restatement as rk
from tests import rhat_restatement as rr
from tests.rank_device import DIAG_KEYS, SCORE_KEYS, make_draws
from tests.test_rank_plan import B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(dtype, K, n, W, P, split=1, **more):
    return dict(dtype=dtype, K=K, n=n, W=W, P=P, split=split, seed=K + n + W + P, **more)


# The draws of a parameter are S = K H W L.  B = 2048 draws make a block of a sort pass.
CASES = {
    # fewer draws than a wavefront; one draw short of a block, a block, one more; three blocks and a ragged fourth
    "s32": _case("f64", 1, 16, 2, 1, diag=True, one_chain_3d=True, place="exact"),
    "sBm1": _case("f32", 1, 89, 23, 3, 0, diag=True),
    "sB": _case("f64", 1, 64, 32, 1, diag=True),
    "sBp1": _case("f64", 3, 683, 1, 1, 0, diag=True),
    "s3B17_f32": _case("f32", 1, 101, 61, 3, 0, diag=True),
    "s3B17_f64": _case("f64", 1, 101, 61, 3, 0),
    # all draws equal; two values only
    "equal": _case("f64", 2, 20, 8, 2, mode="equal", diag=True),
    "equal_f32": _case("f32", 2, 300, 8, 1, mode="equal"),
    "two": _case("f32", 2, 140, 16, 2, mode="two", diag=True),
    # keys that differ only in the lowest digit, only in the highest, only in the sign
    "low_digit_f64": _case("f64", 2, 70, 16, 2, mode="low_digit"),
    "low_digit_f32": _case("f32", 2, 70, 16, 2, mode="low_digit"),
    "high_digit_f64": _case("f64", 2, 70, 16, 2, mode="high_digit"),
    "high_digit_f32": _case("f32", 2, 70, 16, 2, mode="high_digit"),
    "sign": _case("f64", 2, 70, 16, 1, mode="sign"),
    # -0 and +0 (which tie), infinities, subnormals, both signs
    "special_f64": _case("f64", 2, 80, 16, 3, mode="special"),
    "special_f32": _case("f32", 2, 80, 16, 3, mode="special"),
    # tiles of the parameters: 3 MB hold two of the five, 1 MB one, the default all (tests/test_rank_plan.py); the host
    # chains of 2.3 MB go up in copy groups of 1 MB
    "tiles_default": _case("f64", 2, 300, 96, 5),
    "tiles_3mb": _case("f64", 2, 300, 96, 5, work_mb=3, chunk_mb=1),
    "tiles_1mb": _case("f64", 2, 300, 96, 5, work_mb=1),
    # split with an odd number of steps (the middle one unranked) behind a burn-in, chains further apart than their steps
    "odd_burn_k3": _case("f64", 3, 45, 8, 2, place="burn", burn=15, diag=True),
    "odd_k1_f32": _case("f32", 1, 33, 12, 3, diag=True, max_lag=7),
    # slice_interval 3 on the device against pre-sliced, scattered host pointers
    "scattered_slice3": _case("f32", 2, 100, 12, 4, slice=3, scattered=True, diag=True),
    "slice3_whole": _case("f64", 3, 50, 5, 3, 0, slice=3, scattered=True),
    # chain[:, 3:] of a contiguous tensor of 16 stored steps at slice_interval 2: 13 stored steps, 7 used, HL = 6 (the middle
    # one unranked), chains 16 steps apart.  The ESS and R-hat calls inside get a request that no public check has seen
    "odd7_slice2_tail_f64": _case("f64", 2, 13, 3, 2, place="tail", burn=3, slice=2, diag=True),
    "odd7_slice2_tail_f32": _case("f32", 2, 13, 3, 2, place="tail", burn=3, slice=2, diag=True),
    # more than 256 blocks in a pass (S > 524 288): a thread of the scan kernel takes two entries of its digit's row, and the
    # histogram and scatter grids pass 256.  S = 3 x 47 x 3750 = 258 B + 366: 259 blocks, thread 129 of the scan takes one
    # entry and the threads behind it none.  S = 3 x 47 x 3733 = 256 B + B + 17: 258 blocks, two parameters in a tile, 64-bit keys
    "s258B366_f32": _case("f32", 3, 3750, 47, 1, 0),
    "s257B17_f64_p2": _case("f64", 3, 3733, 47, 2, 0, host=False),
    # the case the estimators exist for: one chain of four has three times the scale in the last parameter
    "apart": dict(dtype="f64", K=4, n=400, W=32, P=2, split=1, seed=2, mode="apart", diag=True),
}
assert CASES["tiles_default"]["seed"] == CASES["tiles_3mb"]["seed"] == CASES["tiles_1mb"]["seed"]

_WANT = {}


def _want(name, fold):
    if (name, fold) not in _WANT:
        spec = CASES[name]
        _WANT[name, fold] = rk.normal_scores(make_draws(spec), bool(spec["split"]), bool(fold), spec.get("slice", 1))
    return _WANT[name, fold]


def _want_diag(name):
    if (name, "diag") not in _WANT:
        spec = CASES[name]
        _WANT[name, "diag"] = rk.rank_diagnostics(make_draws(spec), bool(spec["split"]), spec.get("max_lag", 0), spec.get("slice", 1))
    return _WANT[name, "diag"]


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

def test_the_cases_have_the_sizes_they_are_for():
    sizes = {name: _want(name, 0)["scores"][..., 0].size for name in ("s32", "sBm1", "sB", "sBp1", "s3B17_f32", "s3B17_f64", "s258B366_f32", "s257B17_f64_p2")}
    assert sizes == dict(s32=32, sBm1=B - 1, sB=B, sBp1=B + 1, s3B17_f32=3 * B + 17, s3B17_f64=3 * B + 17, s258B366_f32=258 * B + 366, s257B17_f64_p2=256 * B + B + 17)
    assert -(-(258 * B + 366) // B) == 259 and -(-(257 * B + 17) // B) == 258  # blocks of a pass: above the scan kernel's 256 threads
    odd = _want("odd_burn_k3", 0)
    assert odd["scores"].shape == (3, 44, 8, 2) and odd["sequence_length"] == 22 and odd["num_sequences"] == 48  # the middle step is not there
    for name in ("odd7_slice2_tail_f64", "odd7_slice2_tail_f32"):
        odd = _want(name, 0)
        assert odd["scores"].shape == (2, 6, 3, 2) and odd["sequence_length"] == 3 and odd["num_sequences"] == 12  # 7 used steps of 13


def test_restatement_on_known_answers():
    # all equal: one run of S, every score +0
    z = _want("equal", 0)["scores"]
    assert (z == 0.0).all() and not np.signbit(z).any()
    zf = _want("equal", 1)["scores"]
    assert (zf == 0.0).all() and not np.signbit(zf).any()
    d = _want_diag("equal")
    assert np.isnan(d["rhat"]).all() and np.isnan(d["ess_bulk"]).all() and np.isnan(d["ess_tail"]).all()
    # two values: two scores of opposite sign; finite diagnostics
    x = make_draws(CASES["two"])
    z = _want("two", 0)["scores"]
    for p in range(2):
        lo, hi = z[..., p][x[..., p] < 0], z[..., p][x[..., p] > 0]
        assert len(set(lo)) == 1 and len(set(hi)) == 1 and lo[0] < 0 < hi[0]
    assert np.isfinite(_want_diag("two")["rhat"]).all() and np.isfinite(_want_diag("two")["ess_bulk"]).all()
    # distinct draws: the scores are a permutation of the scores of the ranks 1 .. S, in the draws' order
    x = make_draws(CASES["s3B17_f64"])[0, :, :, 1].ravel()
    z = _want("s3B17_f64", 0)["scores"][0, :, :, 1].ravel()
    assert len(set(x)) == x.size and (np.argsort(x) == np.argsort(z)).all()
    S = x.size
    np.testing.assert_array_equal(np.sort(z), rk.score_of_rank(np.arange(S), np.ones(S, np.int64), S))
    # -0 and +0 tie; the order statistics keep -0 below +0
    x = make_draws(CASES["special_f64"])
    z = _want("special_f64", 0)["scores"]
    zeros = x[..., 0] == 0
    assert np.signbit(x[..., 0][zeros]).any() and not np.signbit(x[..., 0][zeros]).all() and len(set(z[..., 0][zeros])) == 1
    assert np.isinf(x).any() and np.isfinite(z).all() and np.isfinite(_want("special_f64", 1)["scores"]).all()
    # a median that is not finite: unfolded it is returned as it is, folded it fails
    x = np.arange(40.0).reshape(1, 10, 4, 1)
    x[0, :, :2, 0] = -np.inf  # half of the draws: the median interpolates between -inf and 2.0
    assert np.isnan(rk.normal_scores(x, False)["median"][0]) and np.isfinite(rk.normal_scores(x, False)["scores"]).all()
    with pytest.raises(ValueError):
        rk.normal_scores(x, False, fold=True)
    # a NaN draw has no place in the order
    with pytest.raises(ValueError):
        rk.normal_scores(np.array([[[[1.0]], [[np.nan]], [[2.0]], [[0.5]]]]), False)


def test_the_folded_rhat_sees_what_the_raw_one_misses():
    """Four chains of 32 walkers and 400 steps: parameter 0 iid normal everywhere, parameter 1 with the same location but three
    times the scale in one chain (the failure case of Vehtari et al. 2021).  Measured with seed = 2 of make_draws: raw R-hat
    1.00013 / 0.99952, rank-normalised 1.00013 / 0.99963, folded 0.99993 / 1.12822; bulk-ESS 52666 / 51178 and tail-ESS
    51574 / 1009 of 51200 draws.  Both bars are 1.01, the value above which current practice calls a chain unconverged."""
    x = make_draws(CASES["apart"])
    raw = rr.gelman_rubin(x)["rhat"]
    d = _want_diag("apart")
    print("raw", raw, "rank", d["rhat_rank"], "folded", d["rhat_folded"], "bulk", d["ess_bulk"], "tail", d["ess_tail"])
    assert raw[1] < 1.01 and d["rhat_rank"][1] < 1.01            # same location: neither the raw nor the bulk R-hat sees it
    assert d["rhat_folded"][1] > 1.01 and d["rhat"][1] == d["rhat_folded"][1]
    assert raw[0] < 1.01 and d["rhat"][0] < 1.01                 # the iid parameter is fine by every measure
    assert d["ess_tail"][1] < 0.1 * d["ess_tail"][0]             # and the tail-ESS falls with the folded R-hat
    N = d["sequence_length"] * d["num_sequences"]
    assert 0.7 * N < d["ess_bulk"][0] < 1.3 * N and 0.5 * N < d["ess_tail"][0] < 1.5 * N


# ---- CPU: the boundary --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.lib()


def _call(L, what="scores", dtype=capi.F64, steps="good", K=2, n_steps=4, W=3, P=2, split=1, device_path=False, slice_interval=1, stride=0, max_lag=0, scores="good"):
    x = np.arange(48, dtype=np.float64).reshape(2, 4, 3, 2)
    addresses = [x[k, s].ctypes.data for k in range(2) for s in range(4)] * 2
    if steps == "null_step":
        addresses[7] = None
    ptrs = (C.c_void_p * len(addresses))(*addresses)
    n_out = 4 if what == "scores" else 10
    outs = [np.full(4096, 777.0) for _ in range(n_out)] + ([np.full(4096, 777, np.int64) for _ in range(2)] if what == "diag" else [])
    shape = [np.full(1, -5, np.int64), np.full(1, -6, np.int64)]
    args = [capi._ptr(a) for a in outs + shape]
    if what == "scores":
        if scores is None:
            args[0] = None
        lead = [split, 0]
        host, dev = L.mcmcpp_hip_normal_scores, L.mcmcpp_hip_normal_scores_device
    else:
        lead = [split, max_lag]
        host, dev = L.mcmcpp_hip_rank_diagnostics, L.mcmcpp_hip_rank_diagnostics_device
    if device_path:
        rc = dev(dtype, -1, None if steps is None else C.c_void_p(x.ctypes.data), K, stride, n_steps, slice_interval, W, P, *(lead + args))
    else:
        rc = host(dtype, -1, None if steps is None else ptrs, K, n_steps, W, P, *(lead + args))
    untouched = all((a == 777).all() for a in outs) and shape[0][0] == -5 and shape[1][0] == -6
    return rc, (L.mcmcpp_hip_rank_diagnostics_last_error() or b"").decode(), untouched


@pytest.mark.parametrize("what", ("scores", "diag"))
@pytest.mark.parametrize("kw,msg", [
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
    (dict(K=1024, W=2 ** 20, P=1, n_steps=4, split=0, device_path=True), "2^31 - 1 draws"),   # S = 2^32
    (dict(K=1, W=2 ** 29, P=1, n_steps=4, split=0, device_path=True), "2^31 - 1 draws"),      # S = 2^31
    (dict(K=512, W=2 ** 20, P=1024, n_steps=2, split=0, device_path=True), "too many draws in all"),   # S = 2^30, S P = 2^40
], ids=lambda v: "_".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_argument_errors_come_before_the_device(lib, what, kw, msg):
    rc, text, untouched = _call(lib, what, **kw)
    assert rc == 1 and msg in text and ("normal_scores" if what == "scores" else "rank_diagnostics") in text, (rc, text)
    assert untouched


def test_null_scores_and_negative_max_lag(lib):
    for device_path in (False, True):
        rc, text, untouched = _call(lib, "scores", scores=None, device_path=device_path)
        assert rc == 1 and "scores must not be NULL" in text and untouched
        rc, text, untouched = _call(lib, "diag", max_lag=-1, device_path=device_path)
        assert rc == 1 and "max_lag" in text and untouched


def test_python_functions_check_their_arguments():
    x = np.zeros((2, 8, 3, 2))
    for f in (capi.normal_scores, capi.rank_diagnostics):
        with pytest.raises(ValueError):
            f(x, slice_interval=0)
        with pytest.raises(ValueError):
            f(np.zeros((3, 2)))
        with pytest.raises(ValueError):
            f(x, chain_stride_steps=9)  # belongs to device memory
        with pytest.raises(capi.HipError) as e:  # the library's own message comes through
            f(x[:, :3])
        assert e.value.code == 1 and "L >= 2" in str(e.value)
    with pytest.raises(ValueError):
        capi.rank_diagnostics(x, max_lag=-1)


def test_exports_and_knob_are_declared(tmp_path):
    with open(os.path.join(ROOT, "include", "mcmcpp_hip.h")) as fh:
        header = fh.read()
    for name in ("mcmcpp_hip_normal_scores", "mcmcpp_hip_normal_scores_device", "mcmcpp_hip_rank_diagnostics", "mcmcpp_hip_rank_diagnostics_device",
                 "mcmcpp_hip_rank_diagnostics_last_error"):
        assert name + "(" in header and name in capi.EXPORTS
    assert "#define MCMCPP_HIP_ABI_VERSION 2" in header
    for doc in ("include/mcmcpp_hip.h", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as fh:
            assert "MCMCPP_HIP_RANK_WORK_MB" in fh.read(), doc
    # the header compiles as C99 with the new declarations in use
    src = tmp_path / "hdr.c"
    src.write_text('#include "mcmcpp_hip.h"\nint main(void) { double r[1]; int64_t l, m, u[1]; const void* s[4] = {0, 0, 0, 0};\n'
                   'int a = mcmcpp_hip_normal_scores(MCMCPP_HIP_F64, -1, s, 1, 4, 2, 1, 1, 0, r, r, 0, 0, &l, &m);\n'
                   'int b = mcmcpp_hip_normal_scores_device(MCMCPP_HIP_F32, -1, 0, 1, 0, 4, 1, 2, 1, 1, 1, r, 0, 0, 0, &l, &m);\n'
                   'int c = mcmcpp_hip_rank_diagnostics(MCMCPP_HIP_F64, -1, s, 1, 4, 2, 1, 1, 0, r, r, r, r, r, r, r, 0, 0, 0, u, u, &l, &m);\n'
                   'int d = mcmcpp_hip_rank_diagnostics_device(MCMCPP_HIP_F32, -1, 0, 1, 0, 4, 1, 2, 1, 1, 8, r, 0, 0, 0, 0, 0, 0, r, r, r, 0, 0, &l, &m);\n'
                   'return a + b + c + d + (mcmcpp_hip_rank_diagnostics_last_error() == 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "hdr.o")])


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """every case, the sampler's chains and the failures, in one child process"""
    out = str(tmp_path_factory.mktemp("rank_device") / "device.npz")
    spec = dict(cases=CASES, sampler=True, errors=True)
    r = subprocess.run([sys.executable, "-m", "tests.rank_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rank_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _prefixes(spec):
    return [p for p, on in (("host_", spec.get("host", True)), ("dev_", spec.get("device", True))) if on]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_normal_scores_equal_restatement(name, device):
    spec = CASES[name]
    for prefix in _prefixes(spec):
        for fold in (0, 1):
            want = _want(name, fold)
            for key in SCORE_KEYS:
                got = device["%s/%sf%d_%s" % (name, prefix, fold, key)]
                assert got.shape == want[key].shape, (prefix, fold, key)
                np.testing.assert_array_equal(_bits(got), _bits(want[key]), err_msg="%sfold%d %s" % (prefix, fold, key))
            assert list(device["%s/%sf%d_shape" % (name, prefix, fold)]) == [want["sequence_length"], want["num_sequences"]]
    # median, q05, q95 are capi.quantiles' on the same draws (which rounds once to the chain's type)
    q = device[name + "/dev_quantiles"]
    want = _want(name, 0)
    with np.errstate(over="ignore"):
        mine = np.stack([want["median"], want["q05"], want["q95"]], axis=1).astype(q.dtype)
    np.testing.assert_array_equal(q, mine)
    if spec.get("mode") == "equal":
        z = device[name + "/dev_f0_scores"]
        assert (z == 0.0).all() and not np.signbit(z).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n].get("diag")])
def test_rank_diagnostics_equal_composition_and_restatement(name, device):
    spec, want = CASES[name], _want_diag(name)
    for prefix in _prefixes(spec):
        for key in DIAG_KEYS:
            got = device["%s/%sdiag_%s" % (name, prefix, key)]
            np.testing.assert_array_equal(_bits(got), _bits(want[key]), err_msg=prefix + key)                      # the restatement
            np.testing.assert_array_equal(_bits(got), _bits(device["%s/comp_%s" % (name, key)]), err_msg="composition " + key)  # the entry points
        assert list(device["%s/%sdiag_shape" % (name, prefix)]) == [want["sequence_length"], want["num_sequences"]]
    if spec.get("mode") == "equal":
        assert np.isnan(want["rhat"]).all() and np.isnan(want["ess_bulk"]).all() and np.isnan(want["ess_tail"]).all()
    if spec.get("mode") == "two":
        assert np.isfinite(want["rhat"]).all() and np.isfinite(want["ess_bulk"]).all()


@pytest.mark.gpu
def test_the_tile_and_the_chunks_change_no_bit(device):
    for prefix in ("host_", "dev_"):
        for fold in (0, 1):
            for key in SCORE_KEYS:
                a = device["tiles_default/%sf%d_%s" % (prefix, fold, key)]
                for other in ("tiles_3mb", "tiles_1mb"):
                    np.testing.assert_array_equal(_bits(a), _bits(device["%s/%sf%d_%s" % (other, prefix, fold, key)]), err_msg=other + key)


@pytest.mark.gpu
def test_scores_of_chains_the_sampler_wrote(device):
    """Three chains of one handle, 900 stored steps: a rejected move repeats the walker's value, so most draws are duplicates
    and the average ranks are what is tested.  (The CPU oracle of the sampler, one such chain: stretch scale 2 accepts 59 % of
    the moves in four dimensions and leaves 41 % duplicates; scale 6 accepts 26 % and leaves 74 %.  The case uses 6.)"""
    chain = device["sampler/chain"]
    assert chain.shape == (3, 900, 64, 4)
    x0 = chain[..., 0].ravel()
    duplicates = x0.size - np.unique(x0).size
    print("duplicates of parameter 0: %d of %d draws" % (duplicates, x0.size))
    assert duplicates > x0.size // 2
    for fold in (0, 1):
        want = rk.normal_scores(chain, True, bool(fold))
        for key in SCORE_KEYS:
            np.testing.assert_array_equal(_bits(device["sampler/f%d_%s" % (fold, key)]), _bits(want[key]), err_msg="fold%d %s" % (fold, key))
    want = rk.rank_diagnostics(chain[:, 100:])
    for key in DIAG_KEYS:
        np.testing.assert_array_equal(_bits(device["sampler/burn_diag_" + key]), _bits(want[key]), err_msg=key)
        np.testing.assert_array_equal(_bits(device["sampler/burn_host_diag_" + key]), _bits(want[key]), err_msg="host form " + key)
    print("rhat", want["rhat"], "bulk", want["ess_bulk"], "tail", want["ess_tail"])
    assert np.isfinite(want["rhat"]).all() and (want["ess_bulk"] > 100).all() and (want["ess_tail"] > 100).all()


@pytest.mark.gpu
def test_failures_are_clean_and_the_next_call_succeeds(device):
    for name, word in (("nan_draw", "NaN"), ("nan_draw_folded", "NaN"), ("host_pointer", "not device memory"), ("scores_small", "allocation"),
                       ("scores_host", "scores is not device memory"), ("scores_null", "scores must not be NULL"), ("diag_nan", "NaN"),
                       ("inf_median_folded", "median of parameter 1 is not finite"), ("nan_median_folded", "median of parameter 1 is not finite"),
                       ("diag_inf_median", "median of parameter 1 is not finite")):
        assert device["errors/%s_code" % name] == 1 and word in str(device["errors/%s_message" % name]), (name, str(device["errors/%s_message" % name]))
        assert device["errors/%s_untouched" % name] == 1, name
    # unfolded, the same draws are ranked and the median comes back as it is: +inf, and NaN
    for tag, check in (("inf_median", np.isposinf), ("nan_median", np.isnan)):
        want = rk.normal_scores(device["errors/%s_steps" % tag])
        np.testing.assert_array_equal(_bits(device["errors/%s_scores" % tag]), _bits(want["scores"]), err_msg=tag)
        np.testing.assert_array_equal(_bits(device["errors/%s_median" % tag]), _bits(want["median"]), err_msg=tag)
        assert check(want["median"][1]) and np.isfinite(want["median"][0])
    want = rk.normal_scores(device["errors/steps"])
    np.testing.assert_array_equal(_bits(device["errors/after_scores"]), _bits(want["scores"]))
