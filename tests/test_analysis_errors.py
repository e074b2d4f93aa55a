"""What every analysis entry point answers to a bad argument, before it opens a device (CPU tests): the return code and the whole
message text, row by row.  The five families (moments, histograms, autocorr, order statistics, device chain) share one host
layer (mcmcpp_amd/csrc/analysis_host.hpp) and keep a message slot each; users match on these texts, so a change of the host
code must leave them as they are, to the letter.  The suites of the families pin some of them by substring.  One GPU test at the
end: the slots of the ESS and R-hat families across the calls of the families that run their code."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi

E_ARG = 1
F64, F32 = capi.F64, capi.F32
X = np.arange(12, dtype=np.float64).reshape(2, 3, 2)  # two steps of 3 walkers x 2 parameters
OUT = np.full(64, 777.0)
RANKS = np.array([0, 5], np.int64)
QUERY = np.array([[1.0, 2.0], [3.0, 4.0]])
NAN_QUERY = np.array([[1.0, 2.0], [3.0, np.nan]])
COUNTS = np.full((2, 2, 2), -5, np.int64)
vp = C.c_void_p


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def step_ptrs(second=True):
    return (vp * 2)(X[0].ctypes.data, X[1].ctypes.data if second else None)


@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.lib()


# ---- order statistics and rank counts: one slot for the four entries ---------------------------------------------------------

def order(L, device_path=False, dtype=F64, steps=True, n_steps=2, slice_interval=1, W=3, P=2, ranks=RANKS, n_ranks=2, values=OUT, null_step=False):
    if device_path:
        return L.mcmcpp_hip_order_statistics_device(dtype, -1, ptr(X) if steps else None, n_steps, slice_interval, W, P, ptr(ranks), n_ranks, ptr(values))
    return L.mcmcpp_hip_order_statistics(dtype, -1, step_ptrs(not null_step) if steps else None, n_steps, W, P, ptr(ranks), n_ranks, ptr(values))


def counts(L, device_path=False, dtype=F64, steps=True, n_steps=2, slice_interval=1, W=3, P=2, query=QUERY, n_query=2, null_step=False):
    if device_path:
        return L.mcmcpp_hip_rank_counts_device(dtype, -1, ptr(X) if steps else None, n_steps, slice_interval, W, P, ptr(query), n_query, ptr(COUNTS[0]), ptr(COUNTS[1]))
    return L.mcmcpp_hip_rank_counts(dtype, -1, step_ptrs(not null_step) if steps else None, n_steps, W, P, ptr(query), n_query, ptr(COUNTS[0]), ptr(COUNTS[1]))


QUANTILE_ROWS = [
    (order, dict(dtype=7), "order_statistics: dtype must be MCMCPP_HIP_F64 or MCMCPP_HIP_F32"),
    (order, dict(P=0), "order_statistics: 1 <= num_params <= 1024"),
    (order, dict(P=1025), "order_statistics: 1 <= num_params <= 1024"),
    (order, dict(W=0), "order_statistics: num_walkers >= 1"),
    (order, dict(n_ranks=0), "order_statistics: 1 <= n_ranks <= 64"),
    (order, dict(n_ranks=65), "order_statistics: 1 <= n_ranks <= 64"),
    (order, dict(ranks=None), "order_statistics: ranks and values must not be NULL"),
    (order, dict(values=None), "order_statistics: ranks and values must not be NULL"),
    (order, dict(device_path=True, values=None), "order_statistics_device: ranks and values must not be NULL"),
    (order, dict(steps=False), "order_statistics: the steps must not be NULL"),
    (order, dict(steps=False, device_path=True), "order_statistics_device: the steps must not be NULL"),
    (order, dict(null_step=True), "order_statistics: a step pointer is NULL"),
    (order, dict(n_steps=0), "order_statistics: no samples (N == 0): n_steps >= 1"),
    (order, dict(n_steps=-1), "order_statistics: no samples (N == 0): n_steps >= 1"),
    (order, dict(ranks=np.array([0, 6], np.int64)), "order_statistics: rank 6 is outside [0, N) with N = 6 samples"),
    (order, dict(ranks=np.array([-1], np.int64), n_ranks=1), "order_statistics: rank -1 is outside [0, N) with N = 6 samples"),
    (order, dict(device_path=True, slice_interval=0), "order_statistics_device: slice_interval >= 1"),
    (order, dict(device_path=True, slice_interval=2, ranks=np.array([3], np.int64), n_ranks=1),
     "order_statistics_device: rank 3 is outside [0, N) with N = 3 samples"),
    (counts, dict(dtype=-1), "rank_counts: dtype must be MCMCPP_HIP_F64 or MCMCPP_HIP_F32"),
    (counts, dict(P=0), "rank_counts: 1 <= num_params <= 1024"),
    (counts, dict(W=-3), "rank_counts: num_walkers >= 1"),
    (counts, dict(n_query=0), "rank_counts: n_query >= 1"),
    (counts, dict(query=None), "rank_counts: query must not be NULL"),
    (counts, dict(query=NAN_QUERY), "rank_counts: a query is NaN (it is neither below nor above a sample)"),
    (counts, dict(steps=False), "rank_counts: the steps must not be NULL"),
    (counts, dict(steps=False, device_path=True), "rank_counts_device: the steps must not be NULL"),
    (counts, dict(null_step=True), "rank_counts: a step pointer is NULL"),
    (counts, dict(n_steps=0), "rank_counts: no samples (N == 0): n_steps >= 1"),
    (counts, dict(device_path=True, slice_interval=-2), "rank_counts_device: slice_interval >= 1"),
]


@pytest.mark.parametrize("call,kw,text", QUANTILE_ROWS, ids=["%s-%s" % (c.__name__, "_".join(k)) for c, k, _ in QUANTILE_ROWS])
def test_quantile_entries(lib, call, kw, text):
    assert call(lib, **kw) == E_ARG
    assert lib.mcmcpp_hip_order_statistics_last_error().decode() == text
    assert (OUT == 777.0).all() and (COUNTS == -5).all()


# ---- autocorrelation times ------------------------------------------------------------------------------------------------------

def autocorr(L, device_path=False, dtype=F64, steps=True, n_steps=2, W=3, P=2, use=0, times=OUT, null_step=False):
    if device_path:
        return L.mcmcpp_hip_autocorr_times_device(dtype, -1, ptr(X) if steps else None, n_steps, W, P, use, 4, ptr(times), None)
    return L.mcmcpp_hip_autocorr_times(dtype, -1, step_ptrs(not null_step) if steps else None, n_steps, W, P, use, 4, ptr(times), None)


AUTOCORR_ROWS = [
    (dict(steps=False), "autocorr_times: steps must not be NULL"),
    (dict(steps=False, device_path=True), "autocorr_times_device: device_steps must not be NULL"),
    (dict(times=None), "autocorr_times: steps and times must not be NULL"),
    (dict(times=None, device_path=True), "autocorr_times: steps and times must not be NULL"),
    (dict(dtype=2), "autocorr_times: dtype must be F64/F32, num_walkers >= 1, num_params >= 1"),
    (dict(W=0), "autocorr_times: dtype must be F64/F32, num_walkers >= 1, num_params >= 1"),
    (dict(P=0, device_path=True), "autocorr_times: dtype must be F64/F32, num_walkers >= 1, num_params >= 1"),
    (dict(n_steps=1), "autocorr_times: 2 <= n_steps <= 2^24"),
    (dict(n_steps=2 ** 24 + 1, device_path=True), "autocorr_times: 2 <= n_steps <= 2^24"),
    (dict(use=-1), "autocorr_times: 0 <= walkers_to_use <= num_walkers"),
    (dict(use=4, device_path=True), "autocorr_times: 0 <= walkers_to_use <= num_walkers"),
    (dict(P=2 ** 30, device_path=True), "autocorr_times: num_params * n_steps and num_walkers * num_params must be below 2^31"),
    (dict(null_step=True), "autocorr_times: a step pointer is NULL"),
]


@pytest.mark.parametrize("kw,text", AUTOCORR_ROWS, ids=["_".join(k) + str(i) for i, (k, _) in enumerate(AUTOCORR_ROWS)])
def test_autocorr_entries(lib, kw, text):
    assert autocorr(lib, **kw) == E_ARG
    assert lib.mcmcpp_hip_autocorr_last_error().decode() == text
    assert (OUT == 777.0).all()


# ---- the device chain -------------------------------------------------------------------------------------------------------------

def compact(L, dtype=F64, steps=X.ctypes.data, n_steps=2, step_elems=6, burn_in=1, interval=1):
    kept = C.c_int64(-1)
    return L.mcmcpp_hip_device_chain_compact(dtype, -1, steps, n_steps, step_elems, burn_in, interval, C.byref(kept))


CHAIN_ROWS = [
    (compact, dict(dtype=3), "device_chain_compact: dtype must be F64 or F32"),
    (compact, dict(n_steps=-1), "device_chain_compact: n_steps >= 0, step_elems >= 1, burn_in >= 0 and interval >= 1"),
    (compact, dict(step_elems=0), "device_chain_compact: n_steps >= 0, step_elems >= 1, burn_in >= 0 and interval >= 1"),
    (compact, dict(burn_in=-1), "device_chain_compact: n_steps >= 0, step_elems >= 1, burn_in >= 0 and interval >= 1"),
    (compact, dict(interval=0), "device_chain_compact: n_steps >= 0, step_elems >= 1, burn_in >= 0 and interval >= 1"),
    (compact, dict(step_elems=2 ** 59), "device_chain_compact: n_steps * step_elems bytes and n_steps * interval must stay below 2^62"),
    (compact, dict(interval=2 ** 62), "device_chain_compact: n_steps * step_elems bytes and n_steps * interval must stay below 2^62"),
    (compact, dict(steps=None), "device_chain_compact: device_steps must not be NULL"),
    (compact, dict(steps=X.ctypes.data + 4), "device_chain_compact: device_steps must be aligned to its element type"),
    (compact, dict(dtype=F32, steps=X.ctypes.data + 2), "device_chain_compact: device_steps must be aligned to its element type"),
    (lambda L: L.mcmcpp_hip_device_copy(None, ptr(X), 8), {}, "device_copy: dst and src must not be NULL"),
    (lambda L: L.mcmcpp_hip_device_copy(ptr(OUT), None, 8), {}, "device_copy: dst and src must not be NULL"),
]


@pytest.mark.parametrize("call,kw,text", CHAIN_ROWS, ids=["%s%d" % ("_".join(k) or "copy", i) for i, (_, k, _t) in enumerate(CHAIN_ROWS)])
def test_device_chain_entries(lib, call, kw, text):
    assert call(lib, **kw) == E_ARG
    assert lib.mcmcpp_hip_device_chain_last_error().decode() == text


def test_device_chain_calls_with_nothing_to_do_need_no_device(lib):
    kept = C.c_int64(-1)
    assert lib.mcmcpp_hip_device_chain_compact(F64, -1, None, 5, 6, 0, 1, C.byref(kept)) == 0 and kept.value == 5  # nothing moves
    assert lib.mcmcpp_hip_device_chain_compact(F64, -1, None, 5, 6, 7, 1, C.byref(kept)) == 0 and kept.value == 0  # nothing is left
    assert lib.mcmcpp_hip_device_copy(None, None, 0) == 0


# ---- moments and histograms: a handle's calls need a handle, and a handle needs a device -------------------------------------------

def moments_create(L, dtype=F64, W=3, P=2, out=True):
    h = vp(12345)
    return L.mcmcpp_hip_moments_create(dtype, -1, W, P, C.byref(h) if out else None), h


def histograms_create(L, dtype=F64, W=3, P=2, bins=10, out=True):
    h = vp(12345)
    return L.mcmcpp_hip_histograms_create(dtype, -1, W, P, bins, 1, C.byref(h) if out else None), h


MOMENTS_BAD = "moments_create: dtype must be F64/F32, num_walkers >= 1, 1 <= num_params <= 1024"
HIST_BAD = "histograms_create: dtype must be F64/F32, num_walkers >= 1, 1 <= num_params <= 65535, bins >= 2"
CREATE_ROWS = [
    (moments_create, "moments", dict(out=False), "moments_create: out is NULL"),
    (moments_create, "moments", dict(dtype=2), MOMENTS_BAD),
    (moments_create, "moments", dict(W=0), MOMENTS_BAD),
    (moments_create, "moments", dict(P=0), MOMENTS_BAD),
    (moments_create, "moments", dict(P=1025), MOMENTS_BAD),
    (histograms_create, "histograms", dict(out=False), "histograms_create: out is NULL"),
    (histograms_create, "histograms", dict(dtype=-1), HIST_BAD),
    (histograms_create, "histograms", dict(W=0), HIST_BAD),
    (histograms_create, "histograms", dict(P=0), HIST_BAD),
    (histograms_create, "histograms", dict(P=65536), HIST_BAD),
    (histograms_create, "histograms", dict(bins=1), HIST_BAD),
]


@pytest.mark.parametrize("call,family,kw,text", CREATE_ROWS, ids=["%s-%s" % (f, "_".join(k)) for _, f, k, _t in CREATE_ROWS])
def test_create_entries(lib, call, family, kw, text):
    rc, h = call(lib, **kw)
    assert rc == E_ARG and h.value == (None if kw.get("out", True) else 12345)  # *out is NULL after a refusal
    assert getattr(lib, "mcmcpp_hip_%s_last_error" % family)(None).decode() == text


HANDLE_CALLS = [
    ("moments", lambda L: L.mcmcpp_hip_moments_add_steps(None, ptr(X), 2, 1)),
    ("moments", lambda L: L.mcmcpp_hip_moments_add_device_steps(None, ptr(X), 2)),
    ("moments", lambda L: L.mcmcpp_hip_moments_add_device_steps_strided(None, ptr(X), 2, 2)),
    ("moments", lambda L: L.mcmcpp_hip_moments_reset(None)),
    ("moments", lambda L: L.mcmcpp_hip_moments_finish(None, None, ptr(OUT), None, None)),
    ("histograms", lambda L: L.mcmcpp_hip_histograms_compute(None, step_ptrs(), 2)),
    ("histograms", lambda L: L.mcmcpp_hip_histograms_compute_device(None, ptr(X), 2, 1)),
    ("histograms", lambda L: L.mcmcpp_hip_histograms_result(None, None, ptr(OUT), None, None, None)),
]


@pytest.mark.parametrize("family,call", HANDLE_CALLS, ids=["%s%d" % (f, i) for i, (f, _) in enumerate(HANDLE_CALLS)])
def test_calls_without_a_handle_are_refused_and_leave_the_message_alone(lib, family, call):
    """(MCMCPP_HIP_E_ARG is all they can say: there is no handle to carry a message, and the slot of *_create stays as it was)"""
    create, _, kw, text = [r for r in CREATE_ROWS if r[1] == family][0]
    assert create(lib, **kw)[0] == E_ARG
    assert call(lib) == E_ARG
    assert getattr(lib, "mcmcpp_hip_%s_last_error" % family)(None).decode() == text
    assert (OUT == 777.0).all()
    getattr(lib, "mcmcpp_hip_%s_destroy" % family)(None)  # (and destroying nothing is fine)


# ---- GPU: the multi-chain families keep their slots to themselves -------------------------------------------------------------------

@pytest.mark.gpu
def test_summary_and_rank_calls_leave_the_ess_and_rhat_slots_alone(tmp_path):
    """The posterior summary and the rank diagnostics run the code of the ESS and R-hat families on chains of their own.  A
    failure of mcmcpp_hip_effective_sample_size_device and of mcmcpp_hip_gelman_rubin_device (a host pointer as device_steps)
    leaves each family's message; neither a summary and rank diagnostics that succeed nor a summary that fails (a NaN draw)
    changes a byte of it.  One child process (tests/summary_device.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "slots.npz")
    r = subprocess.run([sys.executable, "-m", "tests.summary_device", json.dumps(dict(error_slots=True)), out], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "summary_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    assert got["slots/ess_code"] == E_ARG and got["slots/rhat_code"] == E_ARG
    assert str(got["slots/first_ess"]) == "effective_sample_size_device: device_steps is not device memory"
    assert str(got["slots/first_rhat"]) == "gelman_rubin_device: device_steps is not device memory"
    assert np.isfinite(got["slots/ess_mean"]).all() and np.isfinite(got["slots/ess_bulk"]).all()  # the calls in between did succeed
    assert got["slots/nan_code"] == E_ARG and str(got["slots/nan_message"]) == "posterior_summary_device: the draws contain a NaN (it has no place in the order)"
    for when in ("after_success", "after_failure"):
        for family in ("ess", "rhat"):
            assert str(got["slots/%s_%s" % (when, family)]).encode() == str(got["slots/first_%s" % family]).encode(), (when, family)
