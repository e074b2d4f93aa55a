"""Exact order statistics and rank counts of the parameters of a chain (mcmcpp_amd/csrc/quantiles.hip; an extension, beside the
reference's binned PercentileAndMaximumFinder).

CPU: the restatement (tests/quantile_restatement.py: the key map and the radix select, by counting digits only) against np.sort,
bit for bit against a sort by key; the three quantile rules against their formulas; every argument error the entry points check
before they open a device; the header, the chunk knob, and the programs that use the facade class compile and link; and which
launch path of the plan (mcmcpp_amd/csrc/quantile_plan.hpp) every GPU case takes.
GPU: one child process (tests/quantile_device.py, under a time limit of its own) runs every case through the host and the device
entry points; values are compared bit for bit with the restatement, counts exactly with numpy."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import quantile_restatement as qr
from tests.quantile_device import ADVERSARIAL, adversarial_column, make_queries, make_ranks, make_steps, used_count
from tests.test_quantile_plan import build_driver, plan_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    """bit for bit (-0 and +0 differ)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

def _hard_column(N, T, seed):
    """ties, -0 and +0, both infinities, subnormals, and ordinary values of both signs"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N).astype(T)
    special = np.array([-np.inf, np.inf, -0.0, 0.0, np.finfo(T).smallest_subnormal, -np.finfo(T).smallest_subnormal, 3 * np.finfo(T).smallest_subnormal,
                        np.finfo(T).tiny, np.finfo(T).max, -np.finfo(T).max, 1.0, 1.0, 1.0], T)
    where = rng.random(N) < 0.4
    x[where] = rng.choice(special, int(where.sum()))
    return x


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_keys_order_like_the_numbers_and_put_minus_zero_first(T):
    x = np.array([-np.inf, -np.finfo(T).max, -1.0, -np.finfo(T).tiny, -np.finfo(T).smallest_subnormal, -0.0, 0.0, np.finfo(T).smallest_subnormal,
                  np.finfo(T).tiny, 1.0, np.finfo(T).max, np.inf], T)
    k = qr.to_keys(x)
    assert (np.diff(k.astype(object)) > 0).all()  # strictly increasing, -0 before +0
    assert _same(qr.from_keys(k, T), x)
    r = _hard_column(999, T, 3)
    assert _same(qr.from_keys(qr.to_keys(r), T), r)


@pytest.mark.parametrize("N", [1, 2, 257, 777, 1000, 4099])
@pytest.mark.parametrize("digit_bits", [8, 11])
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_restatement_selects_what_a_sort_finds(T, digit_bits, N):
    x = _hard_column(N, T, N + digit_bits)
    by_key = qr.sorted_by_key(x)
    np.testing.assert_array_equal(by_key, np.sort(x))  # the same numbers as np.sort
    zeros = np.flatnonzero(by_key == 0)
    if zeros.size:
        signs = np.signbit(by_key[zeros])
        assert (np.diff(signs.astype(int)) <= 0).all()  # every -0 before every +0
    rng = np.random.default_rng(N)
    ranks = sorted(set([0, N - 1, N // 2] + [int(r) for r in rng.integers(0, N, 12)]))
    got = qr.order_statistics(x.reshape(N, 1, 1), ranks, 1, digit_bits)
    assert _same(got[0], by_key[ranks])


def test_restatement_slices_and_counts_like_numpy():
    x = make_steps(dict(dtype="f64", n=7, W=9, P=3, seed=4, adversarial="three", column=1))
    used = x[::3].reshape(-1, 3)
    got = qr.order_statistics(x, [0, 5, 26], 3)
    for p in range(3):
        assert _same(got[p], np.sort(used[:, p])[[0, 5, 26]])
    q = make_queries(x, 3)
    below, not_above = qr.rank_counts(x, q, 3)
    assert (below[:, 0] < not_above[:, 0]).all()                       # a query equal to a sample
    assert (not_above[:, 1] == 0).all() and (below[:, 2] == 27).all()  # below the minimum, above the maximum
    np.testing.assert_array_equal(below[:, 3], below[:, 4])            # -0 and +0 are one number
    assert (not_above[:, 5] == 0).all() and (not_above[:, 6] == 27).all()


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [1, 2, 10, 1001])
def test_quantile_rules_against_their_formulas(T, N):
    rng = np.random.default_rng(N)
    x = rng.standard_normal((N, 1, 2)).astype(T)
    q = np.array([0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0, 1.0 / 3.0])
    h, lo, hi = capi.quantile_ranks(q, N)
    np.testing.assert_array_equal(h, q * np.float64(N - 1))
    np.testing.assert_array_equal(lo, np.floor(h))
    np.testing.assert_array_equal(hi, np.ceil(h))
    for p in range(2):
        s = np.sort(x[:, 0, p])
        x_lo, x_hi = s[lo], s[hi]
        want = {"lower": x_lo, "higher": x_hi,
                "linear": (x_lo.astype(np.float64) + (x_hi.astype(np.float64) - x_lo.astype(np.float64)) * (h - np.floor(h))).astype(T)}
        for method in ("lower", "higher", "linear"):
            assert _same(qr.quantiles(x, q, method)[p], want[method]), method
            assert _same(capi.quantile_rule(x_lo[None], x_hi[None], h, method, T)[0], want[method]), method
            assert want[method].dtype == T
        if T == np.float64:
            np.testing.assert_array_equal(want["lower"], np.quantile(s, q, method="lower"))
            np.testing.assert_array_equal(want["higher"], np.quantile(s, q, method="higher"))
            np.testing.assert_allclose(want["linear"], np.quantile(s, q), rtol=1e-13, atol=0)
    # equal neighbours are the answer, infinite ones included
    inf = np.array([[np.inf, -np.inf, 2.0]], T)
    assert _same(capi.quantile_rule(inf, inf, np.array([0.5, 0.5, 0.5]), "linear", T), inf)
    with pytest.raises(ValueError):
        capi.quantile_rule(inf, inf, np.array([0.5, 0.5, 0.5]), "nearest", T)
    with pytest.raises(ValueError):
        capi.quantile_ranks([1.5], 10)


# ---- CPU: the boundary --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.lib()


def _order(L, dtype=capi.F64, steps="good", n_steps=2, W=3, P=2, ranks=(0, 5), n_ranks=None, values="good", device_path=False, slice_interval=1):
    """mcmcpp_hip_order_statistics(_device) on two steps of 3 x 2, with one argument made bad; (code, message, values)"""
    x = np.arange(12, dtype=np.float64).reshape(2, 3, 2)
    r = None if ranks is None else np.array(ranks, np.int64)
    out = np.full((max(P, 1), max(1, len(ranks or [0]))), 777.0)
    ptrs = (C.c_void_p * 2)(x[0].ctypes.data, None if steps == "null_step" else x[1].ctypes.data)
    nr = len(ranks or []) if n_ranks is None else n_ranks
    if device_path:
        rc = L.mcmcpp_hip_order_statistics_device(dtype, -1, None if steps is None else C.c_void_p(x.ctypes.data), n_steps, slice_interval, W, P, capi._ptr(r), nr,
                                                  None if values is None else capi._ptr(out))
    else:
        rc = L.mcmcpp_hip_order_statistics(dtype, -1, None if steps is None else ptrs, n_steps, W, P, capi._ptr(r), nr, None if values is None else capi._ptr(out))
    return rc, (L.mcmcpp_hip_order_statistics_last_error() or b"").decode(), out


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype=7), "dtype"),
    (dict(P=0), "num_params"),
    (dict(P=1025), "num_params"),
    (dict(W=0), "num_walkers"),
    (dict(n_ranks=0), "n_ranks"),
    (dict(n_ranks=65), "n_ranks"),
    (dict(ranks=None), "NULL"),
    (dict(values=None), "NULL"),
    (dict(steps=None), "NULL"),
    (dict(steps=None, device_path=True), "NULL"),
    (dict(steps="null_step"), "NULL"),
    (dict(n_steps=0), "N == 0"),
    (dict(n_steps=-1), "N == 0"),
    (dict(ranks=(0, 6)), "rank 6"),
    (dict(ranks=(-1,)), "rank -1"),
    (dict(device_path=True, slice_interval=0), "slice_interval"),
    (dict(device_path=True, slice_interval=2, ranks=(3,)), "rank 3"),  # every second step of two: N = 3
], ids=lambda v: "_".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_order_statistics_argument_errors_come_before_the_device(lib, kw, msg):
    rc, text, out = _order(lib, **kw)
    assert rc == 1 and msg in text, (rc, text)
    assert (out == 777.0).all()


def _counts(L, dtype=capi.F64, steps="good", n_steps=2, W=3, P=2, query="good", n_query=2, device_path=False, slice_interval=1):
    x = np.arange(12, dtype=np.float64).reshape(2, 3, 2)
    q = np.array([[1.0, 2.0], [3.0, np.nan if query == "nan" else 4.0]])
    below, not_above = np.full((2, 2), -5, np.int64), np.full((2, 2), -6, np.int64)
    ptrs = (C.c_void_p * 2)(x[0].ctypes.data, x[1].ctypes.data)
    qp = None if query is None else capi._ptr(q)
    if device_path:
        rc = L.mcmcpp_hip_rank_counts_device(dtype, -1, None if steps is None else C.c_void_p(x.ctypes.data), n_steps, slice_interval, W, P, qp, n_query, capi._ptr(below),
                                             capi._ptr(not_above))
    else:
        rc = L.mcmcpp_hip_rank_counts(dtype, -1, None if steps is None else ptrs, n_steps, W, P, qp, n_query, capi._ptr(below), capi._ptr(not_above))
    return rc, (L.mcmcpp_hip_order_statistics_last_error() or b"").decode(), below, not_above


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype=-1), "dtype"),
    (dict(P=0), "num_params"),
    (dict(W=-3), "num_walkers"),
    (dict(n_query=0), "n_query"),
    (dict(query=None), "NULL"),
    (dict(query="nan"), "NaN"),
    (dict(steps=None), "NULL"),
    (dict(steps=None, device_path=True), "NULL"),
    (dict(n_steps=0), "N == 0"),
    (dict(device_path=True, slice_interval=-2), "slice_interval"),
], ids=lambda v: "_".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_rank_counts_argument_errors_come_before_the_device(lib, kw, msg):
    rc, text, below, not_above = _counts(lib, **kw)
    assert rc == 1 and msg in text, (rc, text)
    assert (below == -5).all() and (not_above == -6).all()


def test_python_functions_check_their_arguments():
    x = np.zeros((2, 3, 2))
    with pytest.raises(ValueError):
        capi.order_statistics(x, [0], slice_interval=0)
    with pytest.raises(ValueError):
        capi.order_statistics(np.zeros((3, 2)), [0])
    with pytest.raises(ValueError):
        capi.rank_counts(x, np.zeros((3, 1)))
    with pytest.raises(ValueError):
        capi.quantiles(x, [0.5], method="nearest")
    with pytest.raises(capi.HipError) as e:  # the library's own message comes through
        capi.order_statistics(x, [6])
    assert e.value.code == 1 and "rank 6" in str(e.value)


def test_exports_and_chunk_knob_are_declared():
    with open(os.path.join(ROOT, "include", "mcmcpp_hip.h")) as fh:
        header = fh.read()
    for name in ("mcmcpp_hip_order_statistics", "mcmcpp_hip_order_statistics_device", "mcmcpp_hip_rank_counts", "mcmcpp_hip_rank_counts_device",
                 "mcmcpp_hip_order_statistics_last_error"):
        assert name + "(" in header and name in capi.EXPORTS
    assert "#define MCMCPP_HIP_ABI_VERSION 2" in header
    for doc in ("include/mcmcpp_hip.h", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as fh:
            assert "MCMCPP_HIP_QUANTILE_CHUNK_MB" in fh.read(), doc


def _compile(src, out):
    from tests.test_histograms import _compile as compile_against_the_facade
    return compile_against_the_facade(src, out)


def test_programs_with_the_facade_class_compile_and_link():
    _compile(os.path.join(ROOT, "examples", "skewed_gaussian_percentiles.cpp"), "skewed_gaussian_percentiles")
    _compile(os.path.join(ROOT, "tests", "cpp", "exact_percentiles_facade.cpp"), "exact_percentiles_facade")


# ---- the GPU cases, and the launch paths they take ----------------------------------------------------------------------

def _case(dtype, n, W, P, adversarial, ranks, slice_interval=1, **more):
    return dict(dtype=dtype, n=n, W=W, P=P, adversarial=adversarial, ranks=ranks, slice=slice_interval, seed=n + W + P, column=n + W, **more)


CASES = {
    # ragged shapes, N = 1, 2, 15, 259, 16, 255 and 256 samples per parameter; P odd in most: rows are not whole 16-byte pieces
    "1x1x1_f64": _case("f64", 1, 1, 1, "constant", "ends"),
    "1x1x1_f32": _case("f32", 1, 1, 1, "zeros", "repeats", 2),
    "1x2x3_f64": _case("f64", 1, 2, 3, "zeros", "repeats"),
    "1x2x3_f32": _case("f32", 1, 2, 3, "inf", "ends"),
    "3x5x1_f64": _case("f64", 3, 5, 1, "three", "percentiles"),
    "3x5x1_f32": _case("f32", 3, 5, 1, "subnormal", "many"),
    "7x37x33_f64": _case("f64", 7, 37, 33, "runs", "many"),
    "7x37x33_f32": _case("f32", 7, 37, 33, "negative", "percentiles", 3),
    "2x8x1024_f64": _case("f64", 2, 8, 1024, "inf", "ends"),
    "2x8x1024_f32": _case("f32", 2, 8, 1024, "last_digit", "repeats", 3),
    "5x51x130_f64": _case("f64", 5, 51, 130, "first_digit", "percentiles"),
    "5x51x130_f32": _case("f32", 5, 51, 130, "first_digit", "many"),
    "2x12x260_f32": _case("f32", 2, 12, 260, "subnormal", "many"),
    "4x64x2_f64": _case("f64", 4, 64, 2, "last_digit", "many"),
    "4x64x2_f32": _case("f32", 4, 64, 2, "three", "percentiles"),
    # slicing: every third step, and an interval past the last step (the first step alone)
    "9x40x5_slice3_f64": _case("f64", 9, 40, 5, "subnormal", "percentiles", 3),
    "9x40x5_slice10_f64": _case("f64", 9, 40, 5, "negative", "many", 10),
    "9x40x5_slice3_f32": _case("f32", 9, 40, 5, "constant", "repeats", 3),
    # many slices of samples per column
    "400x512x2_f64": _case("f64", 400, 512, 2, "runs", "percentiles"),
    "400x512x2_f32": _case("f32", 400, 512, 2, "runs", "many", 3),
    # the host path: 5.4 MB in chunks of 1 MB, from steps that do not lie one behind the other; and in one chunk
    "chunked": _case("f64", 40, 512, 33, "runs", "percentiles", 1, chunk_mb=1, scattered=True, device=False),
    "one_chunk": _case("f64", 40, 512, 33, "runs", "percentiles", 1, device=False),
}
assert {c["adversarial"] for c in CASES.values()} == set(ADVERSARIAL)
assert {c["ranks"] for c in CASES.values()} == {"ends", "percentiles", "many", "repeats"}

_WANT = {}


def _want(name):
    """the case's samples and what the restatement and numpy say about them, computed once"""
    if name not in _WANT:
        spec = CASES[name]
        steps = make_steps(spec)
        ranks = make_ranks(spec, used_count(spec))
        queries = make_queries(steps, spec["slice"])
        _WANT[name] = dict(steps=steps, ranks=ranks, queries=queries, values=qr.order_statistics(steps, ranks, spec["slice"]),
                           counts=qr.rank_counts(steps, queries, spec["slice"]))
    return _WANT[name]


def _paths(exe, name, cus, lds):
    """[(lds, several parameter tiles, distinct rank groups)] of the passes of a case's selection, by the plan"""
    spec, w = CASES[name], _want(name)
    key_bits = 32 if spec["dtype"] == "f32" else 64
    out = []
    for groups in qr.group_counts(w["steps"], w["ranks"], spec["slice"]):
        p = plan_of(exe, n=min(used_count(spec), 2 ** 31 - 1), P=spec["P"], groups=groups, key_bits=key_bits, cus=cus, lds=lds)
        out.append((p["lds"], int(p["ptiles"] > 1), int(groups > 1)))
    return out


# which paths the named cases must take (on any device with 64 KiB of LDS for a block); between them, every path the plan has
PATHS = {
    "1x1x1_f64": {(1, 0, 0)},                                  # one sample: the ranks never part
    "3x5x1_f64": {(1, 0, 0), (1, 0, 1)},                       # LDS counters, one tile, merged then distinct groups
    "7x37x33_f32": {(1, 0, 0), (1, 1, 1)},                     # five groups of 33 parameters: several tiles in LDS
    "7x37x33_f64": {(1, 0, 0), (0, 0, 1)},                     # 64 ranks: more groups than fit beside four parameters: global counters
    "5x51x130_f32": {(1, 1, 0), (0, 0, 1)},                    # 130 parameters: several tiles from the first pass on
    "2x8x1024_f64": {(1, 1, 0), (1, 1, 1)},
    "2x12x260_f32": {(1, 1, 0), (0, 1, 1)},                    # more parameters than a block has threads, and global counters
}


def test_the_cases_take_their_paths_on_256_cus():
    exe = build_driver()
    seen = set()
    for name in CASES:
        taken = _paths(exe, name, 256, 65536)
        assert taken[0][2] == 0  # the first pass: one group for all ranks
        seen |= set(taken)
        if name in PATHS:
            assert set(taken) >= PATHS[name], (name, taken)
    # LDS and global counters; one parameter tile and several; merged and distinct rank groups
    assert seen >= {(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1)}, seen


def test_the_adversarial_columns_are_what_they_are_named_for():
    rng = np.random.default_rng(1)
    for T in (np.float32, np.float64):
        key_bits = 8 * np.dtype(T).itemsize
        col = {kind: adversarial_column(kind, 500, T, rng) for kind in ADVERSARIAL}
        assert all(c.dtype == T and c.shape == (500,) and not np.isnan(c).any() for c in col.values())
        keys = {kind: qr.to_keys(c).astype(object) for kind, c in col.items()}
        assert len(set(keys["constant"])) == 1 and len(set(keys["three"])) == 3
        assert (np.diff(col["runs"]) == 0).sum() > 200 and len(set(col["runs"])) > 100
        assert (col["negative"] < 0).all()
        assert (col["zeros"] == 0).all() and 0 < np.signbit(col["zeros"]).sum() < 500
        assert np.isinf(col["inf"]).sum() > 100 and (col["inf"] == np.inf).any() and (col["inf"] == -np.inf).any()
        assert (np.abs(col["subnormal"]) < np.finfo(T).tiny).all() and len(set(keys["subnormal"])) > 100
        assert len({k >> 8 for k in keys["last_digit"]}) == 1 and len(set(keys["last_digit"])) > 100
        low = {k & ((1 << (key_bits - 8)) - 1) for k in keys["first_digit"]}
        # (negative numbers' keys are complemented: two low parts, one per sign)
        assert len(low) == 2 and len({k >> (key_bits - 8) for k in keys["first_digit"]}) > 100 and np.isfinite(col["first_digit"]).all()


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """every case, the sampler's chain and the failures, in one child process"""
    out = str(tmp_path_factory.mktemp("quantile_device") / "device.npz")
    spec = dict(cases=CASES, sampler=True, errors=True)
    r = subprocess.run([sys.executable, "-m", "tests.quantile_device", json.dumps(spec), out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "quantile_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_restatement(name, device):
    spec, w = CASES[name], _want(name)
    N = used_count(spec)
    ranks = np.array(w["ranks"])
    for prefix in ("host_", "dev_") if spec.get("device", True) else ("host_",):
        got = device[name + "/" + prefix + "values"]
        assert _same(got, w["values"]), prefix
        np.testing.assert_array_equal(device[name + "/" + prefix + "below"], w["counts"][0])
        np.testing.assert_array_equal(device[name + "/" + prefix + "not_above"], w["counts"][1])
    if spec.get("device", True):
        # for every order statistic v returned for rank r: below(v) <= r < not_above(v)
        below, not_above = device[name + "/dev_value_below"], device[name + "/dev_value_not_above"]
        assert below.shape == (spec["P"], len(ranks)) and (below <= ranks).all() and (ranks < not_above).all() and (not_above <= N).all()
        want = qr.rank_counts(w["steps"], w["values"], spec["slice"])
        np.testing.assert_array_equal(below, want[0])
        np.testing.assert_array_equal(not_above, want[1])
    q = w["queries"]
    below, not_above = w["counts"]
    assert (below[:, 0] < not_above[:, 0]).all()                       # equal to a sample
    np.testing.assert_array_equal(below[:, 3], below[:, 4])            # -0 and +0
    np.testing.assert_array_equal(not_above[:, 3], not_above[:, 4])
    assert (below[:, 5] == 0).all() and (not_above[:, 6] == N).all() and q.shape == (spec["P"], 7)


@pytest.mark.gpu
def test_forced_chunks_give_the_one_chunk_result(device):
    a, b = CASES["chunked"], CASES["one_chunk"]
    assert a["n"] * a["W"] * a["P"] * 8 > 5 * 2 ** 20 and a["chunk_mb"] == 1 and "chunk_mb" not in b  # 5.4 MB in chunks of 1 MB
    for key in ("host_values", "host_below", "host_not_above"):
        assert _same(device["chunked/" + key], device["one_chunk/" + key]), key


@pytest.mark.gpu
def test_the_cases_take_every_launch_path_on_this_device(device):
    exe = build_driver()
    lds = min(int(device["shared_mem_per_block"]), 65536)
    seen = set()
    for name in CASES:
        taken = _paths(exe, name, int(device["cus"]), lds)
        seen |= set(taken)
        if name in PATHS and lds == 65536:
            assert set(taken) >= PATHS[name], (name, taken)
    assert seen >= {(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1)}, seen


@pytest.mark.gpu
def test_quantiles_of_a_chain_the_sampler_wrote(device):
    chain, q = device["sampler/chain"], device["sampler/q"]
    assert chain.shape == (200, 64, 4) and len(np.unique(chain[:, :, 0])) > 1000
    for method in ("linear", "lower", "higher"):
        assert _same(device["sampler/" + method], qr.quantiles(chain, q, method)), method
    assert _same(device["sampler/linear_slice3"], qr.quantiles(chain, q, "linear", 3))
    np.testing.assert_allclose(device["sampler/linear"], np.quantile(chain.reshape(-1, 4), q, axis=0).T, rtol=1e-12)


@pytest.mark.gpu
def test_failures_are_clean_and_the_next_call_succeeds(device):
    for name, word in (("nan_sample", "NaN"), ("nan_sample_counts", "NaN"), ("nan_query", "NaN"), ("rank_n", "rank 280"), ("host_pointer", "device"),
                       ("host_pointer_counts", "device"), ("past_the_end", "allocation")):
        assert device["errors/%s_raised" % name] == 1, name
        assert device["errors/%s_code" % name] == 1 and word in str(device["errors/%s_message" % name]), (name, str(device["errors/%s_message" % name]))
        assert device["errors/%s_untouched" % name] == 1, name
    steps = device["errors/steps"]
    want = qr.order_statistics(steps, [0, 140])
    assert _same(device["errors/after_values"], want) and _same(device["errors/after_dev_values"], want)
    below, not_above = qr.rank_counts(steps, np.zeros((3, 1)))
    np.testing.assert_array_equal(device["errors/after_below"], below)
    np.testing.assert_array_equal(device["errors/after_not_above"], not_above)


def _read_facade(raw):
    W, P, n, sl, K, nv = struct.unpack_from("6i", raw, 0)
    off = [24]

    def take(count, dt=np.float64):
        a = np.frombuffer(raw, dt, count, off[0])
        off[0] += a.nbytes
        return a

    chain = take(n * W * P).reshape(n, W, P)
    pct = take(K)
    sel = take(P * K * 3).reshape(P, K, 3)
    values = take(P * nv).reshape(P, nv)
    counts = np.frombuffer(raw, np.dtype([("below", np.int64), ("not_above", np.int64), ("percentile", np.float64)]), P * nv, off[0]).reshape(P, nv)
    off[0] += counts.nbytes
    points = take(1, np.int64)[0]
    assert off[0] == len(raw)
    return chain, sl, pct, sel, values, counts, points


@pytest.mark.gpu
def test_facade_class_on_device_pinned_and_downloaded_chains(tmp_path):
    """tests/cpp/exact_percentiles_facade.cpp with the chain in device memory, in pinned host memory, and in device memory with the
    device path switched off: the same bytes from all three, and the restatement's values for the chain the program wrote"""
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "exact_percentiles_facade.cpp"), "exact_percentiles_facade")
    runs = {}
    for tag, env in (("device", dict(MCMCPP_CHAIN_MEMORY="device")), ("pinned", dict(MCMCPP_CHAIN_MEMORY="pinned")),
                     ("downloaded", dict(MCMCPP_CHAIN_MEMORY="device", MCMCPP_DEVICE_ANALYSIS="0"))):
        outp = tmp_path / (tag + ".bin")
        e = {k: v for k, v in os.environ.items() if k not in ("MCMCPP_CHAIN_MEMORY", "MCMCPP_DEVICE_ANALYSIS")}
        r = subprocess.run([exe, str(outp)], capture_output=True, text=True, timeout=300, env=dict(e, **env))
        assert r.returncode == 0 and "exact_percentiles_facade OK" in r.stdout, tag + r.stdout + r.stderr
        runs[tag] = (r.stdout, outp.read_bytes())
    assert runs["device"] == runs["pinned"] == runs["downloaded"]
    chain, sl, pct, sel, values, counts, points = _read_facade(runs["device"][1])
    assert chain.shape == (201, 64, 4) and sl == 3 and points == 67 * 64  # the initial positions and 200 steps; every third: 67
    q = pct / 100.0
    for k, method in enumerate(("lower", "higher", "linear")):
        assert _same(np.ascontiguousarray(sel[:, :, k]), qr.quantiles(chain, q, method, sl)), method
    below, not_above = qr.rank_counts(chain, values, sl)
    np.testing.assert_array_equal(counts["below"], below)
    np.testing.assert_array_equal(counts["not_above"], not_above)
    assert _same(np.ascontiguousarray(counts["percentile"]), 100.0 * below.astype(np.float64) / np.float64(points))
    assert (below[:, :len(pct)] <= np.floor(q * (points - 1))).all() and (np.floor(q * (points - 1)) < not_above[:, :len(pct)]).all()
    assert (not_above[:, -2] == 0).all() and (below[:, -1] == points).all()


@pytest.mark.gpu
def test_percentiles_example_runs():
    exe = _compile(os.path.join(ROOT, "examples", "skewed_gaussian_percentiles.cpp"), "skewed_gaussian_percentiles")
    r = subprocess.run([exe, "2019"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "samples of each parameter" in r.stdout and r.stdout.count(" | ") == 14
