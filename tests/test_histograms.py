"""Chain analysis: Analysis::CornerHistograms and Analysis::PercentileAndMaximumFinder.

CPU: the restatement (tests/histogram_restatement.py) reproduces fixtures the reference's own classes produced
(tests/golden/make_histogram_golden.py) bit for bit -- histograms, bounds, query values, CSV text; and a program written
like the reference test's analysis section compiles against include/MCMCpp.
GPU: the device (mcmcpp_hip_histograms_*, through the C ABI and through the facade headers) reproduces the fixtures
exactly, and the restatement exactly on ragged and larger shapes, positive data (clamped bins), many upload chunks and a
chain the sampler wrote into device memory.  PATHS walks the launch paths of histograms.hip (mcmcpp_amd/csrc/hist_plan.hpp
chooses among them by bins, pairs and the device's CU count): each case asks the plan which path its shape takes on the
device at hand and fails where that is not the one it is named for.  Cases with `edges` put samples on the bin edges and
one step of T beside them, where a bin decides between two counters.  Every GPU step runs in a child process under its own
time limit."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mcmcpp_amd import capi
from tests import histogram_restatement as hr
from tests.goldens import GOLDEN_DIR
from tests.histogram_device import make_steps
from tests.test_hist_plan import build_driver, plan_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["hist_skewed320x2", "hist_skewed320x2_f32", "hist_96x5_slice3", "hist_96x5_slice3_f32", "hist_40x3_bins2",
            "hist_16x3_csv"]
CSV_FIXTURE = "hist_16x3_csv"


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def _same(a, b):
    """bit for bit, NaNs included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _restated_queries(z, bounds, single, num_points):
    T = bounds.dtype.type
    cs = hr.cum_sums(single)
    P = bounds.shape[0]
    pfv = np.array([[hr.percentile_from_value(bounds, cs, num_points, p, v) for v in z["value_queries"][p]] for p in range(P)], T)
    vfp = np.array([[hr.value_from_percentile(bounds, cs, num_points, p, q) for q in z["percentile_queries"][p]] for p in range(P)], T)
    peak = np.array([hr.value_of_peak(bounds, single, p) for p in range(P)], T)
    pmax = np.array([T(T(bounds[p, 0]) + T(T(bounds[p, 1]) * T(single.shape[1]))) for p in range(P)], T)
    return pfv, vfp, peak, pmax


# ---- CPU ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_fixture(name):
    z = _load(name)
    steps, sl = z["steps"], int(z["slice_interval"])
    assert (steps <= 0).all()  # the inputs keep the reference defined
    c = hr.histograms(steps, int(z["corner_bins"]), sl, True)
    f = hr.histograms(steps, int(z["finder_bins"]), sl, False)
    assert _same(c["bounds"], z["corner_bounds"]) and _same(f["bounds"], z["finder_bounds"])
    np.testing.assert_array_equal(c["single"], z["corner_single"])
    np.testing.assert_array_equal(c["pairs"], z["corner_pairs"])
    np.testing.assert_array_equal(f["single"], z["finder_single"])
    np.testing.assert_array_equal(hr.cum_sums(f["single"]), z["finder_cumsum"])
    assert f["num_points"] == z["num_points"] and c["clamped"].sum() == 0 and f["clamped"].sum() == 0
    pfv, vfp, peak, pmax = _restated_queries(z, f["bounds"], f["single"], f["num_points"])
    assert _same(pfv, z["percentile_from_value"])
    assert _same(vfp, z["value_from_percentile"])
    assert _same(peak, z["peak"])
    assert _same(f["bounds"][:, 0], z["param_minimum"]) and _same(pmax, z["param_maximum"])


def _restated_csv(z):
    c = hr.histograms(z["steps"], int(z["corner_bins"]), int(z["slice_interval"]), True)
    f = hr.histograms(z["steps"], int(z["finder_bins"]), int(z["slice_interval"]), False)
    files = {"corner" + k: v for k, v in hr.corner_csv(c["bounds"], c["single"], c["pairs"]).items()}
    files.update({"finder" + k: v for k, v in hr.percentile_csv(f["bounds"], f["single"]).items()})
    return files


def test_restatement_reproduces_the_reference_csv_files():
    with open(os.path.join(GOLDEN_DIR, CSV_FIXTURE + ".json")) as fh:
        want = json.load(fh)
    assert len(want) == 3 + 3 + 2 * 3
    assert _restated_csv(_load(CSV_FIXTURE)) == want


def test_restatement_clamps_and_counts_out_of_range_bins():
    x = np.array([[[1.0, 0.0], [2.0, 0.0], [3.0, 0.0]]])  # positive maximum; an all-zero parameter
    r = hr.histograms(x, 4)
    # the reference's tweak puts 3.0 above its top edge (2.997) and 0 exactly at bins: both clamped into the last bin
    np.testing.assert_array_equal(r["clamped"], [1, 3])
    np.testing.assert_array_equal(r["single"], [[1, 0, 1, 1], [0, 0, 0, 3]])


def _compile(src, out):
    from tests.test_facade import BUILD, INC, LINK
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, out)
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(dp, f))
                                            for dp, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        capi.build_library()
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"] + INC + [src, "-o", exe] + LINK)
    return exe


def test_reference_style_analysis_program_compiles():
    """the reference test's analysis section (AutoCorrCalc, CovarianceMatrix, CornerHistograms,
    PercentileAndMaximumFinder), and the facade test programs, compile and link against include/MCMCpp with -Werror"""
    _compile(os.path.join(ROOT, "examples", "skewed_gaussian_analysis.cpp"), "skewed_gaussian_analysis")
    _compile(os.path.join(ROOT, "tests", "cpp", "histograms_facade.cpp"), "histograms_facade")
    _compile(os.path.join(ROOT, "tests", "cpp", "histograms_fixture.cpp"), "histograms_fixture")


def test_exports_and_chunk_knob_are_declared():
    with open(os.path.join(ROOT, "include", "mcmcpp_hip.h")) as fh:
        header = fh.read()
    for name in ("mcmcpp_hip_histograms_create", "mcmcpp_hip_histograms_compute", "mcmcpp_hip_histograms_compute_device",
                 "mcmcpp_hip_histograms_result", "mcmcpp_hip_histograms_destroy", "mcmcpp_hip_histograms_last_error"):
        assert name + "(" in header and name in capi.EXPORTS
    assert "MCMCPP_HIP_HIST_CHUNK_MB" in header


# The launch paths of histograms.hip, by the plan's numbers on a device of 256 CUs and 64 KiB of LDS for a block.
# name: (spec, element types, what the plan must say).  n = W x (steps used).
PATHS = {
    # 33 153 pairs in 519 tiles of 64, one pair in the last; hist_bounds_kernel's second round of parameters with pt = 2
    "tile64_ragged": (dict(W=70, n=6, P=258, bins=4), ("f64", "f32"), dict(pair_lds=1, tile=64, tiles=519, last_count=1, pair_blocks=1)),
    # 32 896 pairs in 514 full tiles; second round with pt = 1
    "tile64_full": (dict(W=70, n=6, P=257, bins=4), ("f64", "f32"), dict(pair_lds=1, tile=64, tiles=514, last_count=64, pair_blocks=1)),
    # the same tiles over two slices of 4500 samples (17 rounds of 256 threads and 148 more)
    "tile64_two_slices": (dict(W=300, n=30, P=258, bins=4), ("f64",), dict(pair_lds=1, tile=64, tiles=519, last_count=1, pair_blocks=2, pair_per=4500)),
    "tile8": (dict(W=100, n=6, P=92, bins=3), ("f64", "f32"), dict(pair_lds=1, tile=8, tiles=524, last_count=2)),
    # two 90 x 90 histograms (64 800 bytes) just fit, three would not; 67 MB of counters
    "tile2_lds_bound": (dict(W=100, n=6, P=47, bins=90), ("f64", "f32"), dict(pair_lds=1, tile=2, tiles=541, last_count=1, pair_lds_bytes=64800)),
    "tile1_after_90": (dict(W=100, n=6, P=47, bins=91), ("f64", "f32"), dict(pair_lds=1, tile=1, tiles=1081, pair_lds_bytes=33124)),
    "pairs_lds_exact": (dict(W=100, n=6, P=3, bins=128), ("f64", "f32"), dict(pair_lds=1, tile=1, pair_lds_bytes=65536)),
    "pairs_global": (dict(W=100, n=6, P=3, bins=129), ("f64", "f32"), dict(pair_lds=0, tile=1, pair_lds_bytes=0)),
    "single_lds_exact": (dict(W=250, n=20, P=2, bins=16384, pairs=False, edges=True), ("f64", "f32"), dict(single_lds=1, single_lds_bytes=65536, idx_bytes=2)),
    "single_global": (dict(W=250, n=20, P=2, bins=16385, pairs=False, edges=True), ("f64", "f32"), dict(single_lds=0, single_lds_bytes=0, single_blocks=4)),
    # the largest index a type holds (255, 65 535) and the first shape of the next type, with the top bins filled
    "idx_u8_top": (dict(W=300, n=4, P=2, bins=256, edges=True), ("f64", "f32"), dict(idx_bytes=1, pair_lds=0)),
    "idx_u16_first": (dict(W=300, n=4, P=2, bins=257, edges=True), ("f64", "f32"), dict(idx_bytes=2, pair_lds=0)),
    "idx_u16_top": (dict(W=300, n=4, P=2, bins=65536, pairs=False, edges=True), ("f64", "f32"), dict(idx_bytes=2, single_lds=0)),
    "idx_u32_first": (dict(W=300, n=4, P=2, bins=65537, pairs=False, edges=True), ("f64", "f32"), dict(idx_bytes=4, single_lds=0)),
}
PATH_CASES = [(name, dt) for name, (_, dts, _) in PATHS.items() for dt in dts]
PATH_SEED = 7


def _path_spec(name, dtype):
    return dict(PATHS[name][0], kind="random", slice=1, seed=PATH_SEED, dtype=dtype)


def _plan_on(exe, spec, cus, lds):
    used = (spec["n"] + spec.get("slice", 1) - 1) // spec.get("slice", 1)
    return plan_of(exe, n=spec["W"] * used, P=spec["P"], bins=spec["bins"], pairs=int(spec.get("pairs", True)), cus=cus, lds=lds)


def test_the_path_cases_take_their_paths_on_256_cus():
    """the table above, on the CU count and LDS size it was worked out for; between them the cases take every path the plan has
    but the split of the pair launch along grid.y (tests/test_hist_plan.py: no case of a few seconds reaches it)"""
    exe = build_driver()
    plans = {}
    for name, (spec, _, want) in PATHS.items():
        plans[name] = p = _plan_on(exe, spec, 256, 65536)
        assert {k: p[k] for k in want} == want, name
        assert p["pair_launches"] == (1 if spec.get("pairs", True) else 0)
    assert {p["tile"] for p in plans.values()} == {0, 1, 2, 8, 64}
    assert {p["idx_bytes"] for p in plans.values()} == {1, 2, 4}
    assert {(p["single_lds"], p["single_blocks"] > 1) for p in plans.values()} >= {(1, False), (0, True)}
    assert {(p["pair_lds"], p["pair_blocks"] > 1) for p in plans.values() if p["npairs"]} >= {(1, False), (1, True), (0, False)}


EDGE_SPECS = [dict(W=300, n=4, P=2, bins=b, slice=1, seed=PATH_SEED, dtype=dt) for dt in ("f64", "f32") for b in (256, 257, 16384, 16385, 65536, 65537)] + [
    dict(W=250, n=20, P=2, bins=16384, slice=1, seed=PATH_SEED, dtype="f32"),
    dict(W=97, P=7, n=10, bins=257, slice=3, dtype="f64", seed=104), dict(W=130, P=2, n=12, bins=100, slice=2, dtype="f32", seed=132)]


@pytest.mark.parametrize("spec", EDGE_SPECS, ids=lambda s: "W%(W)dP%(P)dbins%(bins)d_%(dtype)s" % s)
def test_edge_data_sits_on_the_bin_edges_and_leaves_the_bounds_alone(spec):
    """what the GPU cases with `edges` rest on, from the restatement alone: they cannot pass for want of such samples"""
    plain, x = make_steps(spec), make_steps(dict(spec, edges=True))
    sl, bins, P = spec["slice"], spec["bins"], spec["P"]
    assert (x <= 0).all() and (x != plain).sum() > 100 * P and (x[::sl] != plain[::sl]).sum() == (x != plain).sum()
    r = hr.histograms(x, bins, sl, False)
    assert _same(r["bounds"], hr.find_binning(plain[::sl], bins))  # the bounds are the undisturbed data's
    assert (r["single"][:, -1] > 0).all()                            # the top bin of every parameter holds samples
    np.testing.assert_array_equal(r["clamped"], [2] * P)             # the top edge and its upper neighbour, nothing else
    T = x.dtype.type
    q = ((x[::sl].reshape(-1, P) - r["bounds"][:, 0]) / r["bounds"][:, 1]).astype(T)
    assert (np.abs(q - np.rint(q)) <= 2 * np.spacing(np.abs(q))).sum() > 100  # quotients within 2 ulp of an integer
    assert (q == np.rint(q)).sum() > 20 and (np.rint(q) > q).sum() > 20      # on an edge exactly, and just below one


# ---- GPU ----------------------------------------------------------------------------------------------------------

def _device(spec, tmp_path, timeout=300):
    out = str(tmp_path / "device.npz")
    r = subprocess.run([sys.executable, "-m", "tests.histogram_device", json.dumps(spec), out], cwd=ROOT, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0 and "histogram_device OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_matches_the_reference_fixture(name, tmp_path):
    z = _load(name)
    d = _device(dict(kind="fixture", name=name), tmp_path)
    assert _same(d["corner_bounds"], z["corner_bounds"]) and _same(d["finder_bounds"], z["finder_bounds"])
    np.testing.assert_array_equal(d["corner_single"], z["corner_single"])
    np.testing.assert_array_equal(d["corner_pairs"], z["corner_pairs"])
    np.testing.assert_array_equal(d["finder_single"], z["finder_single"])
    assert d["corner_num_points"] == z["num_points"] == d["finder_num_points"]
    assert d["corner_clamped"].sum() == 0 and d["finder_clamped"].sum() == 0


def _write_driver_input(z, path):
    steps, vq, pq = z["steps"], z["value_queries"], z["percentile_queries"]
    n, W, P = steps.shape
    with open(path, "wb") as fh:
        fh.write(struct.pack("9i", 0 if steps.dtype == np.float64 else 1, W, P, n, int(z["slice_interval"]), int(z["corner_bins"]),
                             int(z["finder_bins"]), vq.shape[1], pq.shape[1]))
        fh.write(steps.tobytes() + vq.tobytes() + pq.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_facade_matches_the_reference_fixture(name, tmp_path):
    """include/MCMCpp/Analysis/{CornerHistograms,PercentileAndMaximumFinder}.h over a Chain holding the fixture's steps"""
    z = _load(name)
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "histograms_fixture.cpp"), "histograms_fixture")
    inp, outp, csv = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "csv"
    csv.mkdir()
    _write_driver_input(z, inp)
    r = subprocess.run([exe, str(inp), str(outp), str(csv)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "histograms_fixture OK" in r.stdout, r.stdout + r.stderr
    steps = z["steps"]
    T = steps.dtype.type
    P = steps.shape[2]
    cb, pb = int(z["corner_bins"]), int(z["finder_bins"])
    got = np.fromfile(str(outp), dtype=T, count=-1)
    k = [0]

    def take(count):
        a = got[k[0]:k[0] + count]
        k[0] += count
        return a

    cbounds = z["corner_bounds"]
    edges = np.array([[cbounds[p, 0], T(cbounds[p, 0] + T(T(cb) * cbounds[p, 1]))] for p in range(P)], T)
    assert _same(take(2 * P).reshape(P, 2), edges)
    assert _same(take(P * cb).reshape(P, cb), z["corner_single"].astype(T))
    npairs = P * (P - 1) // 2
    assert _same(take(npairs * cb * cb).reshape(npairs, cb, cb), z["corner_pairs"].astype(T))
    assert _same(take(z["percentile_from_value"].size).reshape(P, -1), z["percentile_from_value"])
    assert _same(take(z["value_from_percentile"].size).reshape(P, -1), z["value_from_percentile"])
    assert _same(take(P), z["peak"])
    assert _same(take(P), z["param_minimum"])
    assert _same(take(P), z["param_maximum"])
    clamped = np.frombuffer(got[k[0]:].tobytes(), np.int64)
    np.testing.assert_array_equal(clamped, np.zeros(2 * P, np.int64))
    if name == CSV_FIXTURE:
        with open(os.path.join(GOLDEN_DIR, CSV_FIXTURE + ".json")) as fh:
            want = json.load(fh)
        assert {f: open(os.path.join(str(csv), f)).read() for f in os.listdir(str(csv))} == want


def _check_against_restatement(d, steps, bins, sl, pairs, prefix):
    want = hr.histograms(steps, bins, sl, pairs)
    assert d[prefix + "num_points"] == want["num_points"]
    assert _same(d[prefix + "bounds"], want["bounds"])
    np.testing.assert_array_equal(d[prefix + "single"], want["single"])
    np.testing.assert_array_equal(d[prefix + "clamped"], want["clamped"])
    if pairs:
        np.testing.assert_array_equal(d[prefix + "pairs"], want["pairs"])
    return want


RAGGED = [
    # W not a multiple of 64; P in {1, 2, 7, 32, 33}; bins in {2, 100, 257, 10 000}; slice > 1
    dict(W=70, P=1, n=9, bins=2, slice=1, dtype="f64"),
    dict(W=130, P=2, n=12, bins=100, slice=2, dtype="f32", edges=True),
    dict(W=97, P=7, n=10, bins=257, slice=3, dtype="f64", edges=True),
    dict(W=200, P=32, n=6, bins=100, slice=1, dtype="f64"),
    dict(W=65, P=33, n=8, bins=16, slice=2, dtype="f32"),
    dict(W=150, P=7, n=7, bins=10000, slice=1, dtype="f32", pairs=False),
    dict(W=333, P=2, n=5, bins=10000, slice=2, dtype="f64", pairs=False),
    dict(W=64, P=33, n=4, bins=100, slice=1, dtype="f64"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("spec", RAGGED, ids=lambda s: "W%(W)dP%(P)dbins%(bins)d_%(dtype)s" % s)
def test_device_equals_restatement_on_ragged_shapes(spec, tmp_path):
    d = _device(dict(spec, kind="random", seed=spec["W"] + spec["P"]), tmp_path)
    steps = d["steps"]
    for prefix in ("host_", "dev_"):
        w = _check_against_restatement(d, steps, spec["bins"], spec["slice"], spec.get("pairs", True), prefix)
        # (edge data: the top edge and its upper neighbour lie at `bins` and above -- test_edge_data_sits_on_the_bin_edges...)
        np.testing.assert_array_equal(w["clamped"], [2 if spec.get("edges") else 0] * spec["P"])


def _check_result(d, want, prefix):
    assert d[prefix + "num_points"] == want["num_points"]
    assert _same(d[prefix + "bounds"], want["bounds"])
    np.testing.assert_array_equal(d[prefix + "single"], want["single"])
    np.testing.assert_array_equal(d[prefix + "clamped"], want["clamped"])
    if want["pairs"] is not None:
        np.testing.assert_array_equal(d[prefix + "pairs"], want["pairs"])
    else:
        assert prefix + "pairs" not in d


@pytest.fixture(scope="module")
def device_plan(tmp_path_factory):
    """spec -> the plan of its launches on the device the cases run on"""
    info = _device(dict(kind="device_info"), tmp_path_factory.mktemp("device_info"))
    exe = build_driver()
    lds = int(subprocess.run([exe, "lds", "shared=%d" % int(info["shared_mem_per_block"])], capture_output=True, text=True, check=True).stdout)
    return lambda spec: _plan_on(exe, spec, int(info["cus"]), lds)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", PATH_CASES, ids=["%s_%s" % c for c in PATH_CASES])
def test_device_equals_restatement_on_every_launch_path(name, dtype, device_plan, tmp_path):
    spec, named = _path_spec(name, dtype), PATHS[name][2]
    plan = device_plan(spec)
    assert {k: plan[k] for k in named} == named, "on this device %s takes another path than the one it is named for: %r" % (name, plan)
    d = _device(spec, tmp_path)
    steps = d["steps"]
    assert _same(steps, make_steps(spec))
    want = hr.histograms(steps, spec["bins"], 1, spec.get("pairs", True))
    if spec.get("edges"):
        assert (want["single"][:, -1] > 0).all() and (want["clamped"] == 2).all()
    else:
        assert want["clamped"].sum() == 0
    for prefix in ("host_", "dev_"):
        _check_result(d, want, prefix)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n,sl", [(0, 1), (3, 5)], ids=["no_steps", "one_step_of_three"])
def test_nothing_or_one_step_selected(n, sl, dtype, tmp_path):
    """no stored step at all: empty histograms over the bounds the analysis classes' start values give; slice 5 of 3 steps: the first"""
    spec = dict(kind="random", W=70, n=n, P=3, bins=16, slice=sl, dtype=dtype, seed=PATH_SEED)
    d = _device(spec, tmp_path)
    want = hr.histograms(d["steps"], 16, sl, True)
    assert want["num_points"] == (70 if n else 0) and d["steps"].shape == (n, 70, 3)
    for prefix in ("host_", "dev_"):
        _check_result(d, want, prefix)
        assert d[prefix + "single"].sum() == 3 * want["num_points"] and d[prefix + "pairs"].sum() == 3 * want["num_points"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_positive_data_is_clamped_and_counted_like_the_restatement(dtype, tmp_path):
    spec = dict(kind="random", W=90, P=5, n=11, bins=40, slice=1, dtype=dtype, positive=True, constant=[3], constant_value=2.5,
                zero=[4])
    d = _device(spec, tmp_path)
    for prefix in ("host_", "dev_"):
        w = _check_against_restatement(d, d["steps"], 40, 1, True, prefix)
        assert (w["clamped"][:3] > 0).all() and w["clamped"][3] == 0 and w["clamped"][4] == 90 * 11


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_degenerate_parameters(dtype, tmp_path):
    """a negative constant, a zero parameter (clamped at the top: 0 lands at exactly `bins`)"""
    spec = dict(kind="random", W=77, P=4, n=6, bins=10, slice=1, dtype=dtype, constant=[1], zero=[2])
    d = _device(spec, tmp_path)
    for prefix in ("host_", "dev_"):
        w = _check_against_restatement(d, d["steps"], 10, 1, True, prefix)
        assert w["clamped"][2] == 77 * 6 and w["clamped"][[0, 1, 3]].sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_many_upload_chunks_give_the_same_counts(dtype, tmp_path):
    # one step is 2000 * 33 elements (264 / 528 KB); a 1 MB chunk holds one to three of them: 25 selected steps, many chunks
    spec = dict(kind="random", W=2000, P=33, n=50, bins=20, slice=2, dtype=dtype, chunk_mb=1)
    d = _device(spec, tmp_path)
    for prefix in ("host_", "dev_"):
        _check_against_restatement(d, d["steps"], 20, 2, True, prefix)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,sl", [("f64", 1), ("f32", 3)])
def test_device_chain_written_by_the_sampler(dtype, sl, tmp_path):
    d = _device(dict(kind="device_chain", W=300, P=6, n=40, bins=50, slice=sl, dtype=dtype), tmp_path)
    _check_against_restatement(d, d["steps"], 50, sl, True, "dev_")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_and_oversize_requests_fail_cleanly(dtype, tmp_path):
    d = _device(dict(kind="errors", dtype=dtype), tmp_path)
    assert d["nan_raised"] == 1 and d["nan_code"] == 1 and "NaN" in str(d["nan_message"])
    assert d["result_after_failure"] == 0
    _check_against_restatement(d, d["steps"], 16, 1, True, "after_")
    assert d["oversize_raised"] == 1 and d["oversize_code"] == 6 and "byte" in str(d["oversize_message"])
    _check_against_restatement(d, d["steps"], 16, 1, True, "later_")


@pytest.mark.gpu
def test_facade_program_against_the_restatement(tmp_path):
    """tests/cpp/histograms_facade.cpp: both classes on chains the facade's sampler produced, every getter and CSV file
    against the restatement of the same chain"""
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "histograms_facade.cpp"), "histograms_facade")
    outp = tmp_path / "out.bin"
    r = subprocess.run([exe, str(outp), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "histograms_facade OK" in r.stdout, r.stdout + r.stderr
    raw = outp.read_bytes()
    off = 0
    for tag in ("f64", "f64_slice3", "f32"):
        dt_code, W, P, n, sl, cb, pb, nv, npq = struct.unpack_from("9i", raw, off)
        off += 36
        T = np.float64 if dt_code == 0 else np.float32
        size = np.dtype(T).itemsize

        def take(count, dt=T):
            nonlocal off
            a = np.frombuffer(raw, dt, count, off)
            off += a.nbytes
            return a

        steps = take(n * W * P).reshape(n, W, P)
        c = hr.histograms(steps, cb, sl, True)
        f = hr.histograms(steps, pb, sl, False)
        lo, w = c["bounds"][:, 0], c["bounds"][:, 1]
        edges = np.array([[lo[p], T(lo[p] + T(T(1) * w[p])), T(lo[p] + T(T(cb - 1) * w[p])), T(lo[p] + T(T(cb) * w[p]))]
                          for p in range(P)], T)
        assert _same(take(4 * P).reshape(P, 4), edges), tag
        assert _same(take(P * cb).reshape(P, cb), c["single"].astype(T)), tag
        npairs = P * (P - 1) // 2
        assert _same(take(npairs * cb * cb).reshape(npairs, cb, cb), c["pairs"].astype(T)), tag
        np.testing.assert_array_equal(take(P, np.int64), c["clamped"])
        fb = f["bounds"]
        assert _same(take(P), fb[:, 0])
        assert _same(take(P), np.array([T(fb[p, 0] + T(fb[p, 1] * T(pb))) for p in range(P)], T))
        np.testing.assert_array_equal(take(P, np.int64), f["clamped"])
        cs = hr.cum_sums(f["single"])
        pairs = take(P * nv * 2).reshape(P, nv, 2)
        for p in range(P):
            for v, got in pairs[p]:
                assert _same(T(got), hr.percentile_from_value(fb, cs, f["num_points"], p, v)), (tag, p, v)
        pairs = take(P * npq * 2).reshape(P, npq, 2)
        for p in range(P):
            for q, got in pairs[p]:
                assert _same(T(got), hr.value_from_percentile(fb, cs, f["num_points"], p, q)), (tag, p, q)
        assert _same(take(P), np.array([hr.value_of_peak(fb, f["single"], p) for p in range(P)], T))
        files = {tag + "_corner" + k: v for k, v in hr.corner_csv(c["bounds"], c["single"], c["pairs"]).items()}
        files.update({tag + "_finder" + k: v for k, v in hr.percentile_csv(fb, f["single"]).items()})
        for fname, text in files.items():
            assert (tmp_path / fname).read_text() == text, fname
        assert size in (4, 8)
    assert off == len(raw)


@pytest.mark.gpu
def test_analysis_example_runs(tmp_path):
    exe = _compile(os.path.join(ROOT, "examples", "skewed_gaussian_analysis.cpp"), "skewed_gaussian_analysis")
    r = subprocess.run([exe, "2019", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "The 15.9, 50, 84.1 percentiles are:" in r.stdout
    assert (tmp_path / "chainHist_p1_p0.csv").exists() and (tmp_path / "percentileHistograms_cs_p1.csv").exists()
