"""Chain analysis: Analysis::CovarianceMatrix.

CPU: the oracle's restatement (oracle/stretch_oracle_typed.inc: chain_covariance) against fixtures produced by the
reference's own CovarianceMatrix over its own Chain (tests/golden/make_golden.py covariance) -- bit for bit.
GPU: the device accumulation (mcmcpp_hip_moments_*, matrix cores) against the oracle.  The reference's sequential
Kahan sums cannot be kept by a parallel sum, so the bar is a stated tolerance: every covariance element within
1e-10 * sqrt(var_i var_j) (fp64) of the oracle's, every correlation element within 1e-10; for fp32 chains 2e-4,
which is the accuracy of the reference's own fp32 arithmetic (the device accumulates fp32 samples in fp64 and is the
more accurate of the two: it is also checked against an fp64 computation at 1e-6).

Below the first tests, the device is also held to an error bar that scales with the data (tests/moments_reference.py):
an np.longdouble two-pass reference, and a bar of 4 times the larger of the oracle's own measured error and
2**-52 (|m_i m_j| + s_i s_j) -- over offset data, constant parameters, every tile count of the matrix-core kernel in
both types, few samples, the widest parameter sets, chunked uploads (MCMCPP_HIP_MOMENTS_CHUNK_MB) and a NaN sample."""
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po
from tests.goldens import GOLDEN_DIR
from tests.moments_reference import MARGIN, U, Reference, exact_moments, holds, ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["covariance_dense96x16", "covariance_dense96x16_slice5", "covariance_rosen80x8", "covariance_dense80x5_f32"]


def _fixture(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return z["steps"], int(z["slice_interval"]), z["cov"], z["corr"]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_covariance_matches_the_reference_bit_for_bit(name):
    steps, sl, cov, corr = _fixture(name)
    mean, c, r = po.chain_covariance(steps, sl)
    np.testing.assert_array_equal(c, cov)
    np.testing.assert_array_equal(r, corr)
    used = steps[::sl].reshape(-1, steps.shape[2]).astype(np.float64)
    np.testing.assert_allclose(mean, used.mean(axis=0), rtol=1e-5 if steps.dtype == np.float32 else 1e-12, atol=1e-6)


def _close(got_cov, got_corr, cov, corr, tol):
    scale = np.sqrt(np.abs(np.outer(np.diag(cov), np.diag(cov)))).astype(np.float64)
    assert np.all(np.abs(got_cov.astype(np.float64) - cov) <= tol * scale), np.abs(got_cov - cov).max()
    assert np.all(np.abs(got_corr.astype(np.float64) - corr) <= tol), np.abs(got_corr - corr).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_covariance_matches_the_reference_fixture(name):
    steps, sl, cov, corr = _fixture(name)
    f32 = steps.dtype == np.float32
    m = capi.HipMoments(steps.shape[1], steps.shape[2], dtype=capi.F32 if f32 else capi.F64)
    m.add_steps(steps, sl)
    n, mean, c, r = m.finish()
    assert n == len(steps[::sl]) * steps.shape[1]
    _close(c, r, cov, corr, 2e-4 if f32 else 1e-10)


@pytest.mark.gpu
@pytest.mark.parametrize("W,D,n,sl,dt", [
    (10, 1, 50, 1, np.float64), (34, 2, 40, 3, np.float64), (100, 7, 30, 1, np.float64), (64, 16, 25, 2, np.float64),
    (70, 17, 20, 1, np.float64), (4098, 32, 6, 1, np.float64), (130, 33, 12, 5, np.float64), (200, 64, 9, 2, np.float64),
    (150, 65, 7, 1, np.float64),      # beyond the matrix-core path: generic kernel
    (300, 130, 4, 1, np.float64), (96, 5, 60, 2, np.float32), (128, 32, 20, 1, np.float32), (40, 70, 10, 3, np.float32)])
def test_device_covariance_matches_the_oracle(W, D, n, sl, dt):
    rng = np.random.default_rng(W * 131 + D)
    mix = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    steps = (rng.standard_normal((n, W, D)) @ mix + rng.standard_normal(D) * 3).astype(dt)
    f32 = dt == np.float32
    _, cov, corr = po.chain_covariance(steps, sl)
    m = capi.HipMoments(W, D, dtype=capi.F32 if f32 else capi.F64)
    m.add_steps(steps, sl)
    npts, mean, c, r = m.finish()
    assert npts == len(steps[::sl]) * W
    _close(c, r, cov, corr, 2e-4 if f32 else 1e-10)
    # against an independent fp64 computation (for fp32 chains the device is the more accurate of the two)
    used = steps[::sl].reshape(-1, D).astype(np.float64)
    ref = np.cov(used.T, bias=True).reshape(D, D)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    assert np.all(np.abs(c - ref) <= (1e-6 if f32 else 1e-10) * scale + (1e-6 if f32 else 0) * np.abs(np.outer(used.mean(0), used.mean(0))))
    np.testing.assert_allclose(mean, used.mean(axis=0), rtol=1e-6 if f32 else 1e-12, atol=1e-6 if f32 else 1e-13)


@pytest.mark.gpu
def test_device_covariance_accumulates_over_calls_and_resets():
    rng = np.random.default_rng(5)
    steps = rng.standard_normal((40, 256, 32)) * np.linspace(0.5, 2.0, 32)
    _, cov, corr = po.chain_covariance(steps, 1)
    m = capi.HipMoments(256, 32)
    for part in (steps[:7], steps[7:8], steps[8:29], steps[29:]):      # chain blocks arriving one by one
        m.add_steps(part)
    _, _, c, r = m.finish()
    _close(c, r, cov, corr, 1e-10)
    again = m.finish()                                                   # finish does not consume the sums
    np.testing.assert_array_equal(again[2], c)
    m.reset()
    m.add_steps(steps[:10])
    _, cov10, corr10 = po.chain_covariance(steps[:10], 1)
    _, _, c10, r10 = m.finish()
    _close(c10, r10, cov10, corr10, 1e-10)
    with pytest.raises(capi.HipError):
        capi.HipMoments(256, 32).finish()                                # nothing added


@pytest.mark.gpu
def test_device_resident_steps_give_the_same_sums():
    import torch
    rng = np.random.default_rng(9)
    steps = rng.standard_normal((6, 1024, 32)) + 0.5
    a, b = capi.HipMoments(1024, 32), capi.HipMoments(1024, 32)
    a.add_steps(steps)
    t = torch.from_numpy(steps).cuda()
    b.add_device_steps(t.data_ptr(), steps.shape[0])
    for x, y in zip(a.finish(), b.finish()):
        np.testing.assert_array_equal(x, y)                               # same kernel, same order: bit-identical


@pytest.mark.gpu
def test_covariance_facade_against_the_oracle():
    """include/MCMCpp/Analysis/CovarianceMatrix.h on a chain sampled through the facade (tests/cpp/covariance_facade.cpp)."""
    from tests.test_facade import BUILD, INC, LINK
    po.build()
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "covariance_facade")
    src = os.path.join(ROOT, "tests", "cpp", "covariance_facade.cpp")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(dp, f))
                                            for dp, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        capi.build_library()
        oracle_dir = os.path.join(ROOT, "oracle")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"] + INC + [src, "-o", exe] + LINK +
                              ["-L" + oracle_dir, "-loracle", "-Wl,-rpath," + oracle_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "covariance_facade OK" in out.stdout, out.stdout + out.stderr


# ---- the scaled error bar (tests/moments_reference.py) -------------------------------------------------------------

def _offset_steps(W, D, n, off, dt, spread_over_params=True):
    """n x W x D standard normals, default_rng(1), plus an offset: per parameter off * linspace(-1, 1, D), so that
    cross terms of mixed magnitude occur, or the same offset for all"""
    rng = np.random.default_rng(1)
    shift = off * np.linspace(-1.0, 1.0, D) if spread_over_params else off
    return (rng.standard_normal((n, W, D)) + shift).astype(dt)


def _mixed_steps(W, D, n, dt, seed):
    """correlated parameters with means of about 3 against a spread of about 1 (as test_device_covariance_matches_the_oracle)"""
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    return (rng.standard_normal((n, W, D)) @ mix + rng.standard_normal(D) * 3).astype(dt)


def _device(steps, sl=1):
    n, W, D = steps.shape
    m = capi.HipMoments(W, D, dtype=capi.F32 if steps.dtype == np.float32 else capi.F64)
    try:
        m.add_steps(steps, sl)
        return m.finish()
    finally:
        m.close()


def _bar_and_oracle(steps, sl, label):
    """the device against the bar, and against the oracle in the chain's own type at the existing tolerances"""
    ref = Reference(steps, sl)
    npts, mean, c, r = _device(steps, sl)
    assert npts == ref.count
    ref.check(mean, c, label)
    _close(c, r, ref.oracle[1], ref.oracle[2], 2e-4 if steps.dtype == np.float32 else 1e-10)
    return ref, mean, c, r


def test_the_header_names_the_chunk_knob():
    with open(os.path.join(ROOT, "include", "mcmcpp_hip.h")) as fh:
        header = fh.read()
    assert "MCMCPP_HIP_MOMENTS_CHUNK_MB" in header
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        assert "`MCMCPP_HIP_MOMENTS_CHUNK_MB`" in fh.read()


@pytest.mark.parametrize("off", [0.0, 1e3, 1e6])
def test_the_oracle_is_inside_the_bar_on_offset_data(off):
    """The inputs keep the reference inside the bar before the device is asked to: 40 x 64 x 5 standard normals plus
    an offset; the oracle's covariance within 4 * 2**-52 (|m_i m_j| + s_i s_j) of the np.longdouble two-pass result.
    Measured largest error / that bound: 0.13 at offset 0 (1.1e-16), 0.36 at 1e3 (3.2e-10), 0.26 at 1e6 (2.3e-4)."""
    steps = _offset_steps(64, 5, 40, off, np.float64, spread_over_params=False)
    mean, cov = exact_moments(steps, 1)
    sd = np.sqrt(np.diag(cov))
    omean, ocov, _ = po.chain_covariance(steps, 1)
    bound = MARGIN * U * (np.abs(np.outer(mean, mean)) + np.outer(sd, sd))
    print("oracle at offset %g: largest covariance error %.3g, error / bound %.3f; mean error / (4 u |m|) %.3f"
          % (off, np.abs(ocov - cov).max(), ratio(ocov, cov, bound), ratio(omean, mean, MARGIN * U * np.abs(mean))))
    assert np.all(np.abs(ocov - cov) <= bound)


def test_exact_moments_selects_the_sliced_steps_and_widens_floats():
    steps = _mixed_steps(3, 4, 7, np.float32, 2)
    mean, cov = exact_moments(steps, 3)
    used = steps[[0, 3, 6]].reshape(-1, 4).astype(np.float64)
    assert mean.dtype == np.float64 and cov.dtype == np.float64
    np.testing.assert_allclose(mean, used.mean(axis=0), rtol=1e-14)
    np.testing.assert_allclose(cov, np.cov(used.T, bias=True), rtol=1e-12, atol=1e-15)
    # a float result passes exactly where it is the rounding of an fp64 value within the bar
    exact, bar = np.array([1.0, 1.0, 1.0]), np.array([1e-12, 1e-12, 1e-12])
    got = np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))], np.float32)
    assert holds(got, exact, bar).tolist() == [True, False, False]
    assert holds(got.astype(np.float64), exact, bar).tolist() == [True, False, False]


OFFSET_CASES = [(W, D, n, off, dt) for (W, D, n) in ((64, 5, 40), (70, 33, 12))
                for dt, offs in ((np.float64, (0.0, 1e3, 1e6)), (np.float32, (0.0, 1e3))) for off in offs]


@pytest.mark.gpu
@pytest.mark.parametrize("W,D,n,off,dt", OFFSET_CASES)
def test_device_covariance_on_offset_data_meets_the_bar(W, D, n, off, dt):
    """Parameter i is centred at off * linspace(-1, 1, D)[i] with unit spread.  fp32 chains stop at 1e3: 1e6 + N(0, 1)
    leaves too few mantissa bits to be a useful input.
    Measured on the MI355X, largest error / bar (mean, covariance): fp64 64 x 5 x 40: (0.15, 0.13) at 0,
    (0.13, 0.25) at 1e3, (0.13, 0.25) at 1e6; 70 x 33 x 12: (0.25, 0.14), (0.21, 0.25), (0.21, 0.25); the oracle's own
    ratios are the same to two digits.  fp32: (0.97..0.99, 0.93..1.00): these count the half float spacing the
    narrowing may cost into the bar, so they sit just under 1 -- the result is the float nearest the exact value."""
    steps = _offset_steps(W, D, n, off, dt)
    ref = Reference(steps, 1)
    npts, mean, c, r = _device(steps, 1)
    assert npts == ref.count
    ref.check(mean, c, "offset %dx%dx%d %s off=%g" % (W, D, n, np.dtype(dt).name, off))
    assert np.all(holds(r, ref.corr, ref.corr_bar))


@pytest.mark.gpu
@pytest.mark.parametrize("off,dt", [(1e3, np.float64), (1e6, np.float64), (1e3, np.float32)])
def test_a_constant_parameter_does_not_disturb_the_others(off, dt):
    """64 x 5 x 40 as above; parameter 1 is exactly off + 2.5 in every sample, parameter 3 is off + 1e-6 off N(0, 1).
    The constant parameter's variance is within 4 * 2**-52 m**2 of zero (where it comes out negative its correlation
    row and column are NaN, where the oracle's zero variance gives infinities and NaN: non-finite either way, and in
    that row and column only).  Everything else meets the bars.
    Measured on the MI355X, largest error / bar (mean, covariance of the others; |var| / bound of the constant one):
    fp64 at 1e3 (0.13, 0.25; 0: the variance is exactly 0), at 1e6 (0.13, 0.11; 0); fp32 at 1e3 (0.93, 0.92 with the half
    float spacing counted into the bar; 0).  No defect found: finish needed no change."""
    W, D, n, const, near = 64, 5, 40, 1, 3
    steps = _offset_steps(W, D, n, off, np.float64)
    steps[:, :, const] = off + 2.5
    steps[:, :, near] = off + 1e-6 * off * np.random.default_rng(2).standard_normal((n, W))
    steps = steps.astype(dt)
    ref = Reference(steps, 1)
    assert ref.cov[const, const] == 0.0 and ref.mean[const] == off + 2.5
    others = np.arange(D) != const
    npts, mean, c, r = _device(steps, 1)
    ref.check(mean, c, "constant parameter %s off=%g" % (np.dtype(dt).name, off), where=others)
    assert holds(mean[const:const + 1], ref.mean[const:const + 1], ref.mean_bar[const:const + 1])[0]
    var_bound = MARGIN * U * ref.mean[const] ** 2
    print("constant parameter %s off=%g: variance %.3g, |var| / (4 u m^2) = %.3f; the oracle's %.3g"
          % (np.dtype(dt).name, off, c[const, const], abs(float(c[const, const])) / var_bound, ref.oracle[1][const, const]))
    assert abs(float(c[const, const])) <= var_bound
    # the covariances with the constant parameter are zero, to the bar
    assert np.all(holds(c[const, :], ref.cov[const, :], ref.cov_bar[const, :])) and np.all(c[:, const] == c[const, :])
    # correlation: untouched outside that parameter's row and column, which are all that is left out
    compared = np.outer(others, others)
    assert compared.size - np.count_nonzero(compared) == 2 * D - 1
    assert np.all(np.isfinite(r[compared]))
    assert np.all(holds(r[compared], ref.corr[compared], ref.corr_bar[compared]))
    # (the oracle, in fp64: a zero variance, and non-finite correlations in that row and column only)
    assert np.all(np.isfinite(ref.oracle64[2][compared]))
    if ref.oracle64[1][const, const] == 0.0:
        assert not np.any(np.isfinite(ref.oracle64[2][~compared]))


TILE_CASES = [(D, 1, dt) for dt in (np.float64, np.float32) for D in (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)] + \
             [(49, 3, np.float64), (49, 3, np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,sl,dt", TILE_CASES)
def test_every_tile_count_in_both_types(D, sl, dt):
    """One to four 16-parameter tiles of the matrix-core kernel and the first generic size, both sides of every
    boundary, fp64 and fp32.  37 walkers x 7 steps = 259 samples (111 at slice 3): no multiple of 4, and fewer than
    one group of four per wavefront.
    Measured on the MI355X, largest error / bar (mean, covariance) over the D of a type: fp64 (0.19..0.25,
    0.19..0.25); fp32 (0.88..1.00, 0.99..1.00 with the half float spacing of the narrowing counted into the bar)."""
    steps = _mixed_steps(37, D, 7, dt, 1000 + D)
    _bar_and_oracle(steps, sl, "tiles D=%d slice %d %s" % (D, sl, np.dtype(dt).name))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [20, 70])
@pytest.mark.parametrize("W,n", [(1, 1), (1, 2), (3, 1), (2, 2), (5, 1), (9, 7), (257, 1)])
def test_few_samples(W, n, D):
    """1, 2, 3, 4, 5, 63 and 257 samples: a single partial group of four, fewer samples than slots, fewer than four per
    slot; on the matrix cores (D = 20) and in the generic kernel (D = 70).  One sample: the mean is the sample and
    the covariance is zero, exactly.
    Measured on the MI355X, largest error / bar (mean, covariance) over the sample counts: (0.25, 0.27)."""
    steps = _mixed_steps(W, D, n, np.float64, 77 * W + n + D)
    npts, mean, c, r = _device(steps, 1)
    assert npts == W * n
    if W * n == 1:
        np.testing.assert_array_equal(mean, steps[0, 0])
        np.testing.assert_array_equal(c, np.zeros((D, D)))
        return
    Reference(steps, 1).check(mean, c, "few samples %dx%d D=%d" % (W, n, D))


@pytest.mark.gpu
@pytest.mark.parametrize("W,D,n,dt", [(40, 400, 3, np.float64), (40, 1024, 3, np.float64), (24, 1000, 5, np.float32)])
def test_wide_parameter_sets_on_the_generic_kernel(W, D, n, dt):
    """Beyond D of about 363 the 256 MiB cap halves the slot count; at D = 1024 the pair index runs to 524 799 and the
    LDS tile is 32 KB.
    Measured on the MI355X, largest error / bar (mean, covariance): (0.24, 0.25) at D = 400, (0.22, 0.26) at 1024,
    (1.00, 1.00) for fp32 at 1000 with the half float spacing of the narrowing counted into the bar."""
    steps = _mixed_steps(W, D, n, dt, D)
    _bar_and_oracle(steps, 1, "wide %dx%dx%d %s" % (W, D, n, np.dtype(dt).name))


@pytest.mark.gpu
def test_more_than_1024_parameters_are_refused():
    with pytest.raises(capi.HipError):
        capi.HipMoments(8, 1025)
    capi.HipMoments(8, 1024).close()


@pytest.mark.gpu
@pytest.mark.parametrize("D,stride", [(24, 1), (24, 3), (70, 2)])
def test_chunked_uploads(D, stride, monkeypatch):
    """MCMCPP_HIP_MOMENTS_CHUNK_MB=1 with 2000 walkers: D = 24 gives 384 000-byte steps, two per chunk, so 11 selected
    steps go up in five chunks and a short one; D = 70 (generic kernel) gives 1 120 000-byte steps, more than the
    chunk, so the minimum of one step per chunk holds.  The steps in between the selected ones lie 100 away.

    The kernels deal the samples of one launch to the wavefronts (groups of four round-robin; the generic kernel in
    equal shares), so the samples that meet in a slot, and with them the order of summation, depend on where the
    chunks are cut: the result of one contiguous upload (default chunk size, everything in one chunk) is not bit for
    bit that of the chunked one, and is held to the bar instead.  Bit for bit the chunked handle must equal a
    default-sized handle that is given the same chunks as separate contiguous calls: the same launches in the same
    order.  Both are compared with the oracle.
    Measured on the MI355X, largest error / bar (mean, covariance), chunked then contiguous: D = 24 stride 1 (0.21, 0.24)
    and the same; stride 3 (0.23, 0.25) and the same; D = 70 stride 2 (0.15, 0.25) then (0.20, 0.25).  In no case was
    the chunked covariance bit for bit the contiguous one."""
    W, n_sel = 2000, 11
    steps = _mixed_steps(W, D, (n_sel - 1) * stride + 1, np.float64, D + stride)
    for k in range(steps.shape[0]):
        if k % stride:
            steps[k] += 100.0
    selected = np.ascontiguousarray(steps[::stride])
    assert selected.shape[0] == n_sel
    per_chunk = max(1, (1 << 20) // (8 * W * D))
    assert per_chunk == (2 if D == 24 else 1) and n_sel % 2 == 1

    monkeypatch.setenv("MCMCPP_HIP_MOMENTS_CHUNK_MB", "1")             # read when the handle is created
    chunked = capi.HipMoments(W, D)
    monkeypatch.delenv("MCMCPP_HIP_MOMENTS_CHUNK_MB")
    whole, pieces = capi.HipMoments(W, D), capi.HipMoments(W, D)
    chunked.add_steps(steps, stride)
    whole.add_steps(selected)
    for first in range(0, n_sel, per_chunk):
        pieces.add_steps(selected[first:first + per_chunk])
    got, one, parts = chunked.finish(), whole.finish(), pieces.finish()
    for m in (chunked, whole, pieces):
        m.close()
    assert got[0] == one[0] == parts[0] == n_sel * W
    for x, y in zip(got[1:], parts[1:]):
        np.testing.assert_array_equal(x, y)
    ref = Reference(selected, 1)
    ref.check(got[1], got[2], "chunked D=%d stride %d" % (D, stride))
    ref.check(one[1], one[2], "contiguous D=%d stride %d" % (D, stride))
    _close(got[2], got[3], ref.oracle[1], ref.oracle[2], 1e-10)
    _close(one[2], one[3], ref.oracle[1], ref.oracle[2], 1e-10)
    print("chunked D=%d stride %d: bit for bit equal to the contiguous upload: %s" % (D, stride, np.array_equal(got[2], one[2])))


@pytest.mark.gpu
def test_the_upload_buffer_grows_between_calls_and_the_sums_are_kept():
    """The second call brings more steps than the first: the upload buffer is replaced while the slots keep the first
    call's sums.  Bit for bit the result equals that of a handle whose buffer had its final size before the first call.
    Measured on the MI355X, largest error / bar (mean, covariance): (0.23, 0.25)."""
    W, D = 300, 24
    steps = _mixed_steps(W, D, 7, np.float64, 11)
    growing, grown = capi.HipMoments(W, D), capi.HipMoments(W, D)
    grown.add_steps(steps[1:] + 50.0)
    grown.reset()
    for m in (growing, grown):
        m.add_steps(steps[:1])
        m.add_steps(steps[1:])
    a, b = growing.finish(), grown.finish()
    growing.close(), grown.close()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    ref = Reference(steps, 1)
    assert a[0] == ref.count
    ref.check(a[1], a[2], "growing upload buffer")
    _close(a[2], a[3], ref.oracle[1], ref.oracle[2], 1e-10)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("D,p,where", [(20, 17, (4, 33)), (20, 3, (0, 0)), (70, 41, (5, 63))])
def test_a_nan_sample_stays_in_its_parameter(D, p, where, dt):
    """64 walkers x 6 steps; one NaN, in parameter p of one sample.  On the matrix cores the NaN is multiplied by the
    zero padding too: that lands in the padded rows and columns of p's tiles, which nobody reads.  mean[p], cov[p, :]
    and cov[:, p] are NaN on the device as in the oracle; everything else is finite and within the bar of the exact
    moments of the same samples, whose other columns are untouched; corr has the oracle's NaN pattern.
    Measured on the MI355X, largest error / bar (mean, covariance) over the other parameters: fp64
    (0.20..0.22, 0.25); fp32 (0.98..0.99, 1.00 with the half float spacing of the narrowing counted into the bar)."""
    steps = _mixed_steps(64, D, 6, dt, 5 * D + p)
    steps[where[0], where[1], p] = np.nan
    others = np.arange(D) != p
    ref = Reference(steps, 1, keep=others)
    npts, mean, c, r = _device(steps, 1)
    assert npts == ref.count
    hit = ~np.outer(others, others)
    for name, got_mean, got_cov in (("device", mean, c), ("oracle", ref.oracle[0], ref.oracle[1])):
        assert np.isnan(got_mean[p]) and np.all(np.isnan(got_cov[hit])), name
        assert np.all(np.isfinite(got_mean[others])) and np.all(np.isfinite(got_cov[~hit])), name
    ref.check(mean, c, "NaN sample D=%d p=%d %s" % (D, p, np.dtype(dt).name))
    np.testing.assert_array_equal(np.isnan(r), np.isnan(ref.oracle[2]))
    np.testing.assert_array_equal(np.isnan(r), hit)
    tol = 2e-4 if dt == np.float32 else 1e-10
    assert np.all(np.abs(r[~hit].astype(np.float64) - ref.oracle[2][~hit]) <= tol)
