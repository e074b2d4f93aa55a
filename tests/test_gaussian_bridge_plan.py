"""mcmcpp_amd/csrc/gaussian_bridge_plan.hpp: the host's decisions of mcmcpp_hip_evidence_gaussian and the arithmetic of a
proposal's row and of log q, on the CPU.  tests/cpp/gaussian_bridge_plan_cases.cpp compiles the header with the host compiler
alone (-ffp-contract=off) and prints what it plans and computes; the rows, log q, k and p must equal the numpy restatement
(tests/gaussian_bridge_restatement.py) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import de_stream_restatement as ds
from tests import gaussian_bridge_restatement as gb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
OK, TOO_WIDE, MEAN, FACTOR, DIAGONAL = range(5)


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "gaussian_bridge_plan_cases")
    # the host compiler alone, and no include path but the headers' own directory: the plan must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "gaussian_bridge_plan_cases.cpp"), "-I", CSRC])
    return exe


def _run(exe, what, **args):
    return subprocess.run([exe, what] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]


def _bits(x):
    return "%016x" % int(np.array([x], np.float64).view(np.uint64)[0])


def _gaussian(D, seed=0):
    """a mean and a full lower factor with a positive diagonal (what lies above it must not be read: NaN)"""
    rng = np.random.default_rng(100 + D + seed)
    L = np.tril(rng.standard_normal((D, D))) * 0.3
    L[np.diag_indices(D)] = 0.5 + rng.random(D)
    chol = L.copy()
    chol[np.triu_indices(D, 1)] = np.nan
    return rng.standard_normal(D) * 2.0, L, chol


def test_limits(driver):
    assert _run(driver, "limits") == ["max_d=64 stage_bytes=%d diff_threads=256 half_log_2pi=%s" % (34 * 1024, _bits(0.91893853320467274178))]
    # (numpy's logarithm of the rounded 2 pi is within an ulp of the constant's double: ulp(0.9) = 1.1e-16)
    assert abs(gb.HALF_LOG_2PI - 0.5 * np.log(2.0 * np.pi)) <= 2.0 ** -52 and gb.MAX_D == 64


@pytest.mark.parametrize("D, rows", [(1, 256), (2, 256), (3, 256), (16, 256), (17, 128), (33, 128), (34, 64), (64, 64)])
def test_launch_shapes_and_buffer_sizes(driver, D, rows):
    """a thread owns a row; the block's rows are staged as columns [D][rows + 1] of doubles behind the D + D (D + 1) / 2 parameters"""
    for N in (1, rows, rows + 1, 4194304):
        head = {k: int(v) for k, v in (kv.split("=") for kv in _run(driver, "shape", D=D, N=N)[0].split())}
        params = D + D * (D + 1) // 2
        assert head == dict(rows=rows, lds=8 * (params + (rows + 1) * D), blocks=-(-N // rows), fits=1, entries=max(1, (N - 1).bit_length()), params=params,
                            diff_blocks=-(-N // 256))
        assert head["lds"] <= 64 * 1024 and (rows + 1) * D * 8 <= 34 * 1024  # what a launch may ask for without an attribute
    assert _run(driver, "shape", D=D, N=(2 ** 31 - 1) * rows + 1)[0].split()[3] == "fits=0"


def test_the_stream_position_is_64_bits_wide(driver):
    for j, D, d in [(0, 1, 0), (5, 3, 2), (2 ** 31, 2, 1), (2 ** 32 + 7, 64, 63), (2 ** 40, 17, 5), ((2 ** 57) - 1, 64, 63)]:
        assert _run(driver, "position", j=j, D=D, d=d) == [str(j * D + d)]
    assert (2 ** 32 + 7) * 64 + 63 > 2 ** 32


def test_the_restatements_jump_equals_stepping():
    """state_at, by which the restatement reaches a far position, against stepping one draw at a time"""
    st = ds.Stream(11, 3)
    want = st.raws(1000, 8)
    assert (gb.raws(11, 3, 1000, 8) == want).all() and (gb.raws(11, 3, 0, 3) == st.raws(0, 3)).all()
    a = gb.raws(5, 0, 2 ** 40 + 3, 4)
    b = gb.raws(5, 0, 2 ** 40, 7)[3:]
    assert (a == b).all()


def test_p_is_exact_at_both_ends(driver):
    for r in (0, 1, 4095, 4096, 2 ** 63, 2 ** 64 - 4097, 2 ** 64 - 1):
        p = gb.p_of(np.array([r], np.uint64))[0]
        assert _run(driver, "p", r=r) == ["%s %s" % (_bits(p), _bits(1.0 - p))]
        k = r >> 12
        assert p == (2 * k + 1) / 2.0 ** 53 and 1.0 - p == (2 ** 53 - 2 * k - 1) / 2.0 ** 53 and 0.0 < p < 1.0
    assert gb.p_of(np.array([0], np.uint64))[0] == 2.0 ** -53 and gb.p_of(np.array([2 ** 64 - 1], np.uint64))[0] == 1.0 - 2.0 ** -53


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 2, 3, 17, 64])
def test_rows_log_q_and_k_equal_the_restatement(driver, tmp_path, D, dtype):
    N = 40
    mean, L, chol = _gaussian(D)
    raw = gb.raws(7, 2, 0, N * D)
    raw[:4] = [0, 2 ** 64 - 1, 2 ** 63, 12345]  # both ends of p and the middle
    path = tmp_path / "g.bin"
    with open(str(path), "wb") as f:
        f.write(mean.tobytes() + chol.tobytes() + raw.tobytes())
    lines = _run(driver, "rows", file=path, D=D, N=N, f32=int(dtype == np.float32))
    x = gb.rows_from_raws(mean, L, raw.reshape(N, D), dtype)
    lq = gb.log_q(x, mean, L)
    assert lines[0] == _bits(gb.log_norm(L))
    word = np.uint64 if dtype == np.float64 else np.uint32
    fmt = "%016x" if dtype == np.float64 else "%08x"
    for j in range(N):
        assert lines[1 + j].split() == [fmt % int(v) for v in x[j].view(word)] + [_bits(lq[j])], j
    assert np.isfinite(x).all() and np.isfinite(lq).all()
    # the restatement itself: k and log q against the textbook formula
    y = np.linalg.solve(L, (x.astype(np.float64) - mean).T).T
    want = -0.5 * (y ** 2).sum(axis=1) - np.log(np.diag(L)).sum() - 0.5 * D * np.log(2.0 * np.pi)
    assert np.allclose(lq, want, rtol=1e-12, atol=1e-9)


def test_d_65_and_bad_factors_are_refused(driver, tmp_path):
    def check(D, mean, chol):
        path = tmp_path / "c.bin"
        with open(str(path), "wb") as f:
            f.write(np.asarray(mean, np.float64).tobytes() + np.asarray(chol, np.float64).tobytes())
        return [int(v) for v in _run(driver, "check", file=path, D=D)[0].split()]

    mean, L, chol = _gaussian(5)
    assert check(5, mean, chol) == [OK, 0, 0] and gb.refused(mean, chol) is None
    assert check(65, np.zeros(65), np.eye(65))[0] == TOO_WIDE and gb.refused(np.zeros(65), np.eye(65))[0] == "E_UNSUPPORTED"
    assert check(64, np.zeros(64), np.eye(64)) == [OK, 0, 0]
    for bad in (np.nan, np.inf, -np.inf):
        m = mean.copy()
        m[3] = bad
        assert check(5, m, chol) == [MEAN, 3, 0] and gb.refused(m, chol) == ("E_ARG", "mean")
        c = chol.copy()
        c[4, 1] = bad
        assert check(5, mean, c) == [FACTOR, 4, 1] and gb.refused(mean, c) == ("E_ARG", "factor")
    for bad in (0.0, -0.0, -1.0, 2.0 ** -1030):  # zero, negative, subnormal
        c = chol.copy()
        c[2, 2] = bad
        assert check(5, mean, c) == [DIAGONAL, 2, 2] and gb.refused(mean, c) == ("E_ARG", "diagonal")
    c = chol.copy()
    c[2, 2] = np.finfo(np.float64).tiny  # the smallest positive normal number passes
    assert check(5, mean, c) == [OK, 0, 0] and gb.refused(mean, c) is None
