"""The logarithms of the accept test, and the near-tie band that rests on them.

Device and oracle decide `ln U < (D-1) ln z + logp_new - logp_old` with different logarithm functions: mcmcpp::fast_log
against glibc's log in fp64, OCML's logf against glibc's logf in fp32.  Their chains are called identical because both sides
flag a decision whose margin is within tie_eps * scale as a near tie; that is sound only if the two logarithms never differ
by more than the band covers.  This file measures how far they differ and checks the band against it.

  1. CPU   tests/cpp/fast_log_cases.cpp: fast_log against logq (libquadmath) on 15.4 M arguments: faithful (< 1 ulp).
  2. GPU   tests/cpp/accept_log_device.hip: the device builds of dev_log, canonical and draw_store<T>: fast_log returns the
           host build's bits; OCML logf against glibc logf on every float in [2^-24, 4] (d32); the draw records on raw
           outputs chosen for the edges, against a NumPy restatement with individually rounded operations.
  3. both  (d + 3) * eps <= tie_eps with the measured d, tie_eps read from the library; one definition of tie_eps.
  4. GPU   a long fp32 run leaves the oracle's chain only at a decision the oracle flagged.

What the accuracy test can and cannot see (measured by editing Lg3 = 2.857142874366239149e-01 in a scratch copy of
fast_log.hpp and running `fast_log_cases check`):
    Lg3 + 1e-9  (10th digit)  worst error 8.73 ulp, 9 ulp from glibc   fails
    Lg3 + 1e-11 (11th digit)  worst error 1.62 ulp, 2 ulp from glibc   fails
    Lg3 + 1e-12 (12th digit)  worst error 0.92 ulp                      passes: the result is still faithful
    last printed digit 9 -> 8 the same double (a double carries 17 digits; the literal prints 19): the same object code
The last case no test of values can see, so test_fast_log_literals_are_the_doubles_they_denote asks that every digit in the
header is a digit of the double the compiler reads: it fails on that edit."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

from mcmcpp_amd import capi, workloads
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EPS = {po.F64: 2.0 ** -52, po.F32: 2.0 ** -23}
# Roundings that can separate the two sides' `ln_u - delta` beyond the d ulp of the logarithms; see test_band_covers_*
BAND_ROUNDINGS = 3


# ---------------------------------------------------------------------------------------------------------------- builds

@pytest.fixture(scope="module")
def cases_exe():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "fast_log_cases")
    # the host compiler alone, and no include path but the headers' own directory: fast_log.hpp and canonical.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "fast_log_cases.cpp"), "-I", CSRC, "-lquadmath"])
    return exe


@pytest.fixture(scope="module")
def cases(cases_exe):
    """{family: {field: value}} of `fast_log_cases check`, and the bits of fast_log(1.0)."""
    out = subprocess.run([cases_exe, "check"], capture_output=True, text=True, check=True).stdout
    print("\n" + out)
    fams, one_bits = {}, None
    for line in out.splitlines():
        if line.startswith("family="):
            f = dict(kv.split("=") for kv in line.split())
            fams[f.pop("family")] = f
        elif line.startswith("fast_log_of_one_bits="):
            one_bits = int(line.split("=")[1], 16)
    return fams, one_bits


@pytest.fixture(scope="module")
def dev():
    """tests/cpp/accept_log_device.hip with the flags of mcmcpp_amd/csrc/Makefile."""
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "accept_log_device.hip")
    out = os.path.join(BUILD, "libaccept_log_device.so")
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc", ".h")))
    if not os.path.exists(out) or os.path.getmtime(out) < max(newest, os.path.getmtime(src)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                               "-fPIC", "-shared", "-mllvm", "-amdgpu-kernarg-preload-count=16", "-Wall", "-Wno-unused-function",
                               "-Wno-unused-value", "-I" + CSRC, src, "-o", out])
    L = C.CDLL(out)
    L.ald_tie_eps.restype = C.c_double
    L.ald_tie_eps.argtypes = [C.c_int, C.c_int]
    L.ald_stretch_constants.restype = None
    L.ald_stretch_constants.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_double)] * 3
    L.ald_compare_logf_range.restype = None
    L.ald_compare_logf_range.argtypes = [C.c_uint32, C.c_uint, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    for t in ("f64", "f32"):
        getattr(L, "ald_log_" + t).argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        getattr(L, "ald_canonical_" + t).argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        getattr(L, "ald_draw_" + t).argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_uint] + [C.c_void_p] * 3
        getattr(L, "ald_host_log_" + t).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        getattr(L, "ald_host_log_" + t).restype = None
    L.ald_log_f32_range.argtypes = [C.c_uint32, C.c_uint, C.c_void_p]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _t(dtype):
    return "f64" if dtype == po.F64 else "f32"


CHUNK = 1 << 22  # elements per device call: no buffer above 32 MB


def _dev_log(dev, x):
    x = np.ascontiguousarray(x)
    y = np.empty_like(x)
    f = dev.ald_log_f64 if x.dtype == np.float64 else dev.ald_log_f32
    for i in range(0, x.size, CHUNK):
        assert f(_p(x[i:i + CHUNK]), _p(y[i:i + CHUNK]), x[i:i + CHUNK].size) == 0
    return y


def _host_log(dev, x):
    """glibc's log / logf, the oracle's logarithms (NumPy's own are a different implementation)."""
    x = np.ascontiguousarray(x)
    y = np.empty_like(x)
    (dev.ald_host_log_f64 if x.dtype == np.float64 else dev.ald_host_log_f32)(_p(x), _p(y), x.size)
    return y


def _ulp_distance(a, b):
    """Distance of two float arrays in units in the last place: their difference as integers in numerical order."""
    it = np.int64 if a.dtype == np.float64 else np.int32
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    lowest = np.int64(np.iinfo(it).min)
    ia = np.where(ia < 0, lowest - ia, ia)
    ib = np.where(ib < 0, lowest - ib, ib)
    return np.abs(ia - ib)


# ------------------------------------------------------------------------------------------- 1. fast_log on the CPU

def test_log_headers_need_no_hip_header(cases_exe):
    """(cases_exe: g++ compiled the case program against the two headers with no HIP include path)"""
    for name, want in (("fast_log.hpp", ["<stdint.h>", "<string.h>"]), ("canonical.hpp", ["<stdint.h>"])):
        text = open(os.path.join(CSRC, name)).read()
        assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == want, name


def test_fast_log_is_faithful(cases):
    """|fast_log(x) - log x| < 1 ulp of the exact value on every input of every family (judge: logq of libquadmath on the
    exact double), fast_log(1.0) == +0.0, and the sign of the result is the sign of x - 1.
    Measured (`tests/cpp/_build/fast_log_cases check`, 15 425 397 arguments): worst 0.8546 ulp at 0x1.6a09e667f18e7p-1 (just
    below sqrt(1/2)); glibc's log 0.5189; fast_log != glibc log on 6.3 % of all arguments and 6.9 % of the sampler's, never
    by more than 1 ulp."""
    fams, one_bits = cases
    want = {"sampler_a2_z", "sampler_a2_1mu", "sampler_a32_z", "sampler_a32_1mu", "below_one", "above_one", "sqrt2", "sqrt_half", "binades",
            "edges", "total"}
    assert set(fams) == want
    assert int(fams["sampler_a2_z"]["n"]) >= 2000000 and int(fams["sampler_a32_z"]["n"]) >= 2000000
    assert int(fams["below_one"]["n"]) == int(fams["above_one"]["n"]) == 1000000
    assert int(fams["sqrt2"]["n"]) >= 400000 and int(fams["sqrt_half"]["n"]) >= 400000
    assert int(fams["total"]["n"]) == sum(int(f["n"]) for k, f in fams.items() if k != "total")
    for name, f in fams.items():
        print("%-16s n=%-9s worst %.4f ulp at %s; glibc %.4f; fast_log != glibc log on %.2f %% (at most %s ulp apart)"
              % (name, f["n"], float(f["worst_ulp"]), f["worst_arg"], float(f["glibc_worst_ulp"]), 100.0 * int(f["differ"]) / int(f["n"]),
                 f["max_dist"]))
        assert float(f["worst_ulp"]) < 1.0, (name, f)       # (a NaN fails this too)
        assert int(f["sign_bad"]) == 0, (name, f)
    assert one_bits == 0


def test_fast_log_literals_are_the_doubles_they_denote():
    """Every decimal constant of fast_log.hpp, printed with as many digits as the header shows, is the header's text again:
    no digit in the source is noise that could be wrong without changing a bit of object code (see the module docstring)."""
    text = open(os.path.join(CSRC, "fast_log.hpp")).read()
    lits = re.findall(r"\b(\w+) = (\d\.\d+e[-+]\d+)", text)
    assert [n for n, _ in lits] == ["ln2_hi", "ln2_lo", "Lg1", "Lg2", "Lg3", "Lg4", "Lg5", "Lg6", "Lg7"]
    for name, lit in lits:
        digits = len(lit.split("e")[0]) - 2
        assert "%.*e" % (digits, float(lit)) == lit, name


# ------------------------------------------------------------------------------------------- 3. the band (CPU part)

def _tie_eps_literals():
    """Numeric values given to a tie_eps anywhere in the library's or the oracle's sources, outside tie_eps.h."""
    found = []
    for d in (CSRC, os.path.join(ROOT, "oracle")):
        for f in sorted(os.listdir(d)):
            if f.endswith((".hpp", ".hip", ".h", ".c", ".inc", ".cpp")) and f != "tie_eps.h":
                for line in open(os.path.join(d, f)):
                    if re.search(r"tie_eps\s*=|define\s+TIE_EPS", line, re.I) and re.search(r"\d+e-\d+", line):
                        found.append((f, line.strip()))
    return found


def test_tie_eps_is_one_pair_of_numbers(dev):
    """The stretch sampler's (stretch_args<T>, which the batch sampler shares), the DE sampler's and the oracle's bands are
    the same two numbers, and no source gives a tie_eps a number of its own."""
    for dtype, want in ((po.F64, 1e-12), (po.F32, float(np.float32(6e-7)))):
        got = dev.ald_tie_eps(dtype, 0), dev.ald_tie_eps(dtype, 1), po.tie_eps(dtype)
        assert got == (want, want, want), (dtype, got)
    assert _tie_eps_literals() == []
    assert "args.tie_eps = accept_tie_eps<T>();" in open(os.path.join(CSRC, "diffevo.hip")).read()


def _band_condition(d, dtype, tie_eps):
    """The soundness condition of the near-tie band (see test_band_covers_fp64_distance); returns (left side, slack)."""
    eps = EPS[dtype]
    lhs = (d + BAND_ROUNDINGS) * eps * (1 + 16 * eps)
    return lhs, tie_eps / lhs


def test_band_covers_fp64_distance(cases, dev):
    """The condition under which a decision can differ between device and oracle only where both flag a near tie.

    Both sides compute, from identical u, z, lp_new, lp_old (stretch_accept in stretch_kernel.hpp, which the full-step and
    batch accept kernels call and the two half-step kernels spell out; oracle update_walker):
        ln_u  = L(1 - u)                        the two L differ by at most d ulp:  |diff| <= d eps |ln_u|
        zs    = fl(L(z) * (D-1))                d eps |zs| carried through the product, + 1/2 ulp of each side's rounding:
                                                |diff| <= (d + 1) eps |zs|
        s     = fl(zs + lp_new)                 + 1/2 ulp(s) each side:  (d + 1) eps |zs| + eps (|zs| + |lp_new|)
        delta = fl(s - lp_old)                  + 1/2 ulp(delta) each side:  ... + eps (|zs| + |lp_new| + |lp_old|)
    `ln_u < delta` itself is exact.  So `ln_u - delta` differs between the sides by at most
        d eps |ln_u| + (d + 3) eps |zs| + 2 eps |lp_new| + eps |lp_old|  <=  (d + 3) eps scale,
    scale = |ln_u| + |zs| + |lp_new| + |lp_old| as the kernels and the oracle form it.  If the decisions differ, the two
    margins have opposite signs and their magnitudes add up to at most that, so each is below it and is flagged when
        (d + 3) eps <= tie_eps.
    My count of roundings is 3, the issue's: one for zs, one for each of the two sums.  The flag's own arithmetic (margin,
    scale: three sums, tie_eps * scale, each rounded; the two sides' scales differ by O(eps) of themselves) moves both sides
    of `margin <= tie_eps * scale` by a few eps RELATIVE: the factor (1 + 16 eps) on the left pays for it.  Differential
    evolution (de_accept in stretch_kernel.hpp) has no zs term and delta = fl(lp_new - lp_old) is the same on both
    sides: d eps scale, covered by the same condition.

    fp64: d = 1, measured: the case program's largest distance between fast_log and glibc's log, over arguments on which
    fast_log is faithful (test_fast_log_is_faithful) and glibc within 0.52 ulp."""
    fams, _ = cases
    d = int(fams["total"]["max_dist"])
    assert d <= 1
    assert float(fams["total"]["glibc_worst_ulp"]) < 1.0
    tie_eps = dev.ald_tie_eps(po.F64, 0)
    lhs, slack = _band_condition(d, po.F64, tie_eps)
    print("\nfp64: d = %d ulp: (d + %d) eps = %.3e <= tie_eps = %.3e (a factor %.0f to spare)" % (d, BAND_ROUNDINGS, lhs, tie_eps, slack))
    assert lhs <= tie_eps


# -------------------------------------------------------------------------------------------------- 2. on the device

@pytest.mark.gpu
def test_device_fast_log_returns_the_host_builds_bits(cases_exe, dev, tmp_path):
    """dev_log(double) under hipcc for gfx950 (device division and fma) on every argument of part 1: the bits of the host
    build, whose accuracy test_fast_log_is_faithful states; so that statement holds on the device."""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.check_call([cases_exe, "dump", fin, fout])
    x, want = np.fromfile(fin, dtype=np.float64), np.fromfile(fout, dtype=np.float64)
    assert x.size == want.size > 13000000
    got = _dev_log(dev, x)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    print("\ndevice fast_log: %d arguments, %d differ from the host build" % (x.size, bad.size))
    assert bad.size == 0, [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]


@pytest.fixture(scope="module")
def d32(dev):
    """OCML logf (dev_log(float)) against glibc logf on every float in [2^-24, 4]: (d32, arguments that differ, arguments)."""
    t0 = time.time()
    first, last = np.float32(2.0 ** -24).view(np.uint32), np.float32(4.0).view(np.uint32)
    total = differ = 0
    dist, worst = 0, 0
    y = np.empty((1 << 23) + 1, dtype=np.float32)
    b = int(first)
    while b <= int(last):
        n = min(1 << 23, int(last) - b + 1)
        if b + n == int(last):
            n += 1  # 4.0 itself rides with the last binade
        assert dev.ald_log_f32_range(b, n, _p(y)) == 0
        nd, md, wb = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        dev.ald_compare_logf_range(b, n, _p(y), C.byref(nd), C.byref(md), C.byref(wb))
        total += n
        differ += nd.value
        if md.value > dist:
            dist, worst = md.value, wb.value
        b += n
    assert total == 218103809
    print("\nOCML logf against glibc logf on all %d floats in [2^-24, 4]: %d differ (%.4f %%), d32 = %d ulp (first at %s); %.1f s"
          % (total, differ, 100.0 * differ / total, dist, float(np.uint32(worst).view(np.float32)).hex(), time.time() - t0))
    return dist, differ, total


@pytest.mark.gpu
def test_device_logf_against_glibc_logf_on_every_argument(d32):
    """d32 is measured, not assumed.  glibc 2.35 logf is within 0.8177 ulp of the exact value over this range, so d32 = 1
    would say OCML's is faithful here as well; what the band has to cover is whatever comes out
    (test_band_covers_fp32_distance).  Only sanity is asserted here: a number came back for every argument.
    Measured on an MI355X (ROCm's OCML against glibc 2.35): 107 123 330 of 218 103 809 arguments differ (49.12 %), d32 = 2 ulp;
    26 launches of one binade each and the host comparison take 0.7 s."""
    dist, differ, total = d32
    assert total == 218103809 and dist < 2 ** 31 - 1  # (the latter: no NaN)


@pytest.mark.gpu
def test_band_covers_fp32_distance(d32, dev):
    """(d32 + 3) * 2^-23 <= tie_eps, tie_eps as the library sets it: derivation in test_band_covers_fp64_distance.
    Measured: d32 = 2, 5.9605e-7 <= 6.0000e-7: it holds with 0.66 % to spare (the output says "holds, barely")."""
    dist, differ, total = d32
    tie_eps = dev.ald_tie_eps(po.F32, 0)
    lhs, slack = _band_condition(dist, po.F32, tie_eps)
    print("\nfp32: d32 = %d ulp: (d32 + %d) eps = %.4e <= tie_eps = %.4e: %s (tie_eps / left side = %.4f)"
          % (dist, BAND_ROUNDINGS, lhs, tie_eps, "holds, barely" if 1 <= slack < 1.05 else ("holds" if slack >= 1 else "FAILS"), slack))
    assert lhs <= tie_eps


# ---- the draw records

def _bit_length(r):
    x = r.copy()
    n = np.zeros(r.shape, dtype=np.int64)
    for b in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(b)) != 0
        n += b * m
        x = np.where(m, x >> np.uint64(b), x)
    return n + (x != 0)


def _u64_to_float(r, t):
    """(T)r rounded to nearest, ties to even, in integer arithmetic."""
    p = 53 if t == np.float64 else 24
    shift = np.maximum(_bit_length(r) - p, 0).astype(np.uint64)
    q = r >> shift
    rem = r & ((np.uint64(1) << shift) - np.uint64(1))
    one = np.uint64(1)
    half = np.where(shift > 0, one << (np.maximum(shift, one) - one), np.uint64(0))
    up = (shift > 0) & ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1)))
    q = q + up.astype(np.uint64)
    return np.ldexp(q.astype(t), shift.astype(np.int32)).astype(t)  # (q <= 2^p: exact)


def _canonical(r, t):
    u = _u64_to_float(r, t) * t(2.0 ** -64)  # (a power of two: exact)
    return np.where(u >= t(1), np.nextafter(t(1), t(0)), u).astype(t), u >= t(1)


def _edge_raws():
    M = (1 << 64) - 1
    v = {0, 1, 2, M, M - 1}
    for k in range(64):
        v.update(((1 << k) + d) & M for d in (-2, -1, 0, 1, 2))
    for p in (24, 53):
        # where the conversion rounds up to 2^64: the top binade's last midpoint and the representable values around it
        ulp = 1 << (64 - p)
        for centre in ((1 << 64) - ulp // 2, (1 << 64) - ulp, (1 << 64) - ulp - ulp // 2, (1 << 64) - 2 * ulp):
            v.update(centre + d for d in (-2, -1, 0, 1, 2))
        # ties of the conversion in every binade that rounds: odd and even kept parts, the midpoint and its neighbours
        rng = np.random.default_rng(p)
        for e in range(p + 1, 65):
            sh = e - p
            for q in list(rng.integers(1 << (p - 1), 1 << p, size=24)) + [1 << (p - 1), (1 << p) - 1, (1 << p) - 2]:
                v.update((int(q) << sh) + (1 << (sh - 1)) + d for d in (-1, 0, 1))
    return np.array(sorted(x for x in v if 0 <= x <= M), dtype=np.uint64)


@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
def test_canonical_restatement_is_the_oracles(dtype):
    """CPU: the NumPy restatement the device records are compared with agrees with the oracle's C canonical on the edge set."""
    t = po.np_dtype(dtype)
    r = np.concatenate([_edge_raws(), np.random.default_rng(6).integers(0, 1 << 64, size=20000, dtype=np.uint64, endpoint=False)])
    f = po.lib().so_canonical_f64 if dtype == po.F64 else po.lib().so_canonical_f32
    want = np.array([f(int(x)) for x in r], dtype=t)
    u, clamped = _canonical(r, t)
    np.testing.assert_array_equal(u, want)
    assert clamped.sum() >= 5 and (u < 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [(2, 1), (3, 2)], ids=["alpha2", "alpha3_2"])
@pytest.mark.parametrize("dtype", [po.F64, po.F32], ids=["f64", "f32"])
def test_draw_records_on_edge_raw_outputs(dev, cases, d32, dtype, alpha):
    """draw_store<T> (k = 1: z, zs; k = 2: ln_u) and canonical on raw outputs 0, 1, 2^64 - 1, either side of every point
    where the conversion rounds up to 2^64 (the clamp), ties of the conversion, powers of two and their neighbours, and two
    million seeded values, against a NumPy restatement with individually rounded operations."""
    t = po.np_dtype(dtype)
    D = 32
    r = np.concatenate([_edge_raws(), np.random.default_rng(5).integers(0, 1 << 64, size=2000000, dtype=np.uint64, endpoint=False)])
    n = r.size
    dist = int(cases[0]["total"]["max_dist"]) if dtype == po.F64 else d32[0]

    # the constants: stretch_args<T> against T arithmetic here
    g1, g0, dm1 = C.c_double(0), C.c_double(0), C.c_double(0)
    dev.ald_stretch_constants(dtype, alpha[0], alpha[1], D, C.byref(g1), C.byref(g0), C.byref(dm1))
    sqrt_a = np.sqrt(t(alpha[0]) / t(alpha[1]))
    t0 = t(1) / sqrt_a
    t1 = sqrt_a - t0
    assert (g1.value, g0.value, dm1.value) == (float(t1), float(t0), float(D - 1))

    u, clamped = _canonical(r, t)
    got_u = np.empty(n, dtype=t)
    assert getattr(dev, "ald_canonical_" + _t(dtype))(_p(r), _p(got_u), n) == 0
    np.testing.assert_array_equal(got_u.view(np.uint64 if t == np.float64 else np.uint32), u.view(np.uint64 if t == np.float64 else np.uint32))
    assert clamped.sum() >= 5 and clamped[r == np.uint64((1 << 64) - 1)].all()   # the clamp was met
    assert (got_u < 1).all() and (got_u >= 0).all()

    rec = {}
    for k in (1, 2):
        z, zs, ln_u = (np.empty(n, dtype=t) for _ in range(3))
        assert getattr(dev, "ald_draw_" + _t(dtype))(alpha[0], alpha[1], D, k, _p(r), n, _p(z), _p(zs), _p(ln_u)) == 0
        rec[k] = z, zs, ln_u

    # k = 1
    tmp = (t1 * u).astype(t) + t0
    z = (tmp * tmp).astype(t)
    got_z, got_zs, _ = rec[1]
    np.testing.assert_array_equal(got_z, z)
    lz_host, lz_dev = _host_log(dev, z), _dev_log(dev, z)
    same = lz_host == lz_dev
    np.testing.assert_array_equal(got_zs, (lz_dev * t(D - 1)).astype(t))                 # the record is dev_log's product
    np.testing.assert_array_equal(got_zs[same], (lz_host * t(D - 1)).astype(t)[same])    # and the oracle's where the logs agree
    assert _ulp_distance(lz_host, lz_dev).max() <= dist

    # k = 2
    arg = (t(1) - u).astype(t)
    assert (arg > 0).all()                                   # the logarithm's argument is never 0
    _, _, got_ln_u = rec[2]
    assert np.isfinite(got_ln_u).all() and (got_ln_u <= 0).all()
    lu_host, lu_dev = _host_log(dev, arg), _dev_log(dev, arg)
    np.testing.assert_array_equal(got_ln_u, lu_dev)
    same_u = lu_host == lu_dev
    np.testing.assert_array_equal(got_ln_u[same_u], lu_host[same_u])
    assert _ulp_distance(lu_host, lu_dev).max() <= dist
    print("\n%s alpha %d/%d: %d raw outputs, %d clamped; the logs differ on %d of ln z and %d of ln(1-u), by at most %d ulp"
          % (_t(dtype), alpha[0], alpha[1], n, int(clamped.sum()), int((~same).sum()), int((~same_u).sum()), dist))


# --------------------------------------------------------------------------------------------- 4. the long fp32 run

LONG_W, LONG_D, LONG_CHUNK = 16384, 32, 25
LONG_STEPS = 6500


@pytest.mark.gpu
def test_long_fp32_run_leaves_the_oracle_only_at_a_flagged_decision():
    """16 384 x 32 dense Gaussian (rho = 0.5) in fp32, seed 0, LONG_STEPS ensemble steps against the oracle in chunks of 25 with
    every step stored.  Either every chunk is bit-identical and the tie counts agree, or the first decision on which device
    and oracle part is one the oracle flagged as a near tie (and the device flagged one in that chunk too): the documented
    kind.  A divergence at a decision the oracle did not flag fails.

    LONG_STEPS: the oracle alone does 108 ensemble steps per second of this configuration with 16 threads on an 8-core
    host (1000 steps in 9.2 s), 6500 in one minute.

    Measured on an MI355X: identical for 608 ensemble steps (1.0e7 updates); in step 608 walker 11462 (black) parts at a
    decision the oracle flagged (ln_u = delta = -1.67710876 as floats); the device flagged 4 near ties in that chunk."""
    W, D, n = LONG_W, LONG_D, LONG_W // 2
    P = workloads.ar1_precision(D, 0.5, np.float32)
    orc = po.Oracle(W, D, po.CALC_DENSE_GAUSSIAN, P.ravel(), seed=0, dtype=po.F32)
    pos = po.init_positions(po.F32, W, D, salt=0)
    logp = orc.logp(pos)
    orc.set_state(pos, logp)
    hip = capi.HipSampler(W, D, capi.CALC_DENSE_GAUSSIAN, P.ravel(), seed=0, dtype=po.F32)
    np.testing.assert_array_equal(hip.calc_logp(pos), logp)
    hip.set_state(pos, logp)
    t0 = time.time()
    for c in range(LONG_STEPS // LONG_CHUNK):
        before = orc.get_state()
        dev_ties_before = hip.counters()["near_ties"]
        oc, oa = orc.run(LONG_CHUNK, mode=po.MODE_COUNTER, threads=16)
        hc, ha = hip.run(LONG_CHUNK)
        if np.array_equal(hc, oc) and np.array_equal(ha, oa):
            continue
        # the first differing ensemble step and, in it, the first differing walker in update order (red [0, n) before black)
        step_differs = (hc != oc).reshape(LONG_CHUNK, -1).any(axis=1)
        assert step_differs.any(), "accepted counts differ but no stored step does"
        s = int(np.argmax(step_differs))
        w = int(np.argmax((hc[s] != oc[s]).any(axis=1)))
        color, wi = (0, w) if w < n else (1, w - n)
        done = c * LONG_CHUNK
        # the oracle again from the start of the chunk (where both sides were identical) to that half-step
        rep = po.Oracle(W, D, po.CALC_DENSE_GAUSSIAN, P.ravel(), seed=0, dtype=po.F32)
        rep.set_state(before[0], before[1])
        rep.seek(done)
        if s > 0:
            rc, _ = rep.run(s, mode=po.MODE_COUNTER, threads=16)
            np.testing.assert_array_equal(rc, oc[:s])
        if color == 1:
            rep.half_step_shard(0, 0, n)
            rep.half_step_commit()
        rep.half_step_shard(color, 0, wi)
        ties_before = rep.near_ties
        rep.half_step_shard(color, wi, 1)
        ties_after = rep.near_ties
        tie = rep.last_near_tie()
        rep.half_step_shard(color, wi + 1, n - wi - 1)
        rep.half_step_commit()
        half = slice(0, n) if color == 0 else slice(n, W)
        np.testing.assert_array_equal(rep.get_state()[0][half], oc[s][half])   # (the replay is the oracle's own path)
        dev_ties = hip.counters()["near_ties"] - dev_ties_before
        print("\nfirst divergence at ensemble step %d (chunk %d, step %d of it), walker %d (%s): oracle near ties across that one decision: %d;"
              " device near ties in the chunk: %d; last_near_tie = %s" % (done + s, c, s, w, "red" if color == 0 else "black",
                                                                           ties_after - ties_before, dev_ties, tie))
        assert ties_after - ties_before == 1, "device and oracle part at a decision the oracle did not flag as a near tie"
        assert tie is not None and tie[0] == 2 * (done + s) + color and tie[1] == w
        assert dev_ties >= 1, "the device flagged no near tie in the chunk in which it left the oracle"
        print("fp32 long run: first divergence at ensemble step %d of %d, at a flagged decision: ln_u = %.9g, delta = %.9g (%.1f s)"
              % (done + s, LONG_STEPS, tie[3], tie[4], time.time() - t0))
        return
    for a, b, what in zip(hip.get_state(), orc.get_state(), ("positions", "logp", "n_accept")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    c = hip.counters()
    assert c["near_ties"] == orc.near_ties and c["redraws"] == orc.redraws == 0
    print("\nfp32 long run: no divergence in %d steps (%d near ties on both sides, %.1f s)" % (LONG_STEPS, orc.near_ties, time.time() - t0))
