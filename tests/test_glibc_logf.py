"""mcmcpp::glibc_logf: the device's fp32 logarithm has the bits of the host's logf, so fp32 chains stay the oracle's.

The reference and the oracle take the two logarithms of the accept test with glibc's logf.  The fp32 kernels used OCML's,
which differs from it on 49 % of all floats in [2^-24, 4] (tests/test_accept_logs.py), so that a decision inside the near-tie
band could go the other way on the device: the flagship fp32 configuration left the oracle in ensemble step 608.
mcmcpp_amd/csrc/glibc_logf.hpp restates the logf of glibc 2.28 - 2.40 for host and device; dev_log(float) is that function.

  CPU   tests/cpp/glibc_logf_cases.cpp: the header against the platform's logf on every float in [2^-24, 4], built with g++
        and with hipcc's host pass, and once under -fsanitize=address,undefined over one binade; the public include path
        is the same text; the oracle alone flags near ties on the long run's input (without which the GPU run proves nothing).
  GPU   the production dev_log (tests/cpp/accept_log_device.hip, unchanged) against the GPU host's logf on the same
        218 103 809 floats: none differ; draw records bit-equal to the host restatement; 650 ensemble steps of the flagship
        fp32 configuration, through step 608, identical to the oracle in every chunk; a small fp32 differential-evolution run.

A host whose logf is not that algorithm (glibc 2.41 made logf correctly rounded) fails the exhaustive tests, CPU and GPU
alike; they print the C library's version."""
import ctypes as C
import hashlib
import os
import platform
import re
import subprocess
import time

import numpy as np
import pytest

from mcmcpp_amd import capi, workloads
from oracle import pyoracle as po
from tests.test_accept_logs import _canonical, _edge_raws, _p, dev  # noqa: F401  (dev: the shim's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "glibc_logf_cases.cpp")
FIRST, LAST = 0x33800000, 0x40800000   # 2^-24, 4
TOTAL = 218103809
BINADE = ("3f000000", "3f7fffff")      # [1/2, 1): where most of the sampler's arguments lie

GXX = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror"]
HIPCC_HOST = ["/opt/rocm/bin/hipcc", "-x", "hip", "-include", "hip/hip_runtime.h", "-std=c++17", "-O2", "--offload-arch=gfx950",
              "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror"]


def _build(name, compiler, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call(list(compiler) + list(extra) + ["-I", CSRC, SRC, "-o", exe])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    print("\n%s %s: %s%s(C library: %s)" % (os.path.basename(exe), " ".join(args), r.stdout, r.stderr, " ".join(platform.libc_ver())))
    return r


# ------------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("compiler", ["gxx", "hipcc_host"])
def test_header_returns_the_platform_logf_bits_on_every_argument(compiler):
    """Every float in [2^-24, 4], x = 1 among them, and +0 at x = 1: 218 103 809 arguments, no mismatch, with every operation
    rounded on its own (-ffp-contract=off), under the host compiler and under hipcc's host pass (MCMCPP_HD = __host__
    __device__).  About 3 s on one core."""
    exe = _build("glibc_logf_cases_" + compiler, GXX if compiler == "gxx" else HIPCC_HOST)
    r = _run(exe)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip() == "arguments=%d mismatches=0" % TOTAL


def test_header_under_address_and_undefined_behaviour_sanitizers():
    """The same program built with -fsanitize=address,undefined (the shifts and the signed conversion of the argument's bits,
    the table index), over the binade [1/2, 1) and over the lowest and highest binades the sampler passes."""
    exe = _build("glibc_logf_cases_san", GXX, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for rng in (BINADE, ("33800000", "33ffffff"), ("40000000", "40800000")):
        r = _run(exe, *rng)
        assert r.returncode == 0 and "mismatches=0" in r.stdout and "runtime error" not in r.stderr, (rng, r.stdout, r.stderr)


def test_public_include_path_is_the_same_text():
    """include/MCMCpp/Device/GlibcLogf.h (host Calculators) defines nothing of its own: it includes the kernels' header, and
    a program built through it alone returns logf's bits; mcmcpp_hip_plugin.hpp (device functors) includes that header too."""
    pub = open(os.path.join(ROOT, "include", "MCMCpp", "Device", "GlibcLogf.h")).read()
    assert re.findall(r'^#include\s+(\S+)', pub, re.M) == ['"../../../mcmcpp_amd/csrc/glibc_logf.hpp"']
    assert "glibc_logf(" not in re.sub(r"/\*.*?\*/", "", pub, flags=re.S)
    plugin = open(os.path.join(CSRC, "mcmcpp_hip_plugin.hpp")).read()
    assert '#include "glibc_logf.hpp"' in plugin
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "glibc_logf_cases_public")
    subprocess.check_call(GXX + ['-DGLIBC_LOGF_HEADER="Device/GlibcLogf.h"', "-I", os.path.join(ROOT, "include", "MCMCpp"), SRC, "-o", exe])
    r = _run(exe, *BINADE)
    assert r.returncode == 0 and r.stdout.strip() == "arguments=%d mismatches=0" % (1 << 23)


def test_header_needs_no_hip_header_and_no_libm():
    text = open(os.path.join(CSRC, "glibc_logf.hpp")).read()
    assert re.findall(r"^#include\s+(\S+)", text, re.M) == ["<stdint.h>", "<string.h>"]
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"\b(logf?|log1pf?|expf?|fmaf?|ldexpf?|frexpf?|__builtin_\w+)\s*\(", code)
    # and the kernels' fp32 logarithm is this function (the fp64 one stays fast_log)
    sk = open(os.path.join(CSRC, "stretch_kernel.hpp")).read()
    assert "float dev_log(float x) { return glibc_logf(x); }" in sk and "double dev_log(double x) { return fast_log(x); }" in sk


# ---- the long run's input: 16 384 x 32 dense Gaussian (rho = 0.5), fp32, seed 0; 650 ensemble steps in chunks of 25

LONG_W, LONG_D, LONG_CHUNK, LONG_STEPS = 16384, 32, 25, 650


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def oracle_long_run():
    """The oracle alone, once (about 6 s with 16 threads): per chunk the digest of its stored steps, the accepted counts and
    the counters behind it; the start and the final state."""
    P = workloads.ar1_precision(LONG_D, 0.5, np.float32)
    orc = po.Oracle(LONG_W, LONG_D, po.CALC_DENSE_GAUSSIAN, P.ravel(), seed=0, dtype=po.F32)
    pos = po.init_positions(po.F32, LONG_W, LONG_D, salt=0)
    logp = orc.logp(pos)
    orc.set_state(pos, logp)
    t0 = time.time()
    chunks = []
    for c in range(LONG_STEPS // LONG_CHUNK):
        oc, oa = orc.run(LONG_CHUNK, mode=po.MODE_COUNTER, threads=16)
        chunks.append((_digest(oc), oa.copy(), int(orc.near_ties), int(orc.redraws)))
    print("\noracle: %d steps of %d x %d fp32 in %.1f s, %d near ties, %d redraws" % (LONG_STEPS, LONG_W, LONG_D, time.time() - t0,
                                                                                       chunks[-1][2], chunks[-1][3]))
    return {"P": P, "pos": pos, "logp": logp, "chunks": chunks, "final": orc.get_state()}


def test_oracle_flags_near_ties_on_the_long_runs_input(oracle_long_run):
    """Within the 650 steps the oracle meets decisions inside the near-tie band -- those that a logarithm one ulp off can turn.
    Without any, the device following the oracle through them (test_long_fp32_run_is_the_oracles_through_step_608) would
    say nothing about the logarithm."""
    chunks = oracle_long_run["chunks"]
    assert chunks[-1][2] >= 1
    # step 608, where the kernels with OCML's logf left the oracle, lies in chunk 24: flagged decisions up to and in it
    assert chunks[608 // LONG_CHUNK][2] >= 1


# ------------------------------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
def test_device_log_returns_the_hosts_logf_bits_on_every_argument(dev):
    """dev_log(float) as the kernels call it, on every float in [2^-24, 4], against logf of the host the GPU sits in: zero
    arguments differ (OCML's logf: 107 123 330).  26 launches of one binade each; the host comparison takes the time."""
    t0 = time.time()
    total = differ = dist = worst = 0
    y = np.empty((1 << 23) + 1, dtype=np.float32)
    b = FIRST
    while b <= LAST:
        n = min(1 << 23, LAST - b + 1)
        if b + n == LAST:
            n += 1  # 4.0 itself rides with the last binade
        assert dev.ald_log_f32_range(b, n, _p(y)) == 0
        nd, md, wb = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        dev.ald_compare_logf_range(b, n, _p(y), C.byref(nd), C.byref(md), C.byref(wb))
        total += n
        differ += nd.value
        if md.value > dist:
            dist, worst = md.value, wb.value
        b += n
    print("\ndev_log(float) against the host's logf (C library: %s) on all %d floats in [2^-24, 4]: %d differ, at most %d ulp (first at %s); %.1f s"
          % (" ".join(platform.libc_ver()), total, differ, dist, float(np.uint32(worst).view(np.float32)).hex(), time.time() - t0))
    assert total == TOTAL
    assert differ == 0, "the host's logf is not the algorithm of glibc 2.28 - 2.40 (C library: %s)?" % " ".join(platform.libc_ver())
    one = np.ones(1, dtype=np.float32)
    out = np.empty(1, dtype=np.float32)
    assert dev.ald_log_f32(_p(one), _p(out), 1) == 0 and out.view(np.uint32)[0] == 0   # +0 at x = 1


@pytest.fixture(scope="module")
def raws():
    return np.concatenate([_edge_raws(), np.random.default_rng(7).integers(0, 1 << 64, size=1 << 20, dtype=np.uint64, endpoint=False)])


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 33])
@pytest.mark.parametrize("alpha", [(2, 1), (3, 2)], ids=["alpha2", "alpha3_2"])
def test_fp32_draw_records_are_the_host_restatements_bits(dev, raws, alpha, D):
    """draw_store<float>, tasks 1 (z, zs = fl(ln z * (D-1))) and 2 (ln_u = ln(1-u)), on the edge raw outputs of
    test_accept_logs.py and 2^20 seeded ones: bit-equal to the restatement with the host's logf (ald_host_log_f32), not
    merely within the logarithms' distance."""
    t = np.float32
    n = raws.size
    g1, g0, dm1 = C.c_double(0), C.c_double(0), C.c_double(0)
    dev.ald_stretch_constants(po.F32, alpha[0], alpha[1], D, C.byref(g1), C.byref(g0), C.byref(dm1))
    t1, t0, dminus = t(g1.value), t(g0.value), t(dm1.value)
    assert float(dminus) == D - 1
    u, _ = _canonical(raws, t)
    rec = {}
    for k in (1, 2):
        z, zs, ln_u = (np.empty(n, dtype=t) for _ in range(3))
        assert dev.ald_draw_f32(alpha[0], alpha[1], D, k, _p(raws), n, _p(z), _p(zs), _p(ln_u)) == 0
        rec[k] = z, zs, ln_u

    def host_log(x):
        x = np.ascontiguousarray(x)
        y = np.empty_like(x)
        dev.ald_host_log_f32(_p(x), _p(y), x.size)
        return y

    tmp = (t1 * u).astype(t) + t0
    z = (tmp * tmp).astype(t)
    np.testing.assert_array_equal(rec[1][0].view(np.uint32), z.view(np.uint32))
    np.testing.assert_array_equal(rec[1][1].view(np.uint32), (host_log(z) * dminus).astype(t).view(np.uint32))
    arg = (t(1) - u).astype(t)
    assert (arg >= t(2.0 ** -24)).all() and (arg <= 1).all()
    np.testing.assert_array_equal(rec[2][2].view(np.uint32), host_log(arg).view(np.uint32))


@pytest.mark.gpu
def test_long_fp32_run_is_the_oracles_through_step_608(oracle_long_run):
    """The flagship fp32 configuration for 650 ensemble steps (1.06e7 updates) against the oracle, in chunks of 25 with every
    step stored: stored steps, accepted counts, near-tie and redraw counters identical after every chunk, the final state
    identical, and near ties on both sides -- decisions that OCML's logf could turn and did: with it the device left the
    oracle in step 608 at walker 11 462."""
    o = oracle_long_run
    hip = capi.HipSampler(LONG_W, LONG_D, capi.CALC_DENSE_GAUSSIAN, o["P"].ravel(), seed=0, dtype=po.F32)
    np.testing.assert_array_equal(hip.calc_logp(o["pos"]), o["logp"])
    hip.set_state(o["pos"], o["logp"])
    for c, (want_digest, want_acc, want_ties, want_redraws) in enumerate(o["chunks"]):
        hc, ha = hip.run(LONG_CHUNK)
        cnt = hip.counters()
        np.testing.assert_array_equal(ha, want_acc, err_msg="accepted counts, chunk %d (steps %d..)" % (c, c * LONG_CHUNK))
        assert _digest(hc) == want_digest, "stored steps differ in chunk %d (ensemble steps %d .. %d)" % (c, c * LONG_CHUNK, (c + 1) * LONG_CHUNK - 1)
        assert (cnt["near_ties"], cnt["redraws"]) == (want_ties, want_redraws), "counters after chunk %d" % c
    for a, b, what in zip(hip.get_state(), o["final"], ("positions", "logp", "n_accept")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    cnt = hip.counters()
    print("\nfp32 long run: %d steps identical; near ties %d (device) / %d (oracle)" % (LONG_STEPS, cnt["near_ties"], o["chunks"][-1][2]))
    assert cnt["near_ties"] >= 1 and o["chunks"][-1][2] >= 1


@pytest.mark.gpu
def test_small_fp32_differential_evolution_run_is_the_oracles():
    """64 x 4 isotropic Gaussian in fp32, 4000 ensemble steps of differential evolution (its exponential variate is the
    other caller of dev_log): stored steps, accepted counts, final state and counters, bit for bit."""
    W, D, steps = 64, 4, 4000
    pos = po.init_positions(po.F32, W, D, salt=6)
    orc = po.Oracle(W, D, po.CALC_ISO_GAUSSIAN, None, seed=21, dtype=po.F32, mover=po.MOVER_DIFFERENTIAL_EVOLUTION)
    lp = orc.logp(pos)
    orc.set_state(pos, lp)
    want_chain, want_acc = orc.run(steps, 1)
    s = capi.HipSampler(W, D, capi.CALC_ISO_GAUSSIAN, None, seed=21, dtype=po.F32, mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    s.set_state(pos, lp)
    chain, acc = s.run(steps, 1)
    np.testing.assert_array_equal(acc, want_acc)
    np.testing.assert_array_equal(chain.view(np.uint32), want_chain.view(np.uint32))
    for got, want in zip(s.get_state(), orc.get_state()):
        np.testing.assert_array_equal(got, want)
    c = s.counters()
    print("\nfp32 differential evolution: near ties %d (device) / %d (oracle)" % (c["near_ties"], orc.near_ties))
    assert c["redraws"] == orc.redraws and c["ensemble_steps"] == steps
