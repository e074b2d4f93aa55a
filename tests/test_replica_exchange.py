"""Parallel tempering on the device (mcmcpp_hip_exchange_chains, HipSampler.exchange_chains / run_exchanging): the K chains of
one handle on a ladder of targets, with replica-exchange rounds between runs.  Everything is compared, bit for bit, with
tests/replica_restatement.py: K oracles and the exchange written out in Python."""
import math
import os
import subprocess

import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po
from tests import replica_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED, E_STATE = 1, 4, 5

_MC_ON = {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "0"}
_MC_OFF = {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "-1"}


def _ladder(calc, D, K, t=np.float64):
    """chain k's parameter block: chain 0's target flattened by beta_k"""
    betas = {2: (1.0, 0.7), 3: (1.0, 0.5, 0.25), 4: (1.0, 0.7, 0.5, 0.35)}.get(K) or tuple(0.75 ** k for k in range(K))
    if D <= 2:  # (few dimensions: a steeper ladder, so that a good part of the swaps is rejected)
        betas = (1.0, 0.3, 0.1, 0.03)[:K]
    if calc == po.CALC_DENSE_GAUSSIAN:
        a = np.random.default_rng(100 + D).standard_normal((D, D))
        P = a @ a.T / D + np.eye(D)
        return [(b * P).astype(t).ravel() for b in betas]
    if calc == po.CALC_ROSENBROCK:
        return [np.array([1.0, 100.0, 0.05 * b], dtype=t) for b in betas]
    if calc == po.CALC_SKEWED_GAUSSIAN_2D:  # (the epsilon ladder: the narrow direction widens)
        return [np.array([0.13 / b], dtype=t) for b in betas]
    raise ValueError(calc)


def _restated(K, W, D, calc, dtype, seed, stream=0):
    """(restatement in its initial state, that state, the ladder's parameters)"""
    params = _ladder(calc, D, K, po.np_dtype(dtype))
    lad = rr.Ladder(W, D, calc, params, seed, dtype=dtype, stream=stream)
    pos = np.stack([po.init_positions(dtype, W, D, salt=90 + k) for k in range(K)])
    logp = np.stack([lad.logp(k, pos[k]) for k in range(K)])
    lad.set_state(pos, logp)
    return lad, pos, logp, params


def _pair(K, W, D, calc, dtype, seed, env, monkeypatch, stream=0):
    """(handle, restatement) of the same ladder in the same initial state"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    lad, pos, logp, params = _restated(K, W, D, calc, dtype, seed, stream)
    hip = capi.HipSampler(W, D, calc, np.stack(params), seed=seed, stream=stream, dtype=dtype, num_chains=K)
    hip.set_state(pos, logp)
    return hip, lad


def _assert_same_state(hip, lad, what):
    pos, logp, nacc = hip.get_state()
    opos, ologp, onacc = lad.get_state()
    np.testing.assert_array_equal(pos, opos, err_msg=what + ": positions")
    np.testing.assert_array_equal(logp, ologp, err_msg=what + ": log-posteriors")
    np.testing.assert_array_equal(nacc, onacc, err_msg=what + ": n_accept")
    assert int(nacc.sum()) == int(onacc.sum())


ROUND_CASES = [
    (4, 600, 17, po.CALC_DENSE_GAUSSIAN, po.F64, {"MCMCPP_HIP_FULL_STEP": "1"}, 4, 3),
    (4, 600, 17, po.CALC_DENSE_GAUSSIAN, po.F64, {"MCMCPP_HIP_FULL_STEP": "0"}, 4, 3),
    (2, 2054, 32, po.CALC_DENSE_GAUSSIAN, po.F64, dict(_MC_ON, MCMCPP_HIP_FULL_STEP="1"), 4, 3),  # W no multiple of 64
    (16, 256, 20, po.CALC_DENSE_GAUSSIAN, po.F64, dict(_MC_OFF), 4, 3),  # all 8 slots, then 7
    (3, 512, 7, po.CALC_ROSENBROCK, po.F64, {}, 4, 3),
    (4, 320, 2, po.CALC_SKEWED_GAUSSIAN_2D, po.F64, {}, 4, 3),  # the shortest rows: one 16-byte piece
    (4, 600, 9, po.CALC_DENSE_GAUSSIAN, po.F32, {}, 4, 3),  # rows of 36 bytes: no 16-byte pieces
    (2, 66, 1, po.CALC_DENSE_GAUSSIAN, po.F32, {}, 4, 3),  # rows of 4 bytes
    (2, 2050, 1024, po.CALC_ROSENBROCK, po.F64, {}, 1, 1),  # the longest rows: one round, one step in front of it
]
STREAM_CASE = (4, 320, 7, po.CALC_DENSE_GAUSSIAN, po.F64, {}, 4, 3)  # with STREAM, the handle's own
STREAM = 2**63 + 5


def _seed_of(K):
    return 40 + K


def test_the_fp32_cases_meet_no_decision_inside_the_near_tie_band():
    """A condition on the inputs, from the restatement alone (CPU): with their seeds the fp32 cases of ROUND_CASES decide nothing
    inside the near-tie band in any round, so test_exchange_rounds_equal_the_restatement compares every round and the final run
    of theirs too.  (On the device the steps in front of a round are the restatement's bit for bit: that test asserts it.)"""
    f32 = [c for c in ROUND_CASES if c[4] == po.F32]
    assert [(c[0], c[1], c[2]) for c in f32] == [(4, 600, 9), (2, 66, 1)]
    for K, W, D, calc, dtype, _, rounds, steps in f32:
        lad = _restated(K, W, D, calc, dtype, _seed_of(K))[0]
        for r in range(rounds):
            lad.run(steps)
            want = lad.exchange(r)
            assert not want["in_band"] and not want["near_ties"].any(), (K, W, D, r, want["in_band"])
            assert want["proposed"].sum() == W * len(rr.pairs_of(K, r))


def _rounds_equal_the_restatement(monkeypatch, K, W, D, calc, dtype, env, rounds, steps, stream=0):
    hip, lad = _pair(K, W, D, calc, dtype, _seed_of(K), env, monkeypatch, stream)
    for r in range(rounds):
        hc, ha = hip.run(steps)
        oc, oa = lad.run(steps)
        np.testing.assert_array_equal(hc, oc, err_msg="run before round %d" % r)
        np.testing.assert_array_equal(ha, oa, err_msg="run before round %d" % r)
        want = lad.exchange(r)
        got = hip.exchange_chains(r)
        print("round", r, "accepted", want["accepted"], "of", want["proposed"], "near ties", want["near_ties"], got["near_ties"])
        if K == 16:
            assert len(rr.pairs_of(K, r)) == (7 if r & 1 else 8)
        for a, _ in rr.pairs_of(K, r):  # a condition on the inputs
            assert W // 8 <= want["accepted"][a] <= W - W // 8, (r, a, want["accepted"][a])
        assert not want["in_band"], want["in_band"]  # a condition on the inputs (fp32: also asserted without a GPU, above)
        assert not want["near_ties"].any() and not got["near_ties"].any()
        np.testing.assert_array_equal(got["proposed"], want["proposed"])
        np.testing.assert_array_equal(got["accepted"], want["accepted"])
        _assert_same_state(hip, lad, "after round %d" % r)
    hc, ha = hip.run(2)
    oc, oa = lad.run(2)
    np.testing.assert_array_equal(hc, oc, err_msg="final run")
    np.testing.assert_array_equal(ha, oa, err_msg="final run")
    c = hip.counters()
    assert c["redraws"] == 0
    if dtype == po.F64:
        assert c["near_ties"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("K,W,D,calc,dtype,env,rounds,steps", ROUND_CASES)
def test_exchange_rounds_equal_the_restatement(monkeypatch, K, W, D, calc, dtype, env, rounds, steps):
    """set_state, then `rounds` times run(steps) and exchange_chains(r): after every exchange the state (positions,
    log-posteriors, n_accept) equals the restatement's array for array, so do the per-pair counters, and so does a final
    run(2).  The inputs are first checked on the restatement's own counts: every pair of every round accepts at least W/8
    swaps and rejects at least W/8, and no case meets a decision inside the near-tie band of the exchange in any round (so
    that Python's log against fast_log cannot be a source of disagreement): every round and the final run are compared in
    every case, the fp32 ones included."""
    _rounds_equal_the_restatement(monkeypatch, K, W, D, calc, dtype, env, rounds, steps)


@pytest.mark.gpu
def test_exchange_rounds_with_a_handle_stream_of_its_own(monkeypatch):
    """The same with stream = 2^63 + 5 in the handle and in rr.Ladder: the steps draw from (seed + k, stream), the exchange from
    (seed, 2^64 - 1 - stream), whose increment has a zero high word (replica_stream_of, replica_seed)."""
    assert (((2**64 - 1 - STREAM) << 1) | 1) >> 64 == 0 and (((2**64 - 1) << 1) | 1) >> 64 == 1
    _rounds_equal_the_restatement(monkeypatch, *STREAM_CASE, stream=STREAM)


@pytest.mark.gpu
def test_run_exchanging_on_the_device_on_the_host_and_restated(monkeypatch):
    K, W, D, n_saved = 4, 600, 17, 6
    hip, lad = _pair(K, W, D, po.CALC_DENSE_GAUSSIAN, po.F64, 7, {}, monkeypatch)
    dev, _ = _pair(K, W, D, po.CALC_DENSE_GAUSSIAN, po.F64, 7, {}, monkeypatch)
    want_chain, want_acc, want_swaps, want_next = lad.run_exchanging(n_saved, exchange_every=2, first_round=5)
    chain, acc, swaps, nxt = hip.run_exchanging(n_saved, exchange_every=2, first_round=5)
    dchain, dacc, dswaps, dnxt = dev.run_exchanging(n_saved, exchange_every=2, first_round=5, device=True)
    assert nxt == dnxt == want_next == 8
    assert chain.shape == (K, n_saved, W, D) and tuple(dchain.shape) == chain.shape and dchain.is_cuda
    np.testing.assert_array_equal(chain, want_chain)
    np.testing.assert_array_equal(dchain.cpu().numpy(), want_chain)
    np.testing.assert_array_equal(acc, want_acc)
    np.testing.assert_array_equal(dacc, want_acc)
    for key in ("proposed", "accepted", "near_ties"):
        np.testing.assert_array_equal(swaps[key], want_swaps[key])
        np.testing.assert_array_equal(dswaps[key], want_swaps[key])
    assert swaps["accepted"].all() and not swaps["near_ties"].any()
    _assert_same_state(hip, lad, "host chain")
    _assert_same_state(dev, lad, "device chain")
    # an interval, a tail shorter than exchange_every (no trailing exchange), and the caller's array
    out = np.empty((K, 5, W, D))
    chain, acc, swaps, nxt = hip.run_exchanging(5, interval=2, exchange_every=4, first_round=nxt, out=out)
    want_chain, want_acc, want_swaps, want_next = lad.run_exchanging(5, interval=2, exchange_every=4, first_round=want_next)
    assert chain is out and nxt == want_next == 10 and acc.shape == (K, 10)
    np.testing.assert_array_equal(chain, want_chain)
    np.testing.assert_array_equal(acc, want_acc)
    np.testing.assert_array_equal(swaps["accepted"], want_swaps["accepted"])
    with pytest.raises(ValueError):
        hip.run_exchanging(4, interval=2, exchange_every=3)


@pytest.mark.gpu
def test_rounds_are_stateless(monkeypatch):
    """The round number is the caller's: a second handle given the first one's state after round 2 (set_state + seek) computes
    the same round 3 and the same steps behind it.  With K = 2 an odd round has no pair: nothing changes."""
    K, W, D = 3, 512, 7
    a, _ = _pair(K, W, D, po.CALC_ROSENBROCK, po.F64, 21, {}, monkeypatch)
    for r in range(3):
        a.run(3, save_chain=False, want_accepted=False)
        a.exchange_chains(r)
    pos, logp, _ = a.get_state()
    b, _ = _pair(K, W, D, po.CALC_ROSENBROCK, po.F64, 21, {}, monkeypatch)
    b.set_state(pos, logp)
    b.seek(9)
    ra, rb = a.exchange_chains(3), b.exchange_chains(3)
    assert ra["accepted"][1] > 0 and ra["proposed"].tolist() == [0, W]
    for key in ra:
        np.testing.assert_array_equal(ra[key], rb[key])
    pa, la, _ = a.get_state()
    pb, lb, _ = b.get_state()
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(la, lb)
    assert not np.array_equal(pa, pos)
    ca, _ = a.run(2)
    cb, _ = b.run(2)
    np.testing.assert_array_equal(ca, cb)
    two, _ = _pair(2, W, D, po.CALC_ROSENBROCK, po.F64, 21, {}, monkeypatch)
    two.run(2, save_chain=False, want_accepted=False)
    before = two.get_state()
    r = two.exchange_chains(1)
    assert r["proposed"].tolist() == [0] and r["accepted"].tolist() == [0] and r["near_ties"].tolist() == [0]
    for x, y in zip(before, two.get_state()):
        np.testing.assert_array_equal(x, y)
    assert two.exchange_chains(2)["proposed"].tolist() == [W]


@pytest.mark.gpu
def test_non_finite_stored_log_posteriors(monkeypatch):
    """Stored log-posteriors of -inf, +inf and NaN in chosen walkers of either chain: the outcome is what the rule's table says
    (tests/test_replica_plan.py pins replica_accept to the Python rule on every combination), by the comparison alone, and
    none of them is counted as a near tie."""
    K, W, D = 2, 64, 3
    hip, lad = _pair(K, W, D, po.CALC_DENSE_GAUSSIAN, po.F64, 3, {}, monkeypatch)
    pos, logp, _ = hip.get_state()
    inf, nan = math.inf, math.nan
    planted = {(0, 1): -inf, (0, 2): inf, (0, 3): nan, (1, 5): -inf, (1, 6): inf, (1, 7): nan, (0, 9): -inf, (1, 9): -inf, (0, 10): -inf, (1, 10): inf,
               (0, 11): inf, (1, 11): inf, (0, 12): nan, (1, 12): -inf}
    for (k, w), v in planted.items():
        logp[k, w] = v
    hip.set_state(pos, logp)
    want_pos, want_logp = pos.copy(), logp.copy()
    want = rr.exchange_arrays(want_pos, want_logp, lad.logp, 0, 3)
    got = hip.exchange_chains(0)
    got_pos, got_logp, _ = hip.get_state()
    np.testing.assert_array_equal(got_pos, want_pos)
    np.testing.assert_array_equal(got_logp, want_logp)  # (NaN == NaN here: assert_array_equal compares them as equal)
    assert got["accepted"].tolist() == want["accepted"].tolist() and got["near_ties"].tolist() == [0] and want["near_ties"].tolist() == [0]
    swapped = [w for w in range(W) if not np.array_equal(got_pos[0, w], pos[0, w])]
    # delta = +inf accepts: a stored -inf on either side alone, or on both; NaN and -inf deltas reject: +inf stored, NaN stored,
    # and -inf against +inf (inf - inf)
    for w in (1, 5, 9):
        assert w in swapped
    for w in (2, 3, 6, 7, 10, 11, 12):
        assert w not in swapped
    for w in (1, 5, 9):  # the accepted ones carry the cross evaluations, which are finite
        assert np.isfinite(got_logp[0, w]) and np.isfinite(got_logp[1, w])


def _refused(fn, code, text):
    with pytest.raises(capi.HipError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)


def _dense(D):
    return _ladder(po.CALC_DENSE_GAUSSIAN, D, 2)[0]


@pytest.mark.gpu
def test_refused_for_the_differential_evolution_mover():
    de = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8), mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    _refused(lambda: de.exchange_chains(0), E_UNSUPPORTED, "differential-evolution")


@pytest.mark.gpu
def test_refused_for_a_batch_target():
    batch = capi.HipSampler(512, 8, capi.CALC_BATCH, None, batch_callback=(capi.BATCH_LOGP_FN(lambda *a: 0), None))
    _refused(lambda: batch.exchange_chains(0), E_UNSUPPORTED, "batch target")


@pytest.mark.gpu
def test_refused_for_a_sharded_handle():
    shard = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8), shard_begin=0, shard_count=128)
    _refused(lambda: shard.exchange_chains(0), E_UNSUPPORTED, "sharded")


@pytest.mark.gpu
def test_refused_for_a_handle_with_a_communicator():
    comm = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8), comm_world=1, comm_rank=0, comm_id=capi.comm_unique_id())
    _refused(lambda: comm.exchange_chains(0), E_UNSUPPORTED, "communicator")


@pytest.mark.gpu
def test_refused_for_caller_owned_positions():
    import torch
    buf = torch.zeros((512, 8), dtype=torch.float64, device="cuda")
    owned = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8), device_positions=buf.data_ptr())
    _refused(lambda: owned.exchange_chains(0), E_UNSUPPORTED, "caller-owned positions")


@pytest.mark.gpu
def test_refused_for_a_single_chain():
    one = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8))
    pos = po.init_positions(po.F64, 512, 8, salt=1)
    one.set_state(pos, one.calc_logp(pos))
    _refused(lambda: one.exchange_chains(0), E_ARG, "num_chains must be at least 2")


@pytest.mark.gpu
def test_refused_for_a_round_out_of_range(monkeypatch):
    hip, _ = _pair(2, 64, 3, po.CALC_DENSE_GAUSSIAN, po.F64, 3, {}, monkeypatch)
    _refused(lambda: hip.exchange_chains(2**40), E_ARG, "rounds are below 2^40")
    assert hip.exchange_chains(2**40 - 2)["proposed"].tolist() == [64]  # (the last even round is served)


@pytest.mark.gpu
def test_refused_without_a_walker_state():
    """Before set_state.  After a run that failed half way the handle is in the same condition (it insists on a new set_state:
    one flag, one message, which names both causes); a failed run is not provoked here."""
    hip = capi.HipSampler(64, 3, po.CALC_DENSE_GAUSSIAN, np.stack(_ladder(po.CALC_DENSE_GAUSSIAN, 3, 2)), num_chains=2)
    _refused(lambda: hip.exchange_chains(0), E_STATE, "set_state has not been called, or a run failed half way")


@pytest.mark.gpu
def test_refused_while_an_asynchronous_run_is_in_progress(monkeypatch):
    W, D = 512, 8
    P = _dense(D)
    h = capi.HipSampler(W, D, po.CALC_DENSE_GAUSSIAN, P)
    pos = po.init_positions(po.F64, W, D, salt=1)
    h.set_state(pos, h.calc_logp(pos))
    h.run_async(200)
    _refused(lambda: h.exchange_chains(0), E_STATE, "asynchronous run is in progress")
    h.run_wait()


@pytest.mark.gpu
def test_an_iso_gaussian_handle_merely_exchanges():
    """No parameters: all chains have the same target, delta is 0 up to rounding and every proposal with ln U < 0 is accepted."""
    K, W, D = 3, 128, 4
    hip = capi.HipSampler(W, D, po.CALC_ISO_GAUSSIAN, None, seed=2, num_chains=K)
    pos = np.stack([po.init_positions(po.F64, W, D, salt=k) for k in range(K)])
    logp = np.stack([hip.calc_logp(pos[k]) for k in range(K)])
    hip.set_state(pos, logp)
    r = hip.exchange_chains(0)
    assert r["proposed"].tolist() == [W, 0] and r["accepted"][0] >= W - 1
    got_pos, got_logp, _ = hip.get_state()
    moved = [w for w in range(W) if not np.array_equal(got_pos[0, w], pos[0, w])]
    np.testing.assert_array_equal(got_pos[0, moved], pos[1, moved])
    np.testing.assert_array_equal(got_pos[1, moved], pos[0, moved])
    np.testing.assert_array_equal(got_logp[0, moved], logp[1, moved])
    np.testing.assert_array_equal(got_pos[2], pos[2])


def test_entry_point_needs_a_handle_and_is_declared_as_c99(tmp_path):
    """CPU: the entry point exists, refuses a NULL handle, and a C99 translation unit that calls it compiles warning-free."""
    capi.build_library()
    assert capi.lib().mcmcpp_hip_exchange_chains(None, 0, None, None, None) == E_ARG
    assert "mcmcpp_hip_exchange_chains" in capi.EXPORTS
    src = tmp_path / "exchange.c"
    src.write_text('#include "mcmcpp_hip.h"\n'
                   'int one_round(mcmcpp_hip_sampler* h, uint64_t r, uint64_t* acc)\n'
                   '{\n'
                   '    return mcmcpp_hip_exchange_chains(h, r, (uint64_t*)0, acc, (uint64_t*)0);\n'
                   '}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "exchange.o")])
