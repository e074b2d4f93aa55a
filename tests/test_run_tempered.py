"""Tempered runs in one call (mcmcpp_hip_run_tempered, mcmcpp_hip_run_tempered_device, HipSampler.run_tempered): the replica
exchange rounds inside a run's launch sequence.

Against tests/replica_restatement.py, bit for bit, on the cases of tests/test_temper_plan.py (whose input conditions are asserted
there without a GPU, and here again); against the device's own segment loop (HipSampler.run_exchanging, which this entry replaces
but does not touch); in two calls with the round number carried over; with a plug-in calculator; and the refusals."""
import numpy as np
import pytest

from mcmcpp_amd import capi
from oracle import pyoracle as po
from tests import replica_restatement as rr
from tests.test_plugin_contract import COUPLED_TABLE, EX_D, EX_SEED, EX_W, exchange_ladder, plugin  # noqa: F401  (plugin: a fixture)
from tests.test_replica_exchange import _MC_OFF, _MC_ON, STREAM, STREAM_CASE, _dense, _ladder, _refused, _restated, _seed_of
from tests.test_temper_plan import TEMPERED_CASES, restated_once

E_ARG, E_UNSUPPORTED, E_STATE = 1, 4, 5

# (case, the environment switches of its step path)
PATHS = [
    ("A", {"MCMCPP_HIP_FULL_STEP": "1"}),  # every = 1: the rounds meet both buffer parities of the full-step path
    ("A", {"MCMCPP_HIP_FULL_STEP": "0"}),
    ("C", dict(_MC_ON, MCMCPP_HIP_FULL_STEP="1")),
    ("D", dict(_MC_OFF)),
    ("E", {}),
    ("F", {}),
    ("G", {}),
    ("G2", {}),
    ("H", {}),
]


def _handle(K, W, D, calc, dtype, seed, env, monkeypatch, stream=0):
    """a handle of the ladder of tests/test_replica_exchange.py in its initial state"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    _, pos, logp, params = _restated(K, W, D, calc, dtype, seed, stream)
    hip = capi.HipSampler(W, D, calc, np.stack(params), seed=seed, stream=stream, dtype=dtype, num_chains=K)
    hip.set_state(pos, logp)
    return hip


def _same(got, want, what):
    """two results of run_tempered / run_exchanging: chain, accepted per step, swap counters, next round"""
    gc, wc = (x.cpu().numpy() if capi._is_tensor(x) else x for x in (got[0], want[0]))
    np.testing.assert_array_equal(gc, wc, err_msg=what + ": chain")
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": accepted per step")
    for key in ("proposed", "accepted", "near_ties"):
        np.testing.assert_array_equal(got[2][key], want[2][key], err_msg="%s: %s" % (what, key))
    assert got[3] == want[3], what


def _same_state(a, b, what):
    for x, y, name in zip(a.get_state(), b.get_state() if hasattr(b, "get_state") else b, ("positions", "log-posteriors", "n_accept")):
        np.testing.assert_array_equal(x, y, err_msg="%s: %s" % (what, name))


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", PATHS, ids=["%s-%s" % (n, "-".join("%s%s" % (k[11:], v) for k, v in sorted(e.items())) or "default") for n, e in PATHS])
def test_tempered_run_equals_the_restatement(monkeypatch, name, env):
    """One run_tempered call against Ladder.run_exchanging: the chain, the accepted counts per step, the swap counters, the next
    round number and the state afterwards, array for array; no redraw, no near tie of the steps in fp64, none of the exchange;
    and a run(2) behind it still agrees -- what a missing moved bit or a round applied to the wrong buffer would break.  The
    input conditions (tests/test_temper_plan.py asserts them on the CPU) are asserted here again."""
    K, W, D, calc, dtype, n_saved, interval, every, n_rounds, least, most = TEMPERED_CASES[name]
    want = restated_once(name)
    counts = [int(r["accepted"][a]) for rnd, r in want["rounds"] for a, _ in rr.pairs_of(K, rnd)]
    assert len(want["rounds"]) == n_rounds and (min(counts), max(counts)) == (least, most) and W // 8 <= least and most <= W - W // 8
    assert not any(r["in_band"] or r["near_ties"].any() for _, r in want["rounds"])
    hip = _handle(K, W, D, calc, dtype, _seed_of(K), env, monkeypatch)
    chain, acc, swaps, nxt = hip.run_tempered(n_saved, interval=interval, exchange_every=every)
    print(name, "rounds", n_rounds, "accepted", swaps["accepted"], "of", swaps["proposed"], "near ties", swaps["near_ties"])
    assert nxt == want["next"] == n_rounds
    np.testing.assert_array_equal(acc, want["acc"], err_msg="accepted per step")
    np.testing.assert_array_equal(chain, want["chain"], err_msg="chain")
    for key in ("proposed", "accepted", "near_ties"):
        np.testing.assert_array_equal(swaps[key], want["swaps"][key], err_msg=key)
    assert not swaps["near_ties"].any()
    _same_state(hip, want["state"], "after the tempered run")
    final_chain, final_acc = hip.run(2)
    np.testing.assert_array_equal(final_chain, want["final_chain"], err_msg="final run")
    np.testing.assert_array_equal(final_acc, want["final_acc"], err_msg="final run")
    c = hip.counters()
    assert c["redraws"] == 0 and c["ensemble_steps"] == n_saved * interval + 2
    if dtype == po.F64:
        assert c["near_ties"] == 0


LOOP_CASES = [
    # n_saved, interval, exchange_every, first_round, environment
    (6, 1, 2, 5, {}),
    (5, 2, 4, 8, {}),  # a tail shorter than exchange_every
    (7, 1, 2, 1, {"MCMCPP_HIP_GRAPH_STEPS": "3"}),  # replays shorter and longer than a piece
    (7, 1, 2, 0, {"MCMCPP_HIP_FULL_STEP": "0", "MCMCPP_HIP_CHAIN_SUBCHUNK_MB": "1"}),  # sub-chunks of three stored steps: a piece ends with one
    (4, 1, 1, 2, {"MCMCPP_HIP_GRAPH_STEPS": "0"}),  # plain launches
]


@pytest.mark.gpu
@pytest.mark.parametrize("n_saved,interval,every,first,env", LOOP_CASES)
def test_tempered_run_equals_the_segment_loop_on_every_chain_delivery(monkeypatch, n_saved, interval, every, first, env):
    """run_exchanging on a second handle in the same state, with a host destination and with device=True, against run_tempered
    with a pageable out, a pinned out (the trickle and direct paths where the handle takes them) and device=True: identical
    chains, counts, counters and states."""
    K, W, D = 4, 600, 17
    make = lambda: _handle(K, W, D, po.CALC_DENSE_GAUSSIAN, po.F64, 7, env, monkeypatch)  # noqa: E731
    loop_host, loop_dev = make(), make()
    want = loop_host.run_exchanging(n_saved, interval=interval, exchange_every=every, first_round=first)
    _same(loop_dev.run_exchanging(n_saved, interval=interval, exchange_every=every, first_round=first, device=True), want, "the loop with device=True")
    assert want[3] == first + n_saved * interval // every and want[2]["accepted"].all()
    outs = {"pageable out": np.empty((K, n_saved, W, D)), "pinned out": capi.pinned_empty((K, n_saved, W, D)), "default": None}
    for what, out in outs.items():
        h = make()
        got = h.run_tempered(n_saved, interval=interval, exchange_every=every, first_round=first, out=out)
        assert out is None or got[0] is out
        _same(got, want, what)
        _same_state(h, loop_host, what)
        assert h.counters() == loop_host.counters()
    h = make()
    got = h.run_tempered(n_saved, interval=interval, exchange_every=every, first_round=first, device=True)
    assert got[0].is_cuda and tuple(got[0].shape) == (K, n_saved, W, D)
    _same(got, want, "device=True")
    _same_state(h, loop_dev, "device=True")
    # and the runs behind them agree
    np.testing.assert_array_equal(h.run(3)[0], loop_host.run(3)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case,stream", [((4, 600, 17, po.CALC_DENSE_GAUSSIAN, po.F64, {}, 4, 3), 0), (STREAM_CASE, STREAM)], ids=["stream0", "stream2^63+5"])
def test_two_calls_continue_one_tempered_run(monkeypatch, case, stream):
    """run_tempered(6, every 3) then run_tempered(5, every 3, first_round carried over) equals run_tempered(11, every 3): the
    first call's length is a multiple of exchange_every.  Once with the handle's own stream 2^63 + 5, whose exchange stream has
    an increment with a zero high word; that one also against the restatement."""
    K, W, D, calc, dtype, env = case[:6]
    one = _handle(K, W, D, calc, dtype, _seed_of(K), env, monkeypatch, stream)
    two = _handle(K, W, D, calc, dtype, _seed_of(K), env, monkeypatch, stream)
    chain, acc, swaps, nxt = one.run_tempered(11, exchange_every=3, first_round=4)
    c1, a1, s1, n1 = two.run_tempered(6, exchange_every=3, first_round=4)
    c2, a2, s2, n2 = two.run_tempered(5, exchange_every=3, first_round=n1)
    assert (n1, n2, nxt) == (6, 7, 7)
    np.testing.assert_array_equal(np.concatenate([c1, c2], axis=1), chain)
    np.testing.assert_array_equal(np.concatenate([a1, a2], axis=1), acc)
    for key in swaps:
        np.testing.assert_array_equal(s1[key] + s2[key], swaps[key])
    assert swaps["proposed"].tolist() == [W * len([r for r in (4, 5, 6) if r % 2 == k % 2]) for k in range(K - 1)]
    _same_state(one, two, "two calls")
    if stream:
        lad = _restated(K, W, D, calc, dtype, _seed_of(K), stream)[0]
        want_chain, want_acc, want_swaps, want_next = lad.run_exchanging(11, exchange_every=3, first_round=4)
        np.testing.assert_array_equal(chain, want_chain)
        np.testing.assert_array_equal(acc, want_acc)
        np.testing.assert_array_equal(swaps["accepted"], want_swaps["accepted"])
        assert want_next == nxt and not swaps["near_ties"].any()
        _same_state(one, lad, "stream 2^63 + 5")


@pytest.mark.gpu
def test_tempered_run_of_a_plugin_calculator(monkeypatch, plugin):  # noqa: F811
    """The contract functor of tests/cpp/plugin_contract.hip, two chains with different blocks, against the segment loop on the
    device: the cross kernel hands each workgroup row the block of the chain it evaluates for (the functor reads its block in
    every hook: the table in LDS, Regs, and the parameter block in eval)."""
    params = np.stack(exchange_ladder()[:2])
    assert not np.array_equal(params[0], params[1])
    pos = np.stack([po.init_positions(po.F64, EX_W, EX_D, salt=90 + k) for k in range(2)])

    def make():
        h = capi.HipSampler(EX_W, EX_D, COUPLED_TABLE, params, seed=EX_SEED, num_chains=2)
        h.set_state(pos, np.stack([h.calc_logp(pos[k], chain=k) for k in range(2)]))
        return h

    loop, tempered = make(), make()
    want = loop.run_exchanging(6, exchange_every=2, first_round=2)
    got = tempered.run_tempered(6, exchange_every=2, first_round=2)
    _same(got, want, "plug-in")
    _same_state(tempered, loop, "plug-in")
    assert want[2]["proposed"].tolist() == [2 * EX_W] and 0 < want[2]["accepted"][0] < 2 * EX_W  # (rounds 2 and 4 pair the two chains)
    np.testing.assert_array_equal(tempered.run(2)[0], loop.run(2)[0])


@pytest.mark.gpu
def test_refusals(monkeypatch):
    de = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8), mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    _refused(lambda: de.run_tempered(2), E_UNSUPPORTED, "differential-evolution")
    batch = capi.HipSampler(512, 8, capi.CALC_BATCH, None, batch_callback=(capi.BATCH_LOGP_FN(lambda *a: 0), None))
    _refused(lambda: batch.run_tempered(2), E_UNSUPPORTED, "batch target")
    shard = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8), shard_begin=0, shard_count=128)
    _refused(lambda: shard.run_tempered(2), E_UNSUPPORTED, "sharded")
    one = capi.HipSampler(512, 8, po.CALC_DENSE_GAUSSIAN, _dense(8))
    pos = po.init_positions(po.F64, 512, 8, salt=1)
    one.set_state(pos, one.calc_logp(pos))
    _refused(lambda: one.run_tempered(2), E_ARG, "num_chains must be at least 2")
    fresh = capi.HipSampler(64, 3, po.CALC_DENSE_GAUSSIAN, np.stack(_ladder(po.CALC_DENSE_GAUSSIAN, 3, 2)), num_chains=2)
    _refused(lambda: fresh.run_tempered(2), E_STATE, "set_state has not been called")
    hip = _handle(2, 64, 3, po.CALC_DENSE_GAUSSIAN, po.F64, 3, {}, monkeypatch)
    before = hip.get_state()
    _refused(lambda: hip.run_tempered(2, exchange_every=0), E_ARG, "exchange_every must be at least 1")
    _refused(lambda: hip.run_tempered(2, first_round=2**40 - 1), E_ARG, "rounds are below 2^40")
    _refused(lambda: hip.run_tempered(2, first_round=2**40 - 1, device=True), E_ARG, "rounds are below 2^40")
    assert capi.lib().mcmcpp_hip_run_tempered(hip.h, -1, 1, 1, 0, None, None, None, None, None, None) == E_ARG  # (the run's own refusal)
    assert capi.lib().mcmcpp_hip_run_tempered(None, 1, 1, 1, 0, None, None, None, None, None, None) == E_ARG
    for x, y in zip(before, hip.get_state()):
        np.testing.assert_array_equal(x, y)  # (a refused call has touched nothing)
    # zero steps: success, zero rounds; and the last round is served
    chain, acc, swaps, nxt = hip.run_tempered(0, first_round=9)
    assert chain.shape == (2, 0, 64, 3) and nxt == 9 and swaps["proposed"].tolist() == [0]
    assert hip.run_tempered(1, first_round=2**40 - 2)[2]["proposed"].tolist() == [64]
    # while an asynchronous run is in progress
    one.run_async(200)
    _refused(lambda: one.run_tempered(2), E_STATE, "asynchronous run is in progress")
    one.run_wait()
