"""Sampler handles on generated call sequences, against the oracle as a model (tests/call_sequences.py has both).

Every step kernel, lane mapping and draw path has its own bit-for-bit test; each starts its first run from set_state, at an
even step.  What a handle carries from one call to the next -- the validity of the draw records, the parities that pick the
record and position buffers and are frozen into the graphs, the home buffer of the ensemble, the counters' reset point, the
records made ahead, a run in flight, the graphs dropped by set_chain_params, the graph cache of the differential-evolution
handle, the re-primed records of a batch handle, and on a ladder the rounds of a tempered run (which buffer they find the ensemble
in, the moved bit get_state masks out, the round scratch shared with exchange_chains) and the evidence calls that must leave all
of it alone -- is walked here in 40-operation sequences per (path, seed), six seeds per
path, and compared with the model after every operation: the operation's result, get_state and counters.  There is no
tolerance anywhere.

CPU: the generator is deterministic (a digest of every rendered sequence is pinned: a change of the generator is a visible
change of this file); the six sequences of every path show, between them, every coverage fact of facts_wanted(path) and
every operation kind at least three times; and every sequence meets its input conditions on the oracle alone (no near tie, no
redraw of the stretch move, proposals accepted and rejected, no replica exchange decided inside its near-tie band; on a ladder
also swaps accepted and refused, every log-posterior of an evidence call finite, its solves converged), so that bit-equality is
the right bar.  No sequence is left out: a seed that misses a condition is replaced in call_sequences.SEEDS.

GPU: one test per (path, seed), the directed differential-evolution sequence that crosses the graph cache's limit, and the
shortest failing prefixes found so far, by name."""
import collections

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import call_sequences as cs
from tests.test_batch_calc import cb_lib  # noqa: F401  (the callback library's fixture)

DIGEST = "c6d65c7ce8edf5d90ae736afd099c3c9ecd655b2ade93c76a88ffcb45840a76c"      # the fifteen paths of the first version: as they were
DIGEST_NEW = "cdc2cc8e7c40497ccb4cd35aac6986dcb2be8afe0c6a1310d6dafdc858bd8ef7"  # the ladders and the stretch path with run_device_async
CASES = [(path, seed) for path in cs.PATHS for seed in cs.SEEDS[path]]
CASE_IDS = ["%s-%d" % c for c in CASES]

_MODEL_RUNS = {}


def model_run(path, seed):
    """the sequence on the model alone, computed once"""
    if (path, seed) not in _MODEL_RUNS:
        _MODEL_RUNS[(path, seed)] = cs.model_run(path, seed)[0]
    return _MODEL_RUNS[(path, seed)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_the_generator_is_deterministic_and_pinned():
    assert cs.plan("full_step", 3) == cs.plan("full_step", 3)
    assert len(cs.OLD_PATHS) == 15 and list(cs.PATHS) == list(cs.OLD_PATHS) + list(cs.NEW_PATHS)
    assert cs.digest(paths=cs.OLD_PATHS) == DIGEST, "a sequence of the first fifteen paths changed: they stay as they are"
    assert cs.digest(paths=cs.NEW_PATHS) == DIGEST_NEW, "the generator, its weights, the paths or the seeds changed: look at the sequences, then pin the new digest"


def test_every_path_has_six_sequences_that_start_with_set_state():
    assert len(cs.PATHS) == 22 and set(cs.SEEDS) == set(cs.PATHS)
    for path, seeds in cs.SEEDS.items():
        assert len(seeds) == len(set(seeds)) == 6
        for seed in seeds:
            ops = cs.generate(path, seed)
            assert ops[0][0] == "set_state"
            assert len(ops) == 1 + cs.OPS_PER_SEQUENCE + len(cs.PATHS[path]["directed"])
            # a tempered run whose last round would pass 2^40 - 1 is generated as the refusal it is, never as a run
            for op in ops:
                if op[0] == "run_tempered":
                    assert op[3] >= 1 and op[4] + op[1] * op[2] // op[3] <= cs.MAX_ROUND, op
                if op[:2] == ("refused", "run_tempered_round_out_of_range"):
                    assert op[4] >= 1 and op[5] + op[2] * op[3] // op[4] > cs.MAX_ROUND, op
    # a stream with its top bit set (inc.hi = 1 in pcg_seed), and the special seeds, are met on every path
    for path in cs.PATHS:
        plans = [cs.plan(path, seed) for seed in cs.SEEDS[path]]
        assert any(stream >> 63 for _, stream, _ in plans), path
    everything = [cs.plan(*c)[:2] for c in CASES]
    for special in cs.SPECIAL_64:
        assert any(special == s for s, _ in everything) and any(special == t for _, t in everything)


def test_the_directed_runs_cross_the_default_replay_length():
    directed = cs.PATHS["full_step_default_graphs"]["directed"]
    assert [op[1] * op[2] for op in directed] == [301, 299] and cs.PATHS["full_step_default_graphs"]["graph_steps"] == 300
    for seed in cs.SEEDS["full_step_default_graphs"]:
        ops = cs.generate("full_step_default_graphs", seed)
        i = ops.index(directed[0])
        assert ops[i + 1] == directed[1]
    # the ladder with the default replay length: a tempered run of 301 steps with rounds behind steps 150 and 300, into device
    # memory, then a plain run of 299
    directed = cs.PATHS["ladder3_default_graphs"]["directed"]
    assert directed == (("run_tempered", 301, 1, 150, 0, "device"), ("run", 299, 1, True, True)) and cs.PATHS["ladder3_default_graphs"]["graph_steps"] == 300
    for seed in cs.SEEDS["ladder3_default_graphs"]:
        ops = cs.generate("ladder3_default_graphs", seed)
        i = ops.index(directed[0])
        assert ops[i + 1] == directed[1]


@pytest.mark.parametrize("path", list(cs.PATHS))
def test_the_sequences_of_a_path_cover_its_facts(path):
    """If a fact is missing, the weights change, not this assertion."""
    facts, kinds = set(), collections.Counter()
    for seed in cs.SEEDS[path]:
        m = model_run(path, seed)
        facts |= m.facts
        kinds.update(m.kinds)
    assert not cs.facts_wanted(path) - facts, sorted(cs.facts_wanted(path) - facts)
    rare = {k: kinds[k] for k in cs.kinds_of(path) if kinds[k] < 3}
    assert not rare, rare


@pytest.mark.parametrize("path,seed", CASES, ids=CASE_IDS)
def test_sequences_meet_their_input_conditions(path, seed):
    m = model_run(path, seed)
    assert m.near_ties == 0, "near ties: this sequence needs another seed"
    if cs.PATHS[path]["family"] != "diffevo":
        assert m.redraws == 0, "redraws: this sequence needs another seed"
    assert 0 < m.accepted < m.proposed, "every proposal accepted, or none: this sequence needs another seed"
    assert m.in_band == 0, "a replica exchange decided inside its near-tie band: this sequence needs another seed"
    if cs.PATHS[path]["family"] == "ladder":
        # (rounds inside tempered runs and rounds between runs alike)
        assert m.swaps_accepted > 0 and m.swaps_refused > 0, "every swap accepted, or none: this sequence needs another seed"
        assert m.evidence_nonfinite == 0, "an evidence operation met a log-posterior that is not finite: this sequence needs another seed"
        assert m.evidence_unconverged == 0, "a bridge or MBAR solve did not converge: this sequence needs another seed"


# ---- the directed differential-evolution sequence ---------------------------------------------------------------------------------
# DeSampler::graph_for keeps one graph per (steps of the replay, phase of its first half-step among two batches) and empties
# its cache when a 65th is wanted.  Run lengths 1, 2, ..., 70 on one handle, each below the 128 steps of a replay, are 70
# distinct keys whatever their phases: the run of 65 steps finds 64 graphs cached and takes that branch.
DE_DIRECTED = dict(W=14, D=3, lengths=list(range(1, 71)), seed=77, salt=5)


def de_directed_oracle():
    d = DE_DIRECTED
    orc = po.Oracle(d["W"], d["D"], cs.ISO, None, seed=d["seed"], mover=cs.DE)
    pos = po.init_positions(po.F64, d["W"], d["D"], salt=d["salt"])
    logp = orc.logp(pos)
    orc.set_state(pos, logp)
    chain, acc = orc.run(sum(d["lengths"]))
    return orc, pos, logp, chain, acc


def test_directed_diffevo_sequence_meets_its_conditions():
    orc, _, _, _, acc = de_directed_oracle()
    assert len(set(DE_DIRECTED["lengths"])) == 70 > 64 and max(DE_DIRECTED["lengths"]) < 128
    assert orc.near_ties == 0 and 0 < int(acc.sum()) < DE_DIRECTED["W"] * acc.size


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def set_knobs(monkeypatch, path):
    clear, put = cs.knob_settings(path)
    for k in clear:
        monkeypatch.delenv(k, raising=False)
    for k, v in put.items():
        monkeypatch.setenv(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("path,seed", CASES, ids=CASE_IDS)
def test_generated_sequence(monkeypatch, cb_lib, path, seed):  # noqa: F811
    set_knobs(monkeypatch, path)
    cs.run_sequence(path, seed, cb_lib=cb_lib)


# ---- shortest failing prefixes of generated sequences, kept by name -------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", ["mc_full_step_batch_3", "mc_full_step_batch_0", "full_step"])
def test_half_steps_behind_a_run_whose_launches_read_records_made_ahead(monkeypatch, path):
    """Found by mc_full_step_batch_3, all six seeds (the shortest: seed 2, operations 0..3).  The matrix-core full-step launches of
    one whole ensemble read draw records made ahead in batches and leave the two-buffer records where an earlier step put
    them; half_step_async behind such a run took those for the records of its own step and moved a third of the walkers
    elsewhere.  It makes its step's records now.  (The other two paths passed before: their runs leave the records behind.)"""
    set_knobs(monkeypatch, path)
    ops = [("set_state", 434), ("run", 5, 1, True, True), ("half_step_async", 0), ("half_step_async", 1), ("run", 2, 1, True, True),
           ("half_step_async", 0), ("half_step_async", 1), ("half_step_async", 0), ("half_step_async", 1), ("run", 3, 2, True, True)]
    cs.run_sequence(path, 2, ops=ops)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["ladder3_full_step", "ladder2_full_step_f32"])
def test_an_asynchronous_run_of_several_chains_returns_every_chain(monkeypatch, path):
    """Found while the ladders were given run_async (no multi-chain sequence had a run in flight before).  The library runs all K
    chains on the worker thread and writes chain[K][n_saved][W][D] and accepted[K][steps]; HipSampler.run_async handed it arrays
    for one chain.  It allocates them with the leading K now, as run and run_device_async do."""
    set_knobs(monkeypatch, path)
    ops = [("set_state", 7), ("run_async", 3, 2, True), ("run_wait",)]
    cs.run_sequence(path, 0, ops=ops)


@pytest.mark.gpu
def test_directed_diffevo_run_lengths_1_to_70_cross_the_graph_cache_limit(monkeypatch):
    from mcmcpp_amd import capi
    set_knobs(monkeypatch, "diffevo_iso")
    d = DE_DIRECTED
    orc, pos, logp, want_chain, want_acc = de_directed_oracle()
    hip = capi.HipSampler(d["W"], d["D"], cs.ISO, None, seed=d["seed"], mover=capi.MOVER_DIFFERENTIAL_EVOLUTION)
    hip.set_state(pos, logp)
    got = [hip.run(n) for n in d["lengths"]]
    assert cs.differs(np.concatenate([c for c, _ in got]), want_chain, "the concatenated chain") is None
    assert cs.differs(np.concatenate([a for _, a in got]), want_acc, "accepted per step") is None
    assert cs.differs(hip.get_state(), orc.get_state(), "get_state") is None
    c = hip.counters()
    assert (c["ensemble_steps"], c["near_ties"], c["redraws"]) == (sum(d["lengths"]), 0, orc.redraws)
