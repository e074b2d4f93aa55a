"""Generated call sequences for sampler handles, and the model that says what each call must return.  TEST INFRASTRUCTURE ONLY.

What sits between the step kernels and the caller is host state that a handle carries from one call to the next: which draw
records on the device are still good, the low bits of the step counters that pick record and position buffers and are frozen
into captured graphs, which position buffer holds the ensemble, the counters' reset point, a run in flight on the worker
thread.  A generated sequence walks the public entry points in an order nobody wrote down; the model below -- po.Oracle (K of
them for K chains, chain k seeded seed + k as the library does) plus the bookkeeping of a handle restated in a few lines --
returns what the handle must return for every operation, bit for bit.

  plan(path, seed)      -> (handle seed, handle stream, operations); deterministic: its only randomness is
                           numpy.random.default_rng((path index, seed)), read through integers() and random() alone
  generate(path, seed)  -> the operations
  Model(path, ...)      -> .apply(op) returns the expected result, .state() the expected get_state / counters
  run_sequence(...)     -> executes a sequence on a capi.HipSampler beside the model and compares after every operation
  replay(path, seed, upto)  the same up to an operation, for debugging (sets the path's knobs in os.environ itself)

Operations are tuples, the kind first:
  ("set_state", salt)                       po.init_positions(salt + chain), log-posteriors by the chain's own calculator
  ("run", n_saved, interval, save_chain, want_accepted)
  ("run_async", n_saved, interval, want_accepted)   then only the next three until run_wait
  ("refused_in_flight", "seek" | "calc_logp" | "get_state")   must return MCMCPP_HIP_E_STATE and change nothing
  ("wait_stored", k)                        the first k stored steps are compared when it returns
  ("run_wait",)                             the run's result is compared
  ("run_device", n_saved, interval, want_accepted)  into a torch tensor, read back
  ("half_step_async", colour), ("synchronize",)
  ("seek", step), ("reset_counters",), ("get_state",), ("counters",)
  ("calc_logp", count, rows seed, chain or None), ("calc_logp_device", count, rows seed, chain)
  ("refused", "run_negative" | "run_interval_0" | "half_step_out_of_order" | "seek_unsupported")
  ("set_chain_params", chain, index into BETAS), ("exchange_chains", round)
and on the ladders (family "ladder": K >= 2 chains, a tempered handle):
  ("run_device_async", n_saved, interval, want_accepted)   run_async into a torch tensor (also a stretch operation)
  ("run_tempered", n_saved, interval, exchange_every, first_round, "pageable" | "pinned" | "device")
                                            compared as (chain, accepted per step, swaps dict, next round)
  ("evidence", "ratios" | "bridge" | "mbar", n, rows seed, "host" | "device")   on draws [K][n][W][D] made from the seed alone
  ("refused", "run_tempered_every_0" | "half_step_async"), ("refused", "run_tempered_round_out_of_range", n_saved, interval,
   exchange_every, first_round): a generated tempered run whose last round would pass 2^40 - 1 is this refusal
  ("refused_in_flight", ... | "run_tempered" | "exchange_chains" | "set_chain_params" | "evidence")
"""
import collections
import hashlib
import os

import numpy as np

from oracle import pyoracle as po
from tests import replica_restatement as rr

E_ARG, E_UNSUPPORTED, E_STATE = 1, 4, 5
M64 = 2**64 - 1
ISO, DENSE, ROSENBROCK = po.CALC_ISO_GAUSSIAN, po.CALC_DENSE_GAUSSIAN, po.CALC_ROSENBROCK
STRETCH, DE = po.MOVER_STRETCH, po.MOVER_DIFFERENTIAL_EVOLUTION

# ---- the paths, as data -------------------------------------------------------------------------------------------------------
# env: the knobs set before the handle is created (every name in KNOBS is cleared first); create: keyword arguments of
# capi.HipSampler.  graph_steps / full_step restate what the library makes of them (step_plan.hpp: 300 steps per replay by
# default for ensembles this small, 128 for differential evolution) -- used for the coverage facts alone, and the GPU test
# checks full_step against the launches the handle counts.  long_runs: run shapes beyond n_saved 0..9 x interval 1..4 that put
# run lengths at and above the path's replay length; directed: operations put in after the 20th generated one.
KNOBS = ("MCMCPP_HIP_FULL_STEP", "MCMCPP_HIP_GRAPH_STEPS", "MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS", "MCMCPP_HIP_BATCH_DRAWS",
         "MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS", "MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS", "MCMCPP_HIP_DE_BATCH", "MCMCPP_HIP_DE_SCAN_RUN",
         "MCMCPP_HIP_NO_DRAW_WAVE", "MCMCPP_HIP_PASSES", "MCMCPP_HIP_TRICKLE", "MCMCPP_HIP_CHAIN_SUBCHUNK_MB", "MCMCPP_HIP_PINNED_DIRECT",
         "MCMCPP_HIP_FULL_STEP_MAX_WALKERS", "MCMCPP_HIP_TASK_TABLE_MB", "MCMCPP_HIP_WAVES_PER_SIMD")
_FULL, _HALF, _MC = {"MCMCPP_HIP_FULL_STEP": "1"}, {"MCMCPP_HIP_FULL_STEP": "0"}, {"MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS": "0"}
_LONG_4 = [(4, 1), (2, 2), (8, 1), (4, 3), (5, 4), (12, 1), (11, 1)]
_LONG_5 = [(5, 1), (10, 1), (5, 2), (15, 1), (11, 1), (5, 3)]
_LONG_300 = [(300, 1), (3, 100), (301, 1), (4, 100), (7, 50), (600, 1)]
_LONG_128 = [(128, 1), (64, 2), (129, 1), (2, 128), (100, 2)]


def _path(family, calc, dtype, W, D, env, graph_steps, full_step, long_runs, K=1, create=None, directed=(), weights=None):
    """weights: the key of WEIGHTS the path draws from (by default its family's)"""
    return dict(family=family, calc=calc, dtype=dtype, W=W, D=D, K=K, env=env, create=create or {}, graph_steps=graph_steps,
                full_step=full_step, long_runs=long_runs, directed=tuple(directed), weights=weights or family)


PATHS = collections.OrderedDict([
    ("full_step", _path("stretch", ISO, po.F64, 70, 5, {**_FULL, "MCMCPP_HIP_GRAPH_STEPS": "4"}, 4, True, _LONG_4)),
    ("full_step_default_graphs", _path("stretch", ISO, po.F64, 70, 5, _FULL, 300, True, _LONG_300,
                                       directed=[("run", 301, 1, False, True), ("run", 299, 1, True, True)])),
    ("half_step", _path("stretch", ISO, po.F64, 70, 5, {**_HALF, "MCMCPP_HIP_GRAPH_STEPS": "4"}, 4, False, _LONG_4)),
    ("plain_launches", _path("stretch", ISO, po.F64, 70, 5, _FULL, -1, True, _LONG_4, create={"graph_steps": -1})),
    ("full_step_f32", _path("stretch", ROSENBROCK, po.F32, 70, 9, {**_FULL, "MCMCPP_HIP_GRAPH_STEPS": "4"}, 4, True, _LONG_4)),
    ("mc_full_step_batch_3", _path("stretch", DENSE, po.F64, 134, 20, {**_FULL, **_MC, "MCMCPP_HIP_GRAPH_STEPS": "5", "MCMCPP_HIP_BATCH_DRAWS": "3"},
                                   5, True, _LONG_5)),
    ("mc_full_step_batch_0", _path("stretch", DENSE, po.F64, 134, 20, {**_FULL, **_MC, "MCMCPP_HIP_GRAPH_STEPS": "5", "MCMCPP_HIP_BATCH_DRAWS": "0"},
                                   5, True, _LONG_5)),
    ("mc_half_step", _path("stretch", DENSE, po.F64, 134, 20, {**_HALF, **_MC}, 300, False, _LONG_300)),
    ("mc_half_step_16_walkers", _path("stretch", DENSE, po.F64, 134, 20, {**_HALF, **_MC, "MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS": "1",
                                                                          "MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS": "0"}, 300, False, _LONG_300)),
    ("chains3_full_step", _path("chains", DENSE, po.F64, 134, 20, {**_FULL, "MCMCPP_HIP_GRAPH_STEPS": "4"}, 4, True, _LONG_4, K=3)),
    ("chains3_half_step", _path("chains", DENSE, po.F64, 134, 20, {**_HALF, "MCMCPP_HIP_GRAPH_STEPS": "4"}, 4, False, _LONG_4, K=3)),
    ("diffevo_iso", _path("diffevo", ISO, po.F64, 30, 4, {"MCMCPP_HIP_DE_BATCH": "3"}, 128, False, _LONG_128)),
    ("diffevo_dense", _path("diffevo", DENSE, po.F64, 30, 4, {"MCMCPP_HIP_DE_BATCH": "3"}, 128, False, _LONG_128)),
    ("batch_f64", _path("batch", ISO, po.F64, 70, 5, {}, -1, False, _LONG_4)),
    ("batch_f32", _path("batch", ISO, po.F32, 70, 5, {}, -1, False, _LONG_4)),
])
OLD_PATHS = tuple(PATHS)  # the fifteen paths of the first version of this module: their sequences stay as they are, byte for byte
# The ladders: tempered handles.  K = 2 for the rounds without a pair (every odd one), K = 16 for rounds of 8 and of 7 slots.
_G4 = {"MCMCPP_HIP_GRAPH_STEPS": "4"}
PATHS.update([
    ("ladder3_full_step", _path("ladder", DENSE, po.F64, 134, 20, {**_FULL, **_G4}, 4, True, _LONG_4, K=3)),
    ("ladder3_half_step", _path("ladder", DENSE, po.F64, 134, 20, {**_HALF, **_G4}, 4, False, _LONG_4, K=3,
                                directed=[("run_tempered", 9, 3, 5, 0, "pageable")])),
    ("ladder2_full_step_f32", _path("ladder", ROSENBROCK, po.F32, 70, 9, {**_FULL, **_G4}, 4, True, _LONG_4, K=2,
                                    directed=[("run_tempered", 9, 3, 5, 1, "pinned")], weights="ladder_f32")),
    ("ladder4_plain_launches", _path("ladder", DENSE, po.F64, 134, 20, _FULL, -1, True, _LONG_4, K=4, create={"graph_steps": -1})),
    ("ladder3_default_graphs", _path("ladder", DENSE, po.F64, 134, 20, _FULL, 300, True, _LONG_300, K=3,
                                     directed=[("run_tempered", 301, 1, 150, 0, "device"), ("run", 299, 1, True, True)])),
    ("ladder16_half_step", _path("ladder", DENSE, po.F64, 70, 5, {**_HALF, **_G4}, 4, False, _LONG_4, K=16,
                                 directed=[("run_tempered", 9, 4, 7, 3, "pageable")])),
    # the stretch family's asynchronous run into device memory: a path of its own, with weights of its own
    ("full_step_device_async", _path("stretch", ISO, po.F64, 70, 5, {**_FULL, **_G4}, 4, True, _LONG_4, weights="stretch_device_async")),
])
NEW_PATHS = tuple(p for p in PATHS if p not in OLD_PATHS)
PATH_INDEX = {name: i for i, name in enumerate(PATHS)}

# The six sequences of each path: the generator seeds 0..5, but for those listed with the input condition the oracle missed
# (tests/test_call_sequences.py: no near tie, no redraw of the stretch move, proposals accepted and rejected, no exchange
# decided inside its near-tie band); each is replaced by the next integer that no sequence of the path uses.
SEEDS = {name: [0, 1, 2, 3, 4, 5] for name in PATHS}

OPS_PER_SEQUENCE = 40
DIRECTED_AFTER = 20
LONG_RUN_PROBABILITY = 0.15
BETAS = (1.0, 0.8, 0.6, 0.5, 0.35, 0.25)          # set_chain_params: chain 0's matrix times one of these
CHAINS3_START = (0, 3, 5)                          # the ladder a chains3 handle is created with (indices into BETAS)
LADDER_START = {2: (0, 3), 3: CHAINS3_START, 4: (0, 2, 3, 5)}  # the ladder a handle of K chains is created with; K = 16: geometric
EXCHANGE_ROUNDS = (0, 1, 2, 3, 4, 5, 6, 7, 2**40 - 2, 2**40 - 1)
MAX_ROUND = 2**40                                  # temper_plan.hpp refuses a run with first_round + rounds above this
SPECIAL_64 = (0, M64, 2**63, 2**63 + 1)            # handle seeds and streams: these, or 64 random bits (inc.hi = stream >> 63)

# Weights of the operation kinds while the handle is idle, per family ...
WEIGHTS = {
    "stretch": {"run": 10, "run_async": 4, "run_device": 5, "half_step_async": 5, "synchronize": 2, "seek": 4, "reset_counters": 3,
                "set_state": 3, "calc_logp": 3, "calc_logp_device": 3, "get_state": 3, "counters": 3, "refused": 3},
    "chains": {"run": 10, "run_device": 5, "seek": 4, "reset_counters": 3, "set_state": 3, "calc_logp": 3, "calc_logp_device": 2,
               "get_state": 2, "counters": 2, "refused": 2, "set_chain_params": 3, "exchange_chains": 4},
    "diffevo": {"run": 12, "run_device": 5, "set_state": 3, "reset_counters": 3, "get_state": 3, "counters": 2, "calc_logp": 3, "refused": 4},
    "batch": {"run": 12, "seek": 5, "set_state": 3, "reset_counters": 3, "get_state": 3, "counters": 2, "refused": 3},
    "ladder": {"run_tempered": 10, "run": 5, "run_device": 2.5, "run_async": 5, "run_device_async": 2.5, "evidence": 6.5, "seek": 3.5,
               "reset_counters": 4, "set_state": 2, "set_chain_params": 5, "exchange_chains": 3, "calc_logp": 2.5, "calc_logp_device": 3.5,
               "get_state": 3.5, "counters": 5, "refused": 5},
    # the fp32 ladder's own (its two chains make other sequences of the same weights: these meet its facts)
    "ladder_f32": {"run_tempered": 12, "run": 5, "run_device": 3, "run_async": 5, "run_device_async": 2.5, "evidence": 6.5, "seek": 3.5,
                   "reset_counters": 4, "set_state": 2, "set_chain_params": 4, "exchange_chains": 2.5, "calc_logp": 2.5, "calc_logp_device": 4,
                   "get_state": 4, "counters": 6, "refused": 5},
    # the stretch family's, with a third of the weight of run_async and run_device each moved to run_device_async
    "stretch_device_async": {"run": 10, "run_async": 2.5, "run_device_async": 3.5, "run_device": 3, "half_step_async": 5, "synchronize": 2, "seek": 4,
                             "reset_counters": 3, "set_state": 3, "calc_logp": 3, "calc_logp_device": 3, "get_state": 3, "counters": 3, "refused": 3},
}
# ... while an ensemble step is half done (half_step_async(0) went out) ...
WEIGHTS_HALF_DONE = {"half_step_async": 8, "synchronize": 1, "get_state": 1, "counters": 1, "calc_logp": 1, "refused": 2, "set_state": 0.5,
                     "reset_counters": 0.5}
# ... and while an asynchronous run is in flight (run_wait: before / after the first wait_stored)
WEIGHTS_IN_FLIGHT = {"refused_in_flight": 2, "wait_stored": 3, "run_wait": (0.5, 4)}
WEIGHTS_IN_FLIGHT_LADDER = {"refused_in_flight": 6, "wait_stored": 3, "run_wait": (0.5, 4)}
# What the last state-changing operation multiplies: a run that left an odd step count, a seek, a reset behind a run
FOLLOW = {
    "odd_run": {"run_device": 3, "half_step_async": 3, "set_state": 2, "reset_counters": 2},
    "seek": {"run": 3, "run_async": 2},
    "reset_after_run": {"run": 6},
}
# ... and on a ladder: the hand-overs into and out of a tempered run (a run_tempered behind a tempered run also takes the round
# number that one returned as its first_round, CARRY_ROUND_PROBABILITY of the time)
FOLLOW_LADDER = {
    "odd_tempered": {"run": 9, "run_device": 14.5, "exchange_chains": 10, "set_state": 3.5, "get_state": 5.5},
    "tempered": {"run_tempered": 3.5},
    "odd_run": {"run_tempered": 2.5, "run_device": 2.5, "set_state": 3, "reset_counters": 2},
    "seek": {"run_tempered": 6, "run": 1.5},
    "set_chain_params": {"run_tempered": 5.5, "evidence": 6},
    "reset_counters": {"run_tempered": 6},
    "reset_after_run": {"run_tempered": 2, "run": 6},
    "exchange_chains": {"run_tempered": 7},
}
CARRY_ROUND_PROBABILITY = 0.6
REFUSED = {"stretch": ("run_negative", "run_interval_0", "half_step_out_of_order"), "chains": ("run_negative", "run_interval_0"),
           "diffevo": ("run_negative", "run_interval_0", "seek_unsupported"), "batch": ("run_negative", "run_interval_0"),
           "ladder": ("run_negative", "run_interval_0", "run_tempered_every_0", "run_tempered_round_out_of_range", "half_step_async")}
REFUSED_CODE = {"run_negative": E_ARG, "run_interval_0": E_ARG, "half_step_out_of_order": E_ARG, "seek_unsupported": E_UNSUPPORTED,
                "run_tempered_every_0": E_ARG, "run_tempered_round_out_of_range": E_ARG, "half_step_async": E_UNSUPPORTED}
ROUND_OUT_OF_RANGE = (2, 1, 1, 2**40 - 1)          # the run_tempered of a drawn ("refused", "run_tempered_round_out_of_range"): two rounds
REFUSED_IN_FLIGHT = {"stretch": ("seek", "calc_logp", "get_state"),
                     "ladder": ("seek", "calc_logp", "get_state") + 2 * ("run_tempered", "exchange_chains", "set_chain_params", "evidence")}
LADDER_CALLS = ("run_tempered", "exchange_chains", "set_chain_params", "evidence")
RUN_KINDS = ("run", "run_async", "run_device", "run_device_async")
ASYNC_KINDS = ("run_async", "run_device_async")
STATE_CHANGING = RUN_KINDS + ("half_step_async", "seek", "reset_counters", "set_state", "set_chain_params", "exchange_chains", "run_tempered")
DELIVERIES = ("pageable", "pinned", "device")
EVIDENCE_KINDS = ("ratios", "bridge", "mbar")      # (K = 16: the first two; the joint solve of 16 rungs is tests/test_evidence_mbar.py's)
EVIDENCE_PLACES = ("host", "device")
EXCHANGE_EVERY = (1, 2, 3, 4, 5, 7)                # and the run's length, and one more; 300 steps a replay: EXCHANGE_EVERY_300 too
EXCHANGE_EVERY_300 = (100, 150, 300, 301)


def seek_targets(cfg, step, rng):
    """0, where the handle stands, a small step, the steps whose first draw (index 6 n s: 3 draws per walker, 2 n walkers
    per step) lies just below and just above 2^32, and 2^40"""
    below = (2**32 - 1) // (6 * (cfg["W"] // 2))
    return (0, step, 1 + int(rng.integers(0, 50)), below, below + 1, 2**40)


# ---- the generator ------------------------------------------------------------------------------------------------------------

def _pick(rng, weights):
    """one key of an ordered {key: weight}, by rng.random() alone"""
    keys = [k for k, w in weights.items() if w > 0]
    total = float(sum(weights[k] for k in keys))
    x, acc = rng.random() * total, 0.0
    for k in keys:
        acc += weights[k]
        if x < acc:
            return k
    return keys[-1]


def _special_64(rng):
    i = int(rng.integers(0, 6))
    bits = int(rng.integers(0, 2**63)) * 2 + int(rng.integers(0, 2))
    return SPECIAL_64[i] if i < 4 else bits


def _run_shape(rng, cfg):
    if rng.random() < LONG_RUN_PROBABILITY:
        return cfg["long_runs"][int(rng.integers(0, len(cfg["long_runs"])))]
    return int(rng.integers(0, 10)), int(rng.integers(1, 5))


def plan(path, seed):
    """(handle seed, handle stream, operations) of sequence `seed` of `path`"""
    cfg = PATHS[path]
    fam = cfg["family"]
    ladder = fam == "ladder"
    rng = np.random.default_rng((PATH_INDEX[path], seed))
    handle_seed, stream = _special_64(rng), _special_64(rng)
    ops = [("set_state", int(rng.integers(0, 1000)))]
    # the generator's own view of the handle: enough to tell a legal operation from an illegal one
    step, half_done, in_flight, waited, context = 0, False, None, False, None
    next_round = None  # the round the last tempered run returned, while nothing has changed the state behind it
    evidence_at = refused_at = seed
    drawn, directed = 0, list(cfg["directed"])
    while drawn < OPS_PER_SEQUENCE or in_flight is not None:
        if directed and drawn >= DIRECTED_AFTER and not half_done and in_flight is None:
            for op in directed:
                ops.append(op)
                step += op[1] * op[2]
            context, next_round = "odd_run" if sum(op[1] * op[2] for op in directed) & 1 else None, None
            if directed[-1][0] == "run_tempered":
                op = directed[-1]
                context, next_round = "odd_tempered" if (op[1] * op[2]) & 1 else "tempered", op[4] + op[1] * op[2] // op[3]
            directed = []
            continue
        left = OPS_PER_SEQUENCE - drawn
        if in_flight is not None:
            w = dict(WEIGHTS_IN_FLIGHT_LADDER if ladder else WEIGHTS_IN_FLIGHT)
            w["run_wait"] = w["run_wait"][1 if waited else 0]
            kind = "run_wait" if left <= 1 else _pick(rng, w)
        elif half_done:
            kind = _pick(rng, WEIGHTS_HALF_DONE)
        else:
            w = dict(WEIGHTS[cfg["weights"]])
            for k, f in (FOLLOW_LADDER if ladder else FOLLOW).get(context, {}).items():
                if k in w:
                    w[k] *= f
            if left < 3:
                for k in ASYNC_KINDS:
                    w.pop(k, None)  # (an operation that would be illegal is not drawn: the run could not be waited for)
            kind = _pick(rng, w)
        drawn += 1
        if kind in RUN_KINDS:
            n_saved, interval = _run_shape(rng, cfg)
            flags = (bool(rng.random() < 0.75), bool(rng.random() < 0.75))
            if kind == "run":
                ops.append(("run", n_saved, interval) + flags)
            else:
                ops.append((kind, n_saved, interval, flags[1]))
            if kind in ASYNC_KINDS:
                in_flight, waited = n_saved, False
            step += n_saved * interval
            if n_saved > 0:
                context, next_round = "odd_run" if (n_saved * interval) & 1 else "run", None
        elif kind == "run_tempered":
            n_saved, interval = _run_shape(rng, cfg)
            total = n_saved * interval
            every = EXCHANGE_EVERY + (max(total, 1), total + 1) + (EXCHANGE_EVERY_300 if cfg["graph_steps"] == 300 else ())
            every = every[int(rng.integers(0, len(every)))]
            first = EXCHANGE_ROUNDS[int(rng.integers(0, len(EXCHANGE_ROUNDS)))]
            if next_round is not None and rng.random() < CARRY_ROUND_PROBABILITY:
                first = next_round
            delivery = DELIVERIES[int(rng.integers(0, len(DELIVERIES)))]
            if first + total // every > MAX_ROUND:
                ops.append(("refused", "run_tempered_round_out_of_range", n_saved, interval, every, first))
            else:
                ops.append((kind, n_saved, interval, every, first, delivery))
                step += total
                if total > 0:
                    context, next_round = "odd_tempered" if total & 1 else "tempered", first + total // every
        elif kind == "evidence":
            # (which, place) in rotation, sequence `seed` beginning at pair `seed`: the six sequences meet every pair
            pairs = [(which, place) for which in EVIDENCE_KINDS[:2 if cfg["K"] > 4 else 3] for place in EVIDENCE_PLACES]
            which, place = pairs[evidence_at % len(pairs)]
            evidence_at += 1
            ops.append((kind, which, int(rng.integers(4, 9)), int(rng.integers(0, 2**31)), place))
        elif kind == "refused_in_flight":
            names = REFUSED_IN_FLIGHT[fam]
            ops.append((kind, names[int(rng.integers(0, len(names)))]))
        elif kind == "wait_stored":
            ops.append((kind, int(rng.integers(0, in_flight + 1))))
            waited = True
        elif kind == "run_wait":
            ops.append((kind,))
            in_flight = None
        elif kind == "half_step_async":
            ops.append((kind, 1 if half_done else 0))
            if half_done:
                step += 1
            half_done = not half_done
            context = None
        elif kind == "seek":
            targets = seek_targets(cfg, step, rng)
            step = targets[int(rng.integers(0, len(targets)))]
            ops.append((kind, step))
            context, next_round = "seek", None
        elif kind == "reset_counters":
            ops.append((kind,))
            context = "reset_after_run" if context in ("run", "odd_run") else "reset_counters" if ladder else None
        elif kind == "set_state":
            ops.append((kind, int(rng.integers(0, 1000))))
            step, half_done, context, next_round = 0, False, None, None
        elif kind in ("calc_logp", "calc_logp_device"):
            count, rows_seed = int(rng.integers(1, 21)), int(rng.integers(0, 2**31))
            chain = None
            if fam in ("chains", "ladder"):
                chain = int(rng.integers(0, cfg["K"] + (1 if kind == "calc_logp" else 0)))
                chain = None if chain == cfg["K"] else chain
            ops.append((kind, count, rows_seed, 0 if kind == "calc_logp_device" and chain is None else chain))
        elif kind == "refused":
            names = REFUSED[fam]
            if half_done:
                names = ("half_step_out_of_order", "half_step_out_of_order") + names
            if ladder:  # (in rotation, sequence `seed` beginning at name `seed`: the six sequences meet every name)
                what, refused_at = names[refused_at % len(names)], refused_at + 1
            else:
                what = names[int(rng.integers(0, len(names)))]
            ops.append((kind, what) + (ROUND_OUT_OF_RANGE if what == "run_tempered_round_out_of_range" else ()))
        elif kind == "set_chain_params":
            ops.append((kind, int(rng.integers(0, cfg["K"])), int(rng.integers(0, len(BETAS)))))
            context, next_round = kind if ladder else None, None
        elif kind == "exchange_chains":
            ops.append((kind, EXCHANGE_ROUNDS[int(rng.integers(0, len(EXCHANGE_ROUNDS)))]))
            context, next_round = kind if ladder else None, None
        else:
            ops.append((kind,))  # synchronize, get_state, counters
    return handle_seed, stream, ops


def generate(path, seed):
    return plan(path, seed)[2]


def render(ops):
    return "\n".join("%3d %r" % (i, op) for i, op in enumerate(ops))


def digest(paths=None):
    """SHA-256 over every (path, seed) of SEEDS (paths: of these paths, in this order): the handle's seed and stream and the
    rendered operations"""
    h = hashlib.sha256()
    for path in PATHS if paths is None else paths:
        for seed in SEEDS[path]:
            handle_seed, stream, ops = plan(path, seed)
            h.update(("%s %d %d %d\n%s\n" % (path, seed, handle_seed, stream, render(ops))).encode())
    return h.hexdigest()


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def base_params(cfg):
    t = po.np_dtype(cfg["dtype"])
    if cfg["calc"] == DENSE:
        D = cfg["D"]
        a = np.random.default_rng(cfg["W"] + D).standard_normal((D, D))
        return (a @ a.T / D + np.eye(D)).astype(t).ravel()
    if cfg["calc"] == ROSENBROCK:
        return np.array([1.0, 100.0, 0.05], dtype=t)
    return None


def params_at(cfg, beta):
    """chain 0's parameters flattened by beta: the dense matrix times beta; Rosenbrock: its third parameter times beta"""
    t = po.np_dtype(cfg["dtype"])
    if cfg["calc"] == ROSENBROCK:
        p = base_params(cfg).astype(np.float64)
        p[2] *= beta
        return p.astype(t)
    return (beta * base_params(cfg)).astype(t)


def chain_params(cfg, beta_index):
    return params_at(cfg, BETAS[beta_index])


def start_betas(cfg):
    """the betas a handle of several chains is created with: spread over BETAS; K = 16: a geometric ladder from 1 down to 0.25"""
    K = cfg["K"]
    if K in LADDER_START:
        return [BETAS[i] for i in LADDER_START[K]]
    return [float(0.25 ** (k / (K - 1.0))) for k in range(K)]


def evidence_draws(cfg, betas, n, rows_seed):
    """the draws [K][n][W][D] of an evidence operation, from rows_seed alone (tests/evidence_device.make_draws): Gaussian, chain
    k's wider by 1 / sqrt of its beta"""
    from tests import evidence_device as ed
    return ed.make_draws(dict(dtype="f32" if cfg["dtype"] == po.F32 else "f64", calc="rosen" if cfg["calc"] == ROSENBROCK else "dense", K=cfg["K"], n=n,
                              W=cfg["W"], D=cfg["D"], seed=rows_seed, betas=list(betas)))


def rows_for(cfg, count, rows_seed):
    return (np.random.default_rng(rows_seed).standard_normal((count, cfg["D"])) * 1.5).astype(po.np_dtype(cfg["dtype"]))


# ---- how a run is cut into launches: run_plan.hpp and enqueue_steps restated, for the coverage facts only ------------------------

SUBCHUNK_BYTES = 32 << 20


def launch_chunks(cfg, n_saved, interval, save_chain, to_device, pinned=False):
    """the step counts a run hands to enqueue_steps, in order (pinned: plan_chain's `direct`)"""
    total = n_saved * interval
    if total == 0:
        return []
    G = cfg["graph_steps"]
    step_bytes = cfg["W"] * cfg["D"] * (8 if cfg["dtype"] == po.F64 else 4)
    if cfg["family"] in ("diffevo", "batch") or not save_chain:
        return [total]
    if to_device or (cfg["full_step"] and step_bytes % 16 == 0):
        per = (G if G > 0 else 64) // interval
        if not to_device and not pinned:
            ring = 4
            while ring < 64 and 2 * ring * step_bytes <= 2 * SUBCHUNK_BYTES:
                ring *= 2
            per = min(per, (ring - 2) // 2)
        chunk, out, done = max(per, 1) * interval, [], 0
        while done < total:
            now = min(total - done, chunk)
            if not to_device and not pinned and now == total - done and now > interval:
                now -= interval  # (the trickle window ends a run with a chunk of one interval)
            out.append(now)
            done += now
        return out
    sub = max(1, min(SUBCHUNK_BYTES // (step_bytes * cfg["K"]), (n_saved + 7) // 8))
    return [min(sub, n_saved - first) * interval for first in range(0, n_saved, sub)]


def replays(cfg, chunks):
    """(steps into the run at the head, length) of every graph replay -- of every launch where there are no graphs"""
    G, out, at = cfg["graph_steps"], [], 0
    for c in chunks:
        left = c
        while left > 0:
            now = 1 if G < 1 else min(left, G)
            out.append((at, now))
            at += now
            left -= now
    return out


# ---- the model ----------------------------------------------------------------------------------------------------------------

class Model:
    """What a handle of `path` created with (handle_seed, stream) must return, operation by operation."""

    def __init__(self, path, handle_seed, stream):
        self.path, self.cfg, self.seed, self.stream = path, PATHS[path], handle_seed, stream
        cfg = self.cfg
        self.K, self.W, self.D = cfg["K"], cfg["W"], cfg["D"]
        self.mover = DE if cfg["family"] == "diffevo" else STRETCH
        self.betas = start_betas(cfg) if self.K > 1 else [1.0]  # what set_chain_params installed last, chain by chain
        self.params = [params_at(cfg, b) for b in self.betas] if self.K > 1 else [base_params(cfg)]
        self.orcs = [self._oracle(k) for k in range(self.K)]
        self.nacc_off = [np.zeros(self.W, np.int64) for _ in range(self.K)]  # get_state's counts = the oracle's + these
        self.ties_off = self.redraws_off = 0
        self.step = 0                # ensemble steps done since set_state, or where the last seek put the handle
        self.steps_since_reset = 0
        self.half_done = False
        self.pending = None          # the result of the asynchronous run in flight
        # for the CPU tests
        self.facts, self.kinds = set(), collections.Counter()
        self.accepted = self.proposed = self.in_band = 0
        self._last_change, self._prev_op = None, None  # the last state-changing operation, the last operation
        self._reset_behind_run = self._pair_after_odd_run = False
        self._in_flight_refusals, self._in_flight_ladder_calls, self._in_flight_device = 0, 0, False
        # the rounds of a ladder, inside tempered runs and between runs: swaps accepted and refused; the evidence operations
        self.swaps_accepted = self.swaps_refused = 0
        self.evidence_nonfinite = self.evidence_unconverged = 0
        self._next_round = None  # the round the last tempered run returned (while it is the last state-changing operation)

    def _oracle(self, k):
        return po.Oracle(self.W, self.D, self.cfg["calc"], self.params[k], seed=(self.seed + k) & M64, stream=self.stream,
                         dtype=self.cfg["dtype"], mover=self.mover)

    # -- what get_state and counters must return
    def state(self):
        s = [o.get_state() for o in self.orcs]
        nacc = [(x[2].astype(np.int64) + off).astype(np.uint32) for x, off in zip(s, self.nacc_off)]
        pos, logp = [x[0] for x in s], [x[1] for x in s]
        if self.K == 1:
            return pos[0], logp[0], nacc[0]
        return np.stack(pos), np.stack(logp), np.stack(nacc)

    def counters(self):
        return dict(accepted=int(sum(int(a.sum()) for a in np.atleast_2d(self.state()[2]))), ensemble_steps=self.steps_since_reset,
                    near_ties=self.near_ties, redraws=self.redraws)

    @property
    def near_ties(self):
        return self.ties_off + sum(o.near_ties for o in self.orcs)

    @property
    def redraws(self):
        return self.redraws_off + sum(o.redraws for o in self.orcs)

    # -- the operations
    def apply(self, op):
        kind = op[0]
        self.kinds[kind] += 1
        if self._prev_op and self._prev_op[0] == "evidence" and self._last_change is not None and kind in STATE_CHANGING:
            self.facts.add("an evidence call between two state-changing operations")
        out = getattr(self, "_" + kind)(*op[1:])
        if kind in STATE_CHANGING:
            self._last_change = op
        self._prev_op = op
        return out

    def _last_was_run(self, odd=False):
        last = self._last_change
        return bool(last and last[0] in RUN_KINDS and last[1] * last[2] > 0 and (not odd or (last[1] * last[2]) & 1))

    def _set_state(self, salt):
        if self.step & 1:
            self.facts.add("set_state after an odd number of steps")
        for k, o in enumerate(self.orcs):
            pos = po.init_positions(self.cfg["dtype"], self.W, self.D, salt=salt + k)
            o.set_state(pos, o.logp(pos))
            self.nacc_off[k][:] = 0
        self.ties_off = self.redraws_off = 0
        self.step = self.steps_since_reset = 0
        self.half_done = False

    def start_state(self, salt):
        """the arrays ("set_state", salt) uploads"""
        pos = [po.init_positions(self.cfg["dtype"], self.W, self.D, salt=salt + k) for k in range(self.K)]
        logp = [o.logp(p) for o, p in zip(self.orcs, pos)]
        return (pos[0], logp[0]) if self.K == 1 else (np.stack(pos), np.stack(logp))

    def _steps(self, n_saved, interval, save_chain, want_accepted, to_device=False, kind="run"):
        self._note_run(n_saved, interval, save_chain, to_device, kind)
        mode = po.MODE_SEQUENTIAL if self.mover == DE else po.MODE_COUNTER
        r = [o.run(n_saved, interval=interval, save_chain=save_chain, mode=mode) for o in self.orcs]
        total = n_saved * interval
        self.step += total
        self.steps_since_reset += total
        self.accepted += sum(int(a.sum()) for _, a in r)
        self.proposed += self.W * total * self.K
        chain = None if not save_chain else (r[0][0] if self.K == 1 else np.stack([c for c, _ in r]))
        acc = None if not want_accepted else (r[0][1] if self.K == 1 else np.stack([a for _, a in r]))
        return chain, acc

    def _run(self, n_saved, interval, save_chain, want_accepted):
        return self._steps(n_saved, interval, save_chain, want_accepted)

    def _run_device(self, n_saved, interval, want_accepted):
        return self._steps(n_saved, interval, True, want_accepted, to_device=True, kind="run_device")

    def _run_async(self, n_saved, interval, want_accepted, to_device=False):
        self.pending = self._steps(n_saved, interval, True, want_accepted, to_device=to_device, kind="run_device_async" if to_device else "run_async")
        self._in_flight_refusals, self._in_flight_ladder_calls, self._in_flight_device = 0, 0, to_device

    def _run_device_async(self, n_saved, interval, want_accepted):
        self._run_async(n_saved, interval, want_accepted, to_device=True)

    def _refused_in_flight(self, what):
        self._in_flight_refusals += 1
        self._in_flight_ladder_calls += what in LADDER_CALLS
        return E_STATE

    def _wait_stored(self, k):
        return self.pending[0][:k] if self.K == 1 else self.pending[0][:, :k]

    def _run_wait(self):
        out, self.pending = self.pending, None
        if self._in_flight_refusals:
            self.facts.add("an asynchronous run with a refused call inside it")
            if self._in_flight_device:
                self.facts.add("an asynchronous run into device memory with a refused call inside it")
        if self._in_flight_ladder_calls:
            self.facts.add("an asynchronous %s run with a refused ladder call inside it" % ("device" if self._in_flight_device else "host"))
        return out

    def _half_step_async(self, colour):
        assert colour == (1 if self.half_done else 0) and self.K == 1
        if colour == 0:
            self._pair_after_odd_run = self._last_was_run(odd=True) and self.cfg["full_step"]
        o = self.orcs[0]
        self.accepted += o.half_step_shard(colour, 0, self.W // 2)
        self.proposed += self.W // 2
        o.half_step_commit()
        self.half_done = colour == 0
        if colour == 1:
            self.step += 1
            self.steps_since_reset += 1
            if self._pair_after_odd_run:
                self.facts.add("a half-step pair after an odd full-step run")

    def _synchronize(self):
        return None

    def _seek(self, step):
        assert not self.half_done
        for o in self.orcs:
            o.seek(step)
        self.step = step

    def _reset_counters(self):
        self._reset_behind_run = self._last_was_run()
        for k, o in enumerate(self.orcs):
            self.nacc_off[k] = -o.get_state()[2].astype(np.int64)
        self.steps_since_reset = 0
        return self.counters()

    def _get_state(self):
        return self.state()

    def _counters(self):
        return self.counters()

    def _calc_logp(self, count, rows_seed, chain):
        return self.orcs[chain or 0].logp(rows_for(self.cfg, count, rows_seed))

    _calc_logp_device = _calc_logp

    def _refused(self, what, *args):
        self.facts.add("a refused " + what)
        return REFUSED_CODE[what]

    def _set_chain_params(self, chain, beta_index):
        old = self.orcs[chain]
        pos, logp, nacc = old.get_state()
        self.nacc_off[chain] = self.nacc_off[chain] + nacc.astype(np.int64)
        self.ties_off += old.near_ties
        self.redraws_off += old.redraws
        self.betas[chain] = BETAS[beta_index]
        self.params[chain] = chain_params(self.cfg, beta_index)
        new = self._oracle(chain)
        new.set_state(pos, logp)  # (the stored log-posteriors are not recomputed, by the library either)
        new.seek(self.step)
        self.orcs[chain] = new

    def _exchange_chains(self, rnd):
        pos, logp = [o.positions_view() for o in self.orcs], [o.logp_view() for o in self.orcs]
        P, L = np.stack(pos), np.stack(logp)
        out = rr.exchange_arrays(P, L, lambda k, rows: self.orcs[k].logp(rows), rnd, self.seed, self.stream)
        for k in range(self.K):
            pos[k][...] = P[k]
            logp[k][...] = L[k]
        self.in_band += len(out["in_band"])
        self.swaps_accepted += int(out["accepted"].sum())
        self.swaps_refused += int(out["proposed"].sum()) - int(out["accepted"].sum())
        if self._prev_op and self._prev_op[0] == "run_tempered" and (self._prev_op[1] * self._prev_op[2]) & 1:
            self.facts.add("exchange_chains directly behind a tempered run that ended at an odd step")
        return dict(proposed=out["proposed"], accepted=out["accepted"], near_ties=out["near_ties"])

    def _run_tempered(self, n_saved, interval, every, first_round, delivery):
        """Ladder.run_exchanging's rule on the model's own oracles: steps with interval 1 in pieces that end at the multiples of
        `every` counted from the start of the run, a round behind each such piece (none behind a shorter tail), every interval-th
        step kept"""
        total, K = n_saved * interval, self.K
        self._note_tempered(n_saved, interval, every, first_round, delivery)
        chains, accs = [[] for _ in range(K)], [[] for _ in range(K)]
        swaps = dict(proposed=np.zeros(K - 1, np.uint64), accepted=np.zeros(K - 1, np.uint64), near_ties=np.zeros(K - 1, np.uint64))
        done, rnd, start, prev = 0, first_round, self.step, self._prev_op
        self._prev_op = None  # (the rounds inside the run are not "directly behind" the operation in front of it)
        while done < total:
            piece = min(every - done % every, total - done)
            for k, o in enumerate(self.orcs):
                c, a = o.run(piece, interval=1, save_chain=True, mode=po.MODE_COUNTER)
                chains[k].append(c)
                accs[k].append(a)
                self.accepted += int(a.sum())
            done += piece
            if done % every == 0:
                if self.cfg["full_step"]:
                    self.facts.add("a round that finds the ensemble %s" % ("in the second buffer" if done & 1 else "at home"))
                self.facts.add("a round at record-buffer parity %d" % ((start + done) & 1))
                if not rr.pairs_of(K, rnd):
                    self.facts.add("a round without a pair inside a tempered run")
                r = self._exchange_chains(rnd)
                for key in swaps:
                    swaps[key] += r[key]
                rnd += 1
        self._prev_op = prev
        self.step += total
        self.steps_since_reset += total
        self.proposed += self.W * total * K
        t = po.np_dtype(self.cfg["dtype"])
        chain = np.stack([np.concatenate(c)[interval - 1::interval] if c else np.empty((0, self.W, self.D), t) for c in chains])
        acc = np.stack([np.concatenate(a) if a else np.zeros(0, np.uint32) for a in accs])
        self._next_round = rnd
        return chain, acc, swaps, rnd

    def _evidence(self, which, n, rows_seed, place):
        """the restatements on the model's own log-posteriors of the draws, under the parameters set_chain_params installed last"""
        from tests import bridge_restatement, evidence_restatement, mbar_restatement
        K, W = self.K, self.W
        x = evidence_draws(self.cfg, self.betas, n, rows_seed)
        if self._prev_op and self._prev_op[0] == "set_chain_params":
            self.facts.add("an evidence call directly behind set_chain_params")
        self.facts.add("evidence %s from %s memory" % (which, place))
        lp = lambda k, r: self.orcs[k].logp(x[r]).reshape(n, W)  # noqa: E731  (chain k's log-posteriors of the draws of rung r)
        if which == "mbar":
            out = mbar_restatement.mbar(mbar_restatement.from_logp(np.stack([np.stack([lp(k, r) for r in range(K)]) for k in range(K)])), n, W)
        else:
            own = np.stack([lp(k, k) for k in range(K)])
            lower = np.stack([lp(k - 1, k) if k > 0 else np.zeros_like(own[0]) for k in range(K)])
            upper = np.stack([lp(k + 1, k) if k + 1 < K else np.zeros_like(own[0]) for k in range(K)])
            out = (evidence_restatement.evidence_ratios if which == "ratios" else bridge_restatement.evidence_bridge)(own, lower, upper)
        self.evidence_nonfinite += int(np.asarray(out["nonfinite"]).sum())
        if which != "ratios":
            self.evidence_unconverged += int((np.atleast_1d(out["converged"]) != 1).sum())
        return evidence_result(which, out)

    # -- coverage facts of a run, from the model's own numbers
    def _note_run(self, n_saved, interval, save_chain, to_device, kind):
        total, cfg, f = n_saved * interval, self.cfg, self.facts
        if total == 0:
            f.add("a zero-step run")
            return
        f.add("a run that begins at odd steps-since-origin" if self.step & 1 else "a run that begins at even steps-since-origin")
        if self._prev_op and self._prev_op[0] == "seek":
            f.add("seek directly followed by run")
        if self._last_change and self._last_change[0] == "reset_counters" and self._reset_behind_run:
            f.add("reset_counters between two runs")
        if to_device and self._last_was_run(odd=True):
            f.add("run_device after an odd run")
        if kind in ("run", "run_device") and self._prev_op and self._prev_op[0] == "run_tempered" and (self._prev_op[1] * self._prev_op[2]) & 1:
            f.add("%s directly behind a tempered run that ended at an odd step" % kind)
        heads = replays(cfg, launch_chunks(cfg, n_saved, interval, save_chain, to_device))
        if cfg["full_step"]:
            for at, _ in heads:
                f.add("a replay head with start parity %d, position parity %d" % ((self.step + at) & 1, at & 1))
        G = cfg["graph_steps"]
        if G >= 1:
            whole, rest = any(n == G for _, n in heads), any(n < G for _, n in heads)
            f.add("a run made of whole replays only" if whole and not rest else
                  "a run made of a remainder only" if rest and not whole else "a run made of whole replays and remainders")

    def _note_tempered(self, n_saved, interval, every, first_round, delivery):
        total, cfg, f, prev, last = n_saved * interval, self.cfg, self.facts, self._prev_op, self._last_change
        if total == 0:
            f.add("a zero-step tempered run")
            return
        rounds = total // every
        f.add("a tempered run that begins at %s steps-since-origin" % ("odd" if self.step & 1 else "even"))
        f.add("a tempered run delivered %s" % delivery)
        if rounds and every % interval:
            f.add("a tempered run whose exchange_every is no multiple of its interval")
        f.add("a tempered run without any round" if not rounds else "a tempered run that ends on an exchange point" if total % every == 0 else
              "a tempered run with a tail shorter than exchange_every")
        if rounds >= 2 and self.K == 16:
            f.add("a tempered run with both an 8-slot and a 7-slot round")
        if prev and prev[0] in ("seek", "set_chain_params", "reset_counters", "exchange_chains"):
            f.add("run_tempered directly behind " + prev[0])
        if self._last_was_run(odd=True):
            f.add("run_tempered behind an odd plain run")
        if last and last[0] == "run_tempered" and last[1] * last[2] >= last[3] and rounds and first_round == self._next_round:
            f.add("two tempered runs with the round number carried over")
        # the launches: the run's chunks (launch_chunks), each cut at the exchange points
        G, at = cfg["graph_steps"], 0
        for c in launch_chunks(cfg, n_saved, interval, True, delivery == "device", pinned=delivery == "pinned"):
            end = at + c
            while at < end:
                piece = min(every - at % every, end - at)
                at += piece
                if G >= 1 and piece < G:
                    f.add("a tempered piece shorter than a replay")
                if G >= 1 and piece > G and piece % G:
                    f.add("a tempered piece made of whole replays and a remainder")


# ---- what the sequences of a path must show, and what an evidence operation is compared on ------------------------------------------

# a chunk of a run is longer than a replay only where the stored steps leave through sub-chunks (half-step kernels, or a stored
# step that is no multiple of 16 bytes): elsewhere no piece of a tempered run is
def subchunk_delivery(cfg):
    return not cfg["full_step"] or (cfg["W"] * cfg["D"] * (8 if cfg["dtype"] == po.F64 else 4)) % 16 != 0


def facts_wanted_ladder(path):
    """what a ladder path must show on top of the facts of every multi-chain path"""
    cfg = PATHS[path]
    want = {"a tempered run that begins at odd steps-since-origin", "a tempered run that begins at even steps-since-origin",
            "a round at record-buffer parity 0", "a round at record-buffer parity 1",
            "a tempered run whose exchange_every is no multiple of its interval", "a tempered run that ends on an exchange point",
            "a tempered run with a tail shorter than exchange_every", "a tempered run without any round", "a zero-step tempered run",
            "run_tempered directly behind seek", "run_tempered directly behind set_chain_params", "run_tempered directly behind reset_counters",
            "run_tempered directly behind exchange_chains", "run_tempered behind an odd plain run",
            "run directly behind a tempered run that ended at an odd step", "run_device directly behind a tempered run that ended at an odd step",
            "exchange_chains directly behind a tempered run that ended at an odd step", "two tempered runs with the round number carried over",
            "an evidence call between two state-changing operations", "an evidence call directly behind set_chain_params",
            "an asynchronous host run with a refused ladder call inside it", "an asynchronous device run with a refused ladder call inside it"}
    want |= {"a refused " + name for name in REFUSED["ladder"]}
    want |= {"a tempered run delivered " + d for d in DELIVERIES}
    want |= {"evidence %s from %s memory" % (w, p) for w in EVIDENCE_KINDS[:2 if cfg["K"] > 4 else 3] for p in EVIDENCE_PLACES}
    if cfg["full_step"]:
        want |= {"a round that finds the ensemble in the second buffer", "a round that finds the ensemble at home"}
    if cfg["graph_steps"] >= 1:
        want.add("a tempered piece shorter than a replay")
        if subchunk_delivery(cfg):
            want.add("a tempered piece made of whole replays and a remainder")
    if cfg["K"] == 2:
        want.add("a round without a pair inside a tempered run")
    if cfg["K"] == 16:
        want.add("a tempered run with both an 8-slot and a 7-slot round")
    return want


def evidence_result(which, out):
    """what an evidence operation is compared on: every key the GPU tests of tests/test_evidence.py, test_evidence_bridge.py and
    test_evidence_mbar.py compare, each as an array of at least one dimension"""
    from tests import bridge_device, evidence_device, mbar_device
    keys = {"ratios": evidence_device.KEYS, "bridge": bridge_device.KEYS, "mbar": mbar_device.KEYS}[which] + ("num_draws",)
    return {key: np.atleast_1d(np.asarray(out[key])) for key in keys}


def facts_wanted(path):
    """the coverage facts the six sequences of a path must show between them"""
    cfg = PATHS[path]
    fam = cfg["family"]
    want = {"a run that begins at even steps-since-origin", "a zero-step run", "set_state after an odd number of steps",
            "reset_counters between two runs", "a run that begins at odd steps-since-origin"}
    if fam == "ladder":
        # On top of the facts of every path that hold for a plain run and a tempered run alike.  Left out on purpose: what is about
        # the launches of plain runs alone (replay heads, whole replays and remainders, run_device after an odd run, a seek or a
        # reset in front of a plain run) -- the chains3 paths show them on handles of several chains, the ladders ask for the same
        # hand-overs into a tempered run, and 40 operations of which a quarter are plain runs cannot show both sets.
        return (want - {"reset_counters between two runs"}) | facts_wanted_ladder(path)
    if cfg["full_step"]:
        want |= {"a replay head with start parity %d, position parity %d" % (a, b) for a in (0, 1) for b in (0, 1)}
    if cfg["graph_steps"] >= 1:
        want |= {"a run made of whole replays only", "a run made of a remainder only", "a run made of whole replays and remainders"}
    if fam in ("stretch", "chains", "batch"):
        want.add("seek directly followed by run")
    if fam != "batch":
        want.add("run_device after an odd run")
    if fam == "stretch":
        want.add("an asynchronous run with a refused call inside it")
        if "run_device_async" in WEIGHTS[cfg["weights"]]:
            want.add("an asynchronous run into device memory with a refused call inside it")
        if cfg["full_step"]:
            want.add("a half-step pair after an odd full-step run")
    return want


def kinds_of(path):
    fam = PATHS[path]["family"]
    kinds = set(WEIGHTS[PATHS[path]["weights"]]) | {"set_state"}
    if fam in ("stretch", "ladder"):
        kinds |= {"refused_in_flight", "wait_stored", "run_wait"}
    return kinds


def model_run(path, seed):
    """the whole sequence on the model alone: (model, [expected result of every operation])"""
    handle_seed, stream, ops = plan(path, seed)
    model = Model(path, handle_seed, stream)
    return model, [model.apply(op) for op in ops]


# ---- comparison ---------------------------------------------------------------------------------------------------------------

def differs(got, want, what=""):
    """None when got equals want bit for bit (arrays: shape, dtype and bytes), else a line that says where they part"""
    if isinstance(want, dict):
        if not isinstance(got, dict) or set(got) != set(want):
            return "%s: keys %r, expected %r" % (what, sorted(got) if isinstance(got, dict) else got, sorted(want))
        for k in sorted(want):
            d = differs(got[k], want[k], "%s[%r]" % (what, k))
            if d:
                return d
        return None
    if isinstance(want, (tuple, list)):
        if not isinstance(got, (tuple, list)) or len(got) != len(want):
            return "%s: %r, expected a sequence of %d" % (what, type(got).__name__, len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            d = differs(g, w, "%s[%d]" % (what, i))
            if d:
                return d
        return None
    if isinstance(want, np.ndarray):
        if not isinstance(got, np.ndarray) or got.shape != want.shape or got.dtype != want.dtype:
            return "%s: %s, expected an array %s of %s" % (what, (got.shape, got.dtype) if isinstance(got, np.ndarray) else type(got).__name__,
                                                           want.shape, want.dtype)
        bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
        bad = np.argwhere(np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits))
        if len(bad):
            i = tuple(int(x) for x in bad[0])
            return "%s: %d of %d elements differ, the first at %r: %r, expected %r" % (what, len(bad), want.size, i, got[i], want[i])
        return None
    if got is None or want is None:
        return None if got is want else "%s: %r, expected %r" % (what, got, want)
    return None if int(got) == int(want) else "%s: %r, expected %r" % (what, got, want)


# ---- the handle's side ----------------------------------------------------------------------------------------------------------

def knob_settings(path):
    """(names to clear, {name: value} to set) before the handle is created"""
    return KNOBS, dict(PATHS[path]["env"])


def open_handle(path, handle_seed, stream, cb_lib=None):
    """the capi.HipSampler of a path (batch paths: cb_lib is the fixture of tests/test_batch_calc.py); returns (handle, keep-alive)"""
    from mcmcpp_amd import capi
    cfg = PATHS[path]
    fam, kw, keep = cfg["family"], dict(cfg["create"]), None
    if fam in ("chains", "ladder"):
        return capi.HipSampler(cfg["W"], cfg["D"], cfg["calc"], np.stack([params_at(cfg, b) for b in start_betas(cfg)]), seed=handle_seed,
                               stream=stream, dtype=cfg["dtype"], num_chains=cfg["K"], **kw), None
    if fam == "batch":
        from tests.test_batch_calc import CTarget
        keep = CTarget(cb_lib, cfg["calc"], cfg["D"], None, cfg["dtype"])
        return capi.HipSampler(cfg["W"], cfg["D"], capi.CALC_BATCH, seed=handle_seed, stream=stream, dtype=cfg["dtype"],
                               batch_callback=keep.callback(), **kw), keep
    if fam == "diffevo":
        kw["mover"] = capi.MOVER_DIFFERENTIAL_EVOLUTION
    return capi.HipSampler(cfg["W"], cfg["D"], cfg["calc"], base_params(cfg), seed=handle_seed, stream=stream, dtype=cfg["dtype"], **kw), keep


class Runner:
    """Executes operations on a handle and returns results in the shapes Model.apply returns them."""

    def __init__(self, path, hip, model):
        self.cfg, self.hip, self.model, self.flight = PATHS[path], hip, model, None

    def _code(self, fn, *a, **kw):
        from mcmcpp_amd import capi
        try:
            fn(*a, **kw)
        except capi.HipError as e:
            return e.code
        return 0

    def _stored(self, k):
        """the first k stored steps (of every chain) of the run in flight; from device memory on a stream of their own, as a
        caller of run_device_async reads them"""
        chain = self.flight[0]
        lead = (slice(None),) if self.cfg["K"] > 1 else ()
        if isinstance(chain, np.ndarray):
            return chain[lead + (slice(0, k),)].copy()
        import torch
        mine = torch.cuda.Stream()
        with torch.cuda.stream(mine):
            first = chain[lead + (slice(0, k),)].clone()
        mine.synchronize()
        return first.cpu().numpy()

    def _device_rows(self, rows):
        import torch
        return torch.from_numpy(rows).to("cuda")

    def apply(self, op):
        hip, kind = self.hip, op[0]
        if kind == "set_state":
            return hip.set_state(*self.model.start_state(op[1]))
        if kind == "run":
            return hip.run(op[1], interval=op[2], save_chain=op[3], want_accepted=op[4])
        if kind == "run_device":
            chain, acc = hip.run_device(op[1], interval=op[2], want_accepted=op[3])
            return chain.cpu().numpy(), acc
        if kind in ASYNC_KINDS:
            self.flight = (hip.run_async if kind == "run_async" else hip.run_device_async)(op[1], interval=op[2], want_accepted=op[3])
            return None
        if kind == "refused_in_flight":
            cfg = self.cfg
            return self._code({"seek": lambda: hip.seek(3), "get_state": hip.get_state,
                               "calc_logp": lambda: hip.calc_logp(rows_for(cfg, 2, 1)),
                               "run_tempered": lambda: hip.run_tempered(2), "exchange_chains": lambda: hip.exchange_chains(0),
                               "set_chain_params": lambda: hip.set_chain_params(0, chain_params(cfg, 1)),
                               "evidence": lambda: hip.evidence_ratios(np.zeros((cfg["K"], 4, cfg["W"], cfg["D"]), po.np_dtype(cfg["dtype"])))}[op[1]])
        if kind == "wait_stored":
            hip.wait_stored(op[1])
            return self._stored(op[1])
        if kind == "run_wait":
            hip.run_wait()
            (chain, acc), self.flight = self.flight, None
            return (chain if isinstance(chain, np.ndarray) else chain.cpu().numpy()), acc
        if kind == "run_tempered":
            from mcmcpp_amd import capi
            shape, t = (self.cfg["K"], op[1], self.cfg["W"], self.cfg["D"]), po.np_dtype(self.cfg["dtype"])
            out = None if op[5] == "device" else np.empty(shape, t) if op[5] == "pageable" else capi.pinned_empty(shape, t)
            chain, acc, swaps, nxt = hip.run_tempered(op[1], interval=op[2], exchange_every=op[3], first_round=op[4], out=out, device=op[5] == "device")
            assert out is None or chain is out
            return (chain.cpu().numpy() if out is None else np.array(chain)), acc, swaps, nxt
        if kind == "evidence":
            x = evidence_draws(self.cfg, self.model.betas, op[2], op[3])
            fn = {"ratios": hip.evidence_ratios, "bridge": hip.evidence_bridge, "mbar": hip.evidence_mbar}[op[1]]
            return evidence_result(op[1], fn(x if op[4] == "host" else self._device_rows(x)))
        if kind == "half_step_async":
            return hip.half_step_async(op[1])
        if kind == "synchronize":
            return hip.synchronize()
        if kind == "seek":
            return hip.seek(op[1])
        if kind == "reset_counters":
            hip.reset_counters()
            return hip.counters()
        if kind == "get_state":
            return hip.get_state()
        if kind == "counters":
            return hip.counters()
        if kind == "calc_logp":
            return hip.calc_logp(rows_for(self.cfg, op[1], op[2]), chain=op[3])
        if kind == "calc_logp_device":
            return hip.calc_logp_device(self._device_rows(rows_for(self.cfg, op[1], op[2])), chain=op[3]).cpu().numpy()
        if kind == "refused":
            return self._code({"run_negative": lambda: hip.run(-1, interval=1, save_chain=False, want_accepted=False),
                               "run_interval_0": lambda: hip.run(1, interval=0),
                               "half_step_out_of_order": lambda: hip.half_step_async(0 if self.model.half_done else 1),
                               "seek_unsupported": lambda: hip.seek(4),
                               "run_tempered_every_0": lambda: hip.run_tempered(2, exchange_every=0),
                               "run_tempered_round_out_of_range": lambda: hip.run_tempered(op[2], interval=op[3], exchange_every=op[4], first_round=op[5]),
                               "half_step_async": lambda: hip.half_step_async(0)}[op[1]])
        if kind == "set_chain_params":
            return hip.set_chain_params(op[1], chain_params(self.cfg, op[2]))
        if kind == "exchange_chains":
            return hip.exchange_chains(op[1])
        raise ValueError(kind)


def run_sequence(path, seed, upto=None, cb_lib=None, ops=None, handle=None, log=None):
    """Sequence `seed` of `path` (or the given operations) on a handle and on the model, compared after every operation: the
    operation's result, and -- unless a run is in flight, when get_state is refused -- get_state and counters.  upto: stop
    behind that many operations.  The knobs of the path must be in the environment already (knob_settings).  Returns the model."""
    handle_seed, stream, planned = plan(path, seed)
    ops = planned if ops is None else ops
    ops = ops if upto is None else ops[:upto]
    model = Model(path, handle_seed, stream)
    hip, keep = open_handle(path, handle_seed, stream, cb_lib) if handle is None else handle
    runner = Runner(path, hip, model)

    def fail(i, line):
        raise AssertionError("path %s, seed %d (handle seed %d, stream %d), operation %d %r: %s\noperations so far:\n%s\n"
                             "tests.call_sequences.replay(%r, %d, %d) repeats them" % (path, seed, handle_seed, stream, i, ops[i], line,
                                                                                        render(ops[:i + 1]), path, seed, i + 1))

    for i, op in enumerate(ops):
        want = model.apply(op)
        got = runner.apply(op)
        if log:
            log("%3d %r" % (i, op))
        if want is not None or op[0] in ("refused", "refused_in_flight"):
            d = differs(got, want, "returned")
            if d:
                fail(i, d)
        if model.pending is None:
            d = differs(hip.get_state(), model.state(), "get_state") or differs(hip.counters(), model.counters(), "counters")
            if d:
                fail(i, d)
        if op[0] in ("run", "run_device", "run_tempered") and op[1] > 0:
            steps, launches = op[1] * op[2], hip.last_run_timing()[1]
            per_step = 4 if PATHS[path]["family"] == "batch" else 1 if PATHS[path]["full_step"] else 2
            if launches != per_step * steps:
                fail(i, "the handle counts %d step launches for %d steps: not the kernels this path is about" % (launches, steps))
    del keep
    return model


def replay(path, seed, upto=None, cb_lib=None):
    """run_sequence with the path's knobs put into os.environ (and left there): for debugging from a prompt"""
    clear, put = knob_settings(path)
    for k in clear:
        os.environ.pop(k, None)
    os.environ.update(put)
    return run_sequence(path, seed, upto=upto, cb_lib=cb_lib, log=print)
