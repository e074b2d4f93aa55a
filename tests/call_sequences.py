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


def _path(family, calc, dtype, W, D, env, graph_steps, full_step, long_runs, K=1, create=None, directed=()):
    return dict(family=family, calc=calc, dtype=dtype, W=W, D=D, K=K, env=env, create=create or {}, graph_steps=graph_steps,
                full_step=full_step, long_runs=long_runs, directed=tuple(directed))


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
EXCHANGE_ROUNDS = (0, 1, 2, 3, 4, 5, 6, 7, 2**40 - 2, 2**40 - 1)
SPECIAL_64 = (0, M64, 2**63, 2**63 + 1)            # handle seeds and streams: these, or 64 random bits (inc.hi = stream >> 63)

# Weights of the operation kinds while the handle is idle, per family ...
WEIGHTS = {
    "stretch": {"run": 10, "run_async": 4, "run_device": 5, "half_step_async": 5, "synchronize": 2, "seek": 4, "reset_counters": 3,
                "set_state": 3, "calc_logp": 3, "calc_logp_device": 3, "get_state": 3, "counters": 3, "refused": 3},
    "chains": {"run": 10, "run_device": 5, "seek": 4, "reset_counters": 3, "set_state": 3, "calc_logp": 3, "calc_logp_device": 2,
               "get_state": 2, "counters": 2, "refused": 2, "set_chain_params": 3, "exchange_chains": 4},
    "diffevo": {"run": 12, "run_device": 5, "set_state": 3, "reset_counters": 3, "get_state": 3, "counters": 2, "calc_logp": 3, "refused": 4},
    "batch": {"run": 12, "seek": 5, "set_state": 3, "reset_counters": 3, "get_state": 3, "counters": 2, "refused": 3},
}
# ... while an ensemble step is half done (half_step_async(0) went out) ...
WEIGHTS_HALF_DONE = {"half_step_async": 8, "synchronize": 1, "get_state": 1, "counters": 1, "calc_logp": 1, "refused": 2, "set_state": 0.5,
                     "reset_counters": 0.5}
# ... and while an asynchronous run is in flight (run_wait: before / after the first wait_stored)
WEIGHTS_IN_FLIGHT = {"refused_in_flight": 2, "wait_stored": 3, "run_wait": (0.5, 4)}
# What the last state-changing operation multiplies: a run that left an odd step count, a seek, a reset behind a run
FOLLOW = {
    "odd_run": {"run_device": 3, "half_step_async": 3, "set_state": 2, "reset_counters": 2},
    "seek": {"run": 3, "run_async": 2},
    "reset_after_run": {"run": 6},
}
REFUSED = {"stretch": ("run_negative", "run_interval_0", "half_step_out_of_order"), "chains": ("run_negative", "run_interval_0"),
           "diffevo": ("run_negative", "run_interval_0", "seek_unsupported"), "batch": ("run_negative", "run_interval_0")}
REFUSED_CODE = {"run_negative": E_ARG, "run_interval_0": E_ARG, "half_step_out_of_order": E_ARG, "seek_unsupported": E_UNSUPPORTED}
RUN_KINDS = ("run", "run_async", "run_device")
STATE_CHANGING = RUN_KINDS + ("half_step_async", "seek", "reset_counters", "set_state", "set_chain_params", "exchange_chains")


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
    rng = np.random.default_rng((PATH_INDEX[path], seed))
    handle_seed, stream = _special_64(rng), _special_64(rng)
    ops = [("set_state", int(rng.integers(0, 1000)))]
    # the generator's own view of the handle: enough to tell a legal operation from an illegal one
    step, half_done, in_flight, waited, context = 0, False, None, False, None
    drawn, directed = 0, list(cfg["directed"])
    while drawn < OPS_PER_SEQUENCE or in_flight is not None:
        if directed and drawn >= DIRECTED_AFTER and not half_done and in_flight is None:
            for op in directed:
                ops.append(op)
                step += op[1] * op[2]
            context = "odd_run" if sum(op[1] * op[2] for op in directed) & 1 else None
            directed = []
            continue
        left = OPS_PER_SEQUENCE - drawn
        if in_flight is not None:
            w = dict(WEIGHTS_IN_FLIGHT)
            w["run_wait"] = WEIGHTS_IN_FLIGHT["run_wait"][1 if waited else 0]
            kind = "run_wait" if left <= 1 else _pick(rng, w)
        elif half_done:
            kind = _pick(rng, WEIGHTS_HALF_DONE)
        else:
            w = dict(WEIGHTS[fam])
            for k, f in FOLLOW.get(context, {}).items():
                if k in w:
                    w[k] *= f
            if left < 3:
                w.pop("run_async", None)  # (an operation that would be illegal is not drawn: the run could not be waited for)
            kind = _pick(rng, w)
        drawn += 1
        if kind in ("run", "run_device", "run_async"):
            n_saved, interval = _run_shape(rng, cfg)
            flags = (bool(rng.random() < 0.75), bool(rng.random() < 0.75))
            if kind == "run":
                ops.append(("run", n_saved, interval) + flags)
            else:
                ops.append((kind, n_saved, interval, flags[1]))
            if kind == "run_async":
                in_flight, waited = n_saved, False
            step += n_saved * interval
            if n_saved > 0:
                context = "odd_run" if (n_saved * interval) & 1 else "run"
        elif kind == "refused_in_flight":
            ops.append((kind, ("seek", "calc_logp", "get_state")[int(rng.integers(0, 3))]))
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
            context = "seek"
        elif kind == "reset_counters":
            ops.append((kind,))
            context = "reset_after_run" if context in ("run", "odd_run") else None
        elif kind == "set_state":
            ops.append((kind, int(rng.integers(0, 1000))))
            step, half_done, context = 0, False, None
        elif kind in ("calc_logp", "calc_logp_device"):
            count, rows_seed = int(rng.integers(1, 21)), int(rng.integers(0, 2**31))
            chain = None
            if fam == "chains":
                chain = int(rng.integers(0, cfg["K"] + (1 if kind == "calc_logp" else 0)))
                chain = None if chain == cfg["K"] else chain
            ops.append((kind, count, rows_seed, 0 if kind == "calc_logp_device" and chain is None else chain))
        elif kind == "refused":
            names = REFUSED[fam]
            if half_done:
                names = ("half_step_out_of_order", "half_step_out_of_order") + names
            ops.append((kind, names[int(rng.integers(0, len(names)))]))
        elif kind == "set_chain_params":
            ops.append((kind, int(rng.integers(0, cfg["K"])), int(rng.integers(0, len(BETAS)))))
            context = None
        elif kind == "exchange_chains":
            ops.append((kind, EXCHANGE_ROUNDS[int(rng.integers(0, len(EXCHANGE_ROUNDS)))]))
            context = None
        else:
            ops.append((kind,))  # synchronize, get_state, counters
    return handle_seed, stream, ops


def generate(path, seed):
    return plan(path, seed)[2]


def render(ops):
    return "\n".join("%3d %r" % (i, op) for i, op in enumerate(ops))


def digest():
    """SHA-256 over every (path, seed) of SEEDS: the handle's seed and stream and the rendered operations"""
    h = hashlib.sha256()
    for path in PATHS:
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


def chain_params(cfg, beta_index):
    return (BETAS[beta_index] * base_params(cfg)).astype(po.np_dtype(cfg["dtype"]))


def rows_for(cfg, count, rows_seed):
    return (np.random.default_rng(rows_seed).standard_normal((count, cfg["D"])) * 1.5).astype(po.np_dtype(cfg["dtype"]))


# ---- how a run is cut into launches: run_plan.hpp and enqueue_steps restated, for the coverage facts only ------------------------

SUBCHUNK_BYTES = 32 << 20


def launch_chunks(cfg, n_saved, interval, save_chain, to_device):
    """the step counts a run hands to enqueue_steps, in order"""
    total = n_saved * interval
    if total == 0:
        return []
    G = cfg["graph_steps"]
    step_bytes = cfg["W"] * cfg["D"] * (8 if cfg["dtype"] == po.F64 else 4)
    if cfg["family"] in ("diffevo", "batch") or not save_chain:
        return [total]
    if to_device or (cfg["full_step"] and step_bytes % 16 == 0):
        per = (G if G > 0 else 64) // interval
        if not to_device:
            ring = 4
            while ring < 64 and 2 * ring * step_bytes <= 2 * SUBCHUNK_BYTES:
                ring *= 2
            per = min(per, (ring - 2) // 2)
        chunk, out, done = max(per, 1) * interval, [], 0
        while done < total:
            now = min(total - done, chunk)
            if not to_device and now == total - done and now > interval:
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
        self.params = [chain_params(cfg, b) for b in CHAINS3_START] if cfg["family"] == "chains" else [base_params(cfg)]
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
        self._in_flight_refusals = 0

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

    def _steps(self, n_saved, interval, save_chain, want_accepted, to_device=False):
        self._note_run(n_saved, interval, save_chain, to_device)
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
        return self._steps(n_saved, interval, True, want_accepted, to_device=True)

    def _run_async(self, n_saved, interval, want_accepted):
        self.pending = self._steps(n_saved, interval, True, want_accepted)
        self._in_flight_refusals = 0

    def _refused_in_flight(self, what):
        self._in_flight_refusals += 1
        return E_STATE

    def _wait_stored(self, k):
        return self.pending[0][:k]

    def _run_wait(self):
        out, self.pending = self.pending, None
        if self._in_flight_refusals:
            self.facts.add("an asynchronous run with a refused call inside it")
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

    def _refused(self, what):
        return REFUSED_CODE[what]

    def _set_chain_params(self, chain, beta_index):
        old = self.orcs[chain]
        pos, logp, nacc = old.get_state()
        self.nacc_off[chain] = self.nacc_off[chain] + nacc.astype(np.int64)
        self.ties_off += old.near_ties
        self.redraws_off += old.redraws
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
        return dict(proposed=out["proposed"], accepted=out["accepted"], near_ties=out["near_ties"])

    # -- coverage facts of a run, from the model's own numbers
    def _note_run(self, n_saved, interval, save_chain, to_device):
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
        heads = replays(cfg, launch_chunks(cfg, n_saved, interval, save_chain, to_device))
        if cfg["full_step"]:
            for at, _ in heads:
                f.add("a replay head with start parity %d, position parity %d" % ((self.step + at) & 1, at & 1))
        G = cfg["graph_steps"]
        if G >= 1:
            whole, rest = any(n == G for _, n in heads), any(n < G for _, n in heads)
            f.add("a run made of whole replays only" if whole and not rest else
                  "a run made of a remainder only" if rest and not whole else "a run made of whole replays and remainders")


def facts_wanted(path):
    """the coverage facts the six sequences of a path must show between them"""
    cfg = PATHS[path]
    fam = cfg["family"]
    want = {"a run that begins at even steps-since-origin", "a zero-step run", "set_state after an odd number of steps",
            "reset_counters between two runs", "a run that begins at odd steps-since-origin"}
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
        if cfg["full_step"]:
            want.add("a half-step pair after an odd full-step run")
    return want


def kinds_of(path):
    fam = PATHS[path]["family"]
    kinds = set(WEIGHTS[fam]) | {"set_state"}
    if fam == "stretch":
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
    if fam == "chains":
        return capi.HipSampler(cfg["W"], cfg["D"], cfg["calc"], np.stack([chain_params(cfg, b) for b in CHAINS3_START]), seed=handle_seed,
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
        if kind == "run_async":
            self.flight = hip.run_async(op[1], interval=op[2], want_accepted=op[3])
            return None
        if kind == "refused_in_flight":
            return self._code({"seek": lambda: hip.seek(3), "get_state": hip.get_state,
                               "calc_logp": lambda: hip.calc_logp(rows_for(self.cfg, 2, 1))}[op[1]])
        if kind == "wait_stored":
            hip.wait_stored(op[1])
            return self.flight[0][:op[1]].copy()
        if kind == "run_wait":
            hip.run_wait()
            out, self.flight = self.flight, None
            return out
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
                               "seek_unsupported": lambda: hip.seek(4)}[op[1]])
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
        if op[0] in ("run", "run_device") and op[1] > 0:
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
