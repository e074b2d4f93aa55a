"""Parallel tempering restated on the CPU, independent of the library: K oracles (params_k, seed + k) and the replica
exchange among them written out in Python.  TEST INFRASTRUCTURE ONLY.

Round r pairs chains (k, k + 1) for k = r (mod 2); walker w of chain k with walker w of chain k + 1.  The pair (round, slot
j = k >> 1, walker w) takes the raw output at position (r * 8 + j) * W + w of the pcg64 engine (seed, 2^64 - 1 - stream).
u as libstdc++ makes it (divide by 2^64, clamp below 1), ln U = math.log(1 - u), and in Python floats
    delta = (logp_k(x_{k+1}) - logp_k(x_k)) + (logp_{k+1}(x_k) - logp_{k+1}(x_{k+1})),      accept iff ln U < delta.
A near tie: |ln U - delta| <= tie_eps_f64 * (|ln U| + the four |logp|) and the margin finite."""
import math

import numpy as np

from oracle import pyoracle as po

SLOTS = 8
BELOW_ONE = math.nextafter(1.0, 0.0)


def pairs_of(K, rnd):
    return [(k, k + 1) for k in range(rnd & 1, K - 1, 2)]


def canonical(draw):
    u = draw / 2.0**64  # (int / float: the integer is rounded to nearest even first, the division is exact)
    return BELOW_ONE if u >= 1.0 else u


def decide(draw, lp_aa, lp_bb, lp_ab, lp_ba, flip=False):
    """(accept, near tie, ln U, delta) of one pair of walkers; flip: the sign of delta reversed (a wrong rule, for the
    invariance test)"""
    ln_u = math.log(1.0 - canonical(draw))
    lp_aa, lp_bb, lp_ab, lp_ba = float(lp_aa), float(lp_bb), float(lp_ab), float(lp_ba)
    delta = (lp_ab - lp_aa) + (lp_ba - lp_bb)
    if flip:
        delta = -delta
    margin = abs(ln_u - delta)
    tie = math.isfinite(margin) and margin <= po.tie_eps(po.F64) * (abs(ln_u) + abs(lp_aa) + abs(lp_bb) + abs(lp_ab) + abs(lp_ba))
    return ln_u < delta, tie, ln_u, delta


def _bits(a):
    """an array of floats seen as unsigned integers of the same size: a swap is a move of bits (NaN payloads included)"""
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def swap_arrays(pos, logp, cross, first_chain, pairs, rnd, seed, stream=0, flip=False):
    """The swap of one round on given cross evaluations.  pos [K][W][D] (floats or their integer views) and logp [K][W] (floats)
    are edited in place; cross [pairs][2][W] (floats) holds logp_a(x_b) and logp_b(x_a) of slot j's chains a = first_chain + 2 j
    and b = a + 1; slot j draws from position (rnd * 8 + j) * W on, whatever first_chain is.  Returns dict(accepted, near_ties: [pairs] counters; accept, tie: [pairs][W] flags;
    draws: [pairs][W] raw outputs; in_band: the list of (slot, walker) decided inside the near-tie band)."""
    W = logp.shape[1]
    out = dict(accepted=np.zeros(pairs, np.uint64), near_ties=np.zeros(pairs, np.uint64), accept=np.zeros((pairs, W), bool), tie=np.zeros((pairs, W), bool),
               draws=np.zeros((pairs, W), np.uint64), in_band=[])
    pos_bits, logp_bits, cross_bits = _bits(pos), _bits(logp), _bits(cross)
    for j in range(pairs):
        a = first_chain + 2 * j
        b = a + 1
        g = po.Pcg64(seed, 2**64 - 1 - stream)
        g.advance((rnd * SLOTS + j) * W)
        for w in range(W):
            draw = g.next()
            acc, tie, _, _ = decide(draw, logp[a, w], logp[b, w], cross[j, 0, w], cross[j, 1, w], flip)
            out["draws"][j, w], out["accept"][j, w], out["tie"][j, w] = draw, acc, tie
            if tie:
                out["near_ties"][j] += 1
                out["in_band"].append((j, w))
            if acc:
                row = pos_bits[a, w].copy()
                pos_bits[a, w] = pos_bits[b, w]
                pos_bits[b, w] = row
                logp_bits[a, w:w + 1] = cross_bits[j, 0, w:w + 1]
                logp_bits[b, w:w + 1] = cross_bits[j, 1, w:w + 1]
                out["accepted"][j] += 1
    return out


def exchange_arrays(pos, logp, cross_logp, rnd, seed, stream=0, flip=False):
    """One round on arrays: pos [K][W][D] and logp [K][W] are edited in place.  cross_logp(k, rows) -> chain k's
    log-posteriors of rows.  Returns dict(proposed, accepted, near_ties, in_band): [K-1] counters and the list of
    (pair, walker) decided inside the near-tie band.  (The pairs of a round share no chain: all cross evaluations are made in
    front of the swap, as the device makes them.)"""
    K, W = logp.shape
    out = dict(proposed=np.zeros(K - 1, np.uint64), accepted=np.zeros(K - 1, np.uint64), near_ties=np.zeros(K - 1, np.uint64), in_band=[])
    chains = pairs_of(K, rnd)
    if not chains:
        return out
    cross = np.stack([np.stack([cross_logp(a, pos[b]), cross_logp(b, pos[a])]) for a, b in chains]).astype(logp.dtype, copy=False)
    first = chains[0][0]
    assert first == rnd & 1 and [a for a, _ in chains] == [first + 2 * j for j in range(len(chains))]
    r = swap_arrays(pos, logp, cross, first, len(chains), rnd, seed, stream, flip)
    for j, (a, _) in enumerate(chains):
        out["proposed"][a] = W
        out["accepted"][a] = r["accepted"][j]
        out["near_ties"][a] = r["near_ties"][j]
    out["in_band"] = [(chains[j][0], w) for j, w in r["in_band"]]
    return out


class Ladder:
    """K oracles, chain k with params[k] and seed + k, and the exchange among them."""

    def __init__(self, W, D, calc, params, seed, dtype=po.F64, stream=0):
        self.K, self.W, self.D, self.seed, self.stream, self.dtype = len(params), W, D, seed, stream, dtype
        self.orcs = [po.Oracle(W, D, calc, p, seed=seed + k, stream=stream, dtype=dtype) for k, p in enumerate(params)]

    def logp(self, k, rows):
        return self.orcs[k].logp(rows)

    def set_state(self, pos, logp):
        for k, o in enumerate(self.orcs):
            o.set_state(pos[k], logp[k])

    def run(self, n_saved, interval=1, threads=4):
        """(chain [K][n_saved][W][D], accepted per step [K][n_saved * interval])"""
        r = [o.run(n_saved, interval=interval, mode=po.MODE_COUNTER, threads=threads) for o in self.orcs]
        return np.stack([c for c, _ in r]), np.stack([a for _, a in r])

    def get_state(self):
        s = [o.get_state() for o in self.orcs]
        return tuple(np.stack([x[i] for x in s]) for i in range(3))

    def exchange(self, rnd, flip=False):
        """One round, in place on the oracles' own arrays"""
        pos = [o.positions_view() for o in self.orcs]
        logp = [o.logp_view() for o in self.orcs]
        P, L = np.stack(pos), np.stack(logp)
        out = exchange_arrays(P, L, self.logp, rnd, self.seed, self.stream, flip)
        for k in range(self.K):
            pos[k][...] = P[k]
            logp[k][...] = L[k]
        return out

    def run_exchanging(self, n_saved, interval=1, exchange_every=1, first_round=0, flip=False):
        per = exchange_every // interval
        chains, accs, rnd, done = [], [], first_round, 0
        swaps = dict(proposed=np.zeros(self.K - 1, np.uint64), accepted=np.zeros(self.K - 1, np.uint64), near_ties=np.zeros(self.K - 1, np.uint64))
        while done < n_saved:
            seg = min(per, n_saved - done)
            c, a = self.run(seg, interval)
            chains.append(c)
            accs.append(a)
            done += seg
            if seg == per:
                r = self.exchange(rnd, flip)
                for key in swaps:
                    swaps[key] += r[key]
                rnd += 1
        return np.concatenate(chains, axis=1), np.concatenate(accs, axis=1), swaps, rnd
