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


def exchange_arrays(pos, logp, cross_logp, rnd, seed, stream=0, flip=False):
    """One round on arrays: pos [K][W][D] and logp [K][W] are edited in place.  cross_logp(k, rows) -> chain k's
    log-posteriors of rows.  Returns dict(proposed, accepted, near_ties, in_band): [K-1] counters and the list of
    (pair, walker) decided inside the near-tie band."""
    K, W = logp.shape
    out = dict(proposed=np.zeros(K - 1, np.uint64), accepted=np.zeros(K - 1, np.uint64), near_ties=np.zeros(K - 1, np.uint64), in_band=[])
    for a, b in pairs_of(K, rnd):
        j = a >> 1
        g = po.Pcg64(seed, 2**64 - 1 - stream)
        g.advance((rnd * SLOTS + j) * W)
        lp_ab = cross_logp(a, pos[b])
        lp_ba = cross_logp(b, pos[a])
        out["proposed"][a] = W
        for w in range(W):
            acc, tie, _, _ = decide(g.next(), logp[a, w], logp[b, w], lp_ab[w], lp_ba[w], flip)
            if tie:
                out["near_ties"][a] += 1
                out["in_band"].append((a, w))
            if acc:
                row = pos[a, w].copy()
                pos[a, w] = pos[b, w]
                pos[b, w] = row
                logp[a, w] = lp_ab[w]
                logp[b, w] = lp_ba[w]
                out["accepted"][a] += 1
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
