"""A sequential replay of the random stream of Mover::DifferentialEvolution, in plain Python integers and NumPy.

Independent of the library and of the oracle: neither pcg128.hpp nor oracle/ is read.  The engine is pcg64 as pcg-cpp
defines it (setseq_xsl_rr_128_64): a 128-bit LCG with the default multiplier, the XSL-RR output of the state AFTER the step,
seeded as MultiSampler.h:54 does (engine.seed(seed, stream)).  tests/test_de_planner.py pins its raw stream to
numpy.random.PCG64 with the state set directly.

replay() walks DifferentialEvolution.h:83-87 update after update -- ind1 = engine(n); ind2 = engine(n) until it differs; D
jitters; the accept draw -- with bounded_rand's threshold as a parameter, and returns per batch of updates what the planner
of mcmcpp_amd/csrc/diffevo_plan.hpp must leave behind: each update's partners, the engine state behind its integer draws and
its raw accept draw; the events (update, draws thrown away so far); the stream head behind the batch.  It also lists the
bad positions a scan must find from where the scan starts, and predicts the three sticky flags from their stated rules."""
import numpy as np

M128 = (1 << 128) - 1
MULT = (2549297995355413924 << 64) | 4865540595714422341  # pcg-cpp PCG_DEFAULT_MULTIPLIER_128

SHIFT_MAX, WINDOW, OVERRUN, SEGMENTS, MAX_EVENTS = 4095, 32, 255, 64, 1024
ERR_SHIFT, ERR_CAND, ERR_WINDOW = 1, 2, 4


def seed_engine(seed, stream=0):
    """(state, inc) of pcg64(seed, stream): inc = stream << 1 | 1; state = 0; step; state += seed; step"""
    inc = ((stream << 1) | 1) & M128
    state = ((seed + inc) * MULT + inc) & M128
    return state, inc


def step(state, inc):
    return (state * MULT + inc) & M128


def output(state):
    """XSL-RR 128 -> 64"""
    x = ((state >> 64) ^ state) & 0xFFFFFFFFFFFFFFFF
    rot = state >> 122
    return ((x >> rot) | (x << ((64 - rot) & 63))) & 0xFFFFFFFFFFFFFFFF


def production_threshold(n):
    return (2 ** 64 - n) % n


class Stream:
    """states[k]: the engine state after k steps from the seeded one; raw[k] = output(states[k + 1]) is draw k"""

    def __init__(self, seed, stream=0):
        self.state0, self.inc = seed_engine(seed, stream)
        self.states = [self.state0]
        self.raw = []

    def need(self, draws):
        s, inc, states, raw = self.states[-1], self.inc, self.states, self.raw
        while len(raw) < draws:
            s = (s * MULT + inc) & M128
            states.append(s)
            raw.append(output(s))

    def draw(self, k):
        if k >= len(self.raw):
            self.need(k + 4096)
        return self.raw[k]

    def raws(self, first, count):
        self.need(first + count)
        return np.array(self.raw[first:first + count], dtype=np.uint64)


def update_at(st, a, n, threshold, limit=None):
    """The integer part of an update whose first draw is draw `a`: (ind1, ind2, used, thrown) -- `used` raw draws, of which
    used - 2 were thrown away (their indices in `thrown`, with the stage that threw them: 1 = below the threshold in front of
    ind1, 2 = below it in front of ind2, 3 = an ind2 equal to ind1).  limit: None, or the raw draws the window allows:
    an update that needs more returns None."""
    k, thrown = a, []
    while True:
        if limit is not None and k - a >= limit:
            return None
        v = st.draw(k)
        k += 1
        if v >= threshold:
            break
        thrown.append((k - 1, 1))
    ind1 = v % n
    while True:
        if limit is not None and k - a >= limit:
            return None
        v = st.draw(k)
        k += 1
        if v < threshold:
            thrown.append((k - 1, 2))
            continue
        if v % n != ind1:
            break
        thrown.append((k - 1, 3))
    return ind1, v % n, k - a, thrown


class Batch:
    pass


def replay(seed, n, D, threshold, updates, batches, stream=0, st=None):
    """`batches` batches of `updates` updates each, sequentially.  Per batch (absolute draw indices count from the seeded
    state; states are 128-bit integers):
      first, base, extra_base   the batch's first draw, the engine state in front of it, the draws thrown away before it
      ind1, ind2, s, accept_raw, E, start   per update; s: the state behind the integer draws; start: its first draw
      events                    [(m, shift_after)] for every update that threw draws away
      thrown                    [(draw index, stage)] of the batch
      shift, next_state         the draws thrown away in the batch; the state in front of the next batch"""
    st = st or Stream(seed, stream)
    per = D + 3
    out, a, extra = [], 0, 0
    for _ in range(batches):
        b = Batch()
        b.first, b.base, b.extra_base = a, None, extra
        b.ind1, b.ind2, b.s, b.accept_raw, b.E, b.start, b.events, b.thrown = [], [], [], [], [], [], [], []
        c = 0
        for m in range(updates):
            i1, i2, used, thrown = update_at(st, a, n, threshold)
            b.start.append(a)
            b.ind1.append(i1)
            b.ind2.append(i2)
            b.E.append(used - 2)
            b.thrown += thrown
            acc = a + used + D            # the accept draw: D jitters behind the integer draws
            b.accept_raw.append(st.draw(acc))
            b.s.append(st.states[a + used])
            if used > 2:
                c += used - 2
                b.events.append((m, c))
            a = acc + 1
        assert a == b.first + per * updates + c
        st.need(a + 1)
        b.base = st.states[b.first]
        b.shift, b.next_state = c, st.states[a]
        extra += c
        out.append(b)
    return st, out


def scan_start(batches, b):
    """the draw a scan of batch b calls position 0: the batch's first had the batch in front of it thrown nothing away"""
    return batches[b].first - (batches[b - 1].shift if b > 0 else 0)


def window_e(st, a, n, threshold):
    """E of a bad position as the scan lists it: the draws an update starting there throws away, or OVERRUN where the update
    does not fit kDeWindow raw draws"""
    u = update_at(st, a, n, threshold, limit=WINDOW)
    return OVERRUN if u is None else u[2] - 2


def scan_lists(st, first, scan_positions, seg_len, n, threshold):
    """What a scan from draw `first` lists: per list, the set of (p, E) of the bad positions p in [0, scan_positions) -- a
    position is bad when one of the two draws there lies below the threshold or both name the same walker"""
    raw = st.raws(first, scan_positions + 1)
    ind = raw % np.uint64(n)
    t = np.uint64(threshold)
    bad = (raw[:-1] < t) | (raw[1:] < t) | (ind[:-1] == ind[1:])
    lists = [set() for _ in range(SEGMENTS)]
    for p in np.flatnonzero(bad):
        p = int(p)
        lists[p // seg_len].add((p, window_e(st, first + p, n, threshold)))
    return lists


def predict_flags(st, batches, b, n, threshold, scan_positions, seg_len, bad_capacity, resolve_capacity):
    """(flags the scan of batch b raises, flags its resolve raises) from the stated rules:
      kDeErrCand    scan: a list holds more than bad_capacity positions; resolve: the lists (each cut to bad_capacity) hold more
                    than resolve_capacity together, or the batch has more than kDeMaxEvents events
      kDeErrShift   the draws thrown away in the batch pass kDeShiftMax
      kDeErrWindow  an update of the batch needs more than kDeWindow raw draws
    What a flagged batch and those behind it hold is not specified: predictions hold up to the first flagged batch."""
    lists = scan_lists(st, scan_start(batches, b), scan_positions, seg_len, n, threshold)
    scan = ERR_CAND if any(len(l) > bad_capacity for l in lists) else 0
    res = 0
    if sum(min(len(l), bad_capacity) for l in lists) > resolve_capacity or len(batches[b].events) > MAX_EVENTS:
        res |= ERR_CAND
    if batches[b].shift > SHIFT_MAX:
        res |= ERR_SHIFT
    if any(e > WINDOW - 2 for e in batches[b].E):
        res |= ERR_WINDOW
    return scan, res, lists
