"""A plain NumPy restatement of mcmcpp_amd/csrc/exchange_kernels.hpp: the block layout and what the three kernels leave behind.

Nothing here is shaped like the kernels (no lanes, no workgroups, no atomics): a pack is "the walkers of the slice whose masked
counter differs from `seen`", a scatter is "for every other rank's block, row by row".  Positions and log-posteriors are handled
as UNSIGNED INTEGERS of the element's size (uint64 for fp64, uint32 for fp32), so that a NaN's payload, -0.0 and the infinities
compare bit for bit and no arithmetic can touch them.  Per-walker arrays hold 2 n entries, colour-major, as in the library."""
import numpy as np

MASK = 0x7FFFFFFF      # kAcceptCountMask: the top bit of an accepted counter is the full-step kernels' "moved" mark
TOP = 0x80000000
HEADER_BYTES = 16      # count, cap, two words of padding
UINT = {8: np.uint64, 4: np.uint32}


def align16(b):
    return (b + 15) // 16 * 16


class Layout:
    """[header 16 B][idx: cap x u32][logp: cap x T][rows: cap x D x T], every piece starting on a multiple of 16 bytes"""

    def __init__(self, cap, dims, elem):
        self.cap, self.dims, self.elem = cap, dims, elem
        self.idx = HEADER_BYTES
        self.logp = self.idx + align16(4 * cap)
        self.rows = self.logp + align16(elem * cap)
        self.bytes = self.rows + align16(elem * cap * dims)

    def pieces(self):
        """(name, first byte, bytes in use) of the four pieces"""
        return [("header", 0, HEADER_BYTES), ("idx", self.idx, 4 * self.cap), ("logp", self.logp, self.elem * self.cap),
                ("rows", self.rows, self.elem * self.cap * self.dims)]


def row_pieces(dims, elem):
    """(vector?, pieces per row): a row whose length is a multiple of 16 bytes is copied in 16-byte pieces, any other by elements"""
    if dims * elem % 16 == 0:
        return True, dims * elem // 16
    return False, dims


def lanes_per_row(pieces):
    """the smallest power of two that is >= pieces, 64 at the most"""
    for lpr in (1, 2, 4, 8, 16, 32, 64):
        if lpr >= pieces:
            return lpr
    return 64


def trips(dims, elem):
    """how often the busiest lane of a row goes round the copy loop"""
    pieces = row_pieces(dims, elem)[1]
    return -(-pieces // lanes_per_row(pieces))


def slice_walkers(n, shard_begin, shard_count, color0=0, colors=2):
    """the walkers [shard_begin, shard_begin + shard_count) of colours [color0, color0 + colors), ascending"""
    return np.concatenate([c * n + shard_begin + np.arange(shard_count) for c in range(color0, color0 + colors)]).astype(np.int64)


def sync_seen(n_accept, seen, n, shard_begin, shard_count):
    """seen afterwards: the masked counter on the slice (both colours), untouched elsewhere"""
    out = seen.copy()
    w = slice_walkers(n, shard_begin, shard_count)
    out[w] = n_accept[w] & np.uint32(MASK)
    return out


def pack(n_accept, seen, n, shard_begin, shard_count, color0, colors):
    """(moved walkers ascending, seen afterwards, count)"""
    w = slice_walkers(n, shard_begin, shard_count, color0, colors)
    now = n_accept[w] & np.uint32(MASK)
    moved = w[now != seen[w]]
    out = seen.copy()
    out[moved] = n_accept[moved] & np.uint32(MASK)
    return moved, out, int(moved.size)


class BlockView:
    """the pieces of one block inside a byte buffer, as writable integer views"""

    def __init__(self, buf, cap, dims, elem, offset=0):
        lay = Layout(cap, dims, elem)
        assert buf.dtype == np.uint8 and buf.ndim == 1 and offset % 16 == 0 and offset + lay.bytes <= buf.size
        self.layout = lay
        self.header = buf[offset:offset + HEADER_BYTES].view(np.uint32)
        self.idx = buf[offset + lay.idx:offset + lay.idx + 4 * cap].view(np.uint32)
        self.logp = buf[offset + lay.logp:offset + lay.logp + elem * cap].view(UINT[elem])
        self.rows = buf[offset + lay.rows:offset + lay.rows + elem * cap * dims].view(UINT[elem]).reshape(cap, dims)

    count = property(lambda self: int(self.header[0]))


def scatter(blocks, cap, ranks, rank, dims, elem, pos_a, pos_b, logp_a, logp_b, stats):
    """blocks: the uint8 buffer of `ranks` gathered blocks.  Returns (pos_a, pos_b, logp_a, logp_b, stats, headers) afterwards;
    pos_b / logp_b stay None where None is given, stats is (overflow, max_count), headers the ranks' (count, cap, pad, pad)."""
    bb = Layout(cap, dims, elem).bytes
    views = [BlockView(blocks, cap, dims, elem, p * bb) for p in range(ranks)]
    pos_a, logp_a = pos_a.copy(), logp_a.copy()
    pos_b = None if pos_b is None else pos_b.copy()
    logp_b = None if logp_b is None else logp_b.copy()
    named = set()
    for p in range(ranks):
        if p == rank:
            continue
        v = views[p]
        rows = min(v.count, cap)
        w = v.idx[:rows].astype(np.int64)
        # slices are disjoint: no walker arrives twice in one exchange (the order of two writes is no part of the contract)
        assert len(set(w.tolist())) == rows and not named & set(w.tolist())
        named |= set(w.tolist())
        pos_a[w] = v.rows[:rows]
        logp_a[w] = v.logp[:rows]
        if pos_b is not None:
            pos_b[w] = v.rows[:rows]
        if logp_b is not None:
            logp_b[w] = v.logp[:rows]
    worst = max(v.count for v in views)
    stats = (int(stats[0]) | (1 if worst > cap else 0), max(int(stats[1]), worst))
    headers = np.array([v.header.copy() for v in views], dtype=np.uint32)
    headers[rank, 0] = 0
    return pos_a, pos_b, logp_a, logp_b, stats, headers
