"""The three kernels behind the exchange of moved rows (mcmcpp_amd/csrc/exchange_kernels.hpp), alone and on crafted inputs.

A split ensemble's ranks keep replicas and send each other only the rows that moved: exchange_pack_kernel fills a block of `cap`
slots, exchange_scatter_kernel writes the other ranks' blocks into the replica, exchange_sync_seen_kernel resets what counts as
"moved".  A row missed or written in the wrong place is silent corruption of one replica.  tests/test_split_loopback.py runs them
end to end against the oracle, at whatever counts, caps and shapes its runs happen to reach; this module chooses them.

  CPU   mcmcpp_amd/csrc/exchange_plan.hpp (block layout, pieces and lanes per row, the three grids), through
        tests/cpp/exchange_plan_cases.cpp built with the host compiler alone, against a transcription of the arithmetic the kernels
        and SamplerHost::exchange_compact held inline before (three copies of it), for every D up to 1024 in both element sizes;
        and that every piece is aligned, nothing overlaps and every walker, slot and peer is covered once.
  CPU   that the inputs below have the properties they are there for (counts against caps, pieces and trips per D, walkers that
        differ from `seen` in the top bit alone), from tests/exchange_restatement.py alone.
  GPU   tests/cpp/exchange_device.hip launches each production kernel unchanged, with the grid of exchange_plan.hpp, on those
        inputs; the results are compared with the restatement.  Everything is bit-exact (integer views): there is no tolerance.
        The order of the slots of a packed block comes from an atomicAdd across workgroups and is no part of the contract, so
        a packed block is judged as a set.

What a deliberately wrong kernel does to this module is listed in DESIGN section 2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import exchange_restatement as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

MASK, TOP = xr.MASK, xr.TOP
PATTERN = 0xA5   # what a block holds before a pack; 0xA5A5A5A5 is no walker of any case (the shim would refuse it as an index)
GUARD = 16384    # bytes behind a block that travel with it: two of the longest rows (1024 x 8 bytes)

# ---- rows: (D, element bytes) -> (16-byte pieces?, pieces, lanes per row, trips of the busiest lane); the smallest shapes that
# take each path of the two copy loops
ROWS = {
    (1, 8): (False, 1, 1, 1),        # scalar, one lane per row
    (3, 8): (False, 3, 4, 1),        # scalar, four lanes, one idle
    (2, 8): (True, 1, 1, 1),         # one piece
    (6, 8): (True, 3, 4, 1),         # three pieces on four lanes
    (64, 8): (True, 32, 32, 1),      # the widest row of the end-to-end cases before this module
    (128, 8): (True, 64, 64, 1),     # the lane bound, one trip
    (130, 8): (True, 65, 64, 2),     # the second trip, taken by one lane
    (131, 8): (False, 131, 64, 3),   # scalar, three trips
    (1023, 8): (False, 1023, 64, 16),
    (1024, 8): (True, 512, 64, 8),
    (4, 4): (True, 1, 1, 1),
    (5, 4): (False, 5, 8, 1),
    (12, 4): (True, 3, 4, 1),
    (256, 4): (True, 64, 64, 1),
    (260, 4): (True, 65, 64, 2),
    (1022, 4): (False, 1022, 64, 16),  # 4088 bytes: a multiple of 8, not of 16
    (1024, 4): (True, 256, 64, 4),
}
ROW_IDS = ["D%d_f%d" % (d, 8 * e) for d, e in ROWS]
TWO_ROWS = [(6, 8), (130, 8)]

# ---- slices: n = 300 walkers per colour
N = 300
SLICE_RANGES = [(37, 203), (0, 1), (0, 16), (44, 256), (43, 257), (0, 300)]
COLOURS = [(0, 2), (0, 1), (1, 1)]  # (color0, colors)
SLICES = [(sb, sc, c0, cs) for sb, sc in SLICE_RANGES for c0, cs in COLOURS]
ROW_SLICE = (37, 203, 0, 2)  # 406 walkers: two pack workgroups, the second ragged (150 walkers), its last wavefront with 6
MOVED_SETS = ("none", "all", "last", "third", "second_colour", "top_bit_only", "top_bit_and_low", "outside")

SPECIALS = {8: [0x7FF80000DEADBEEF, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000],   # NaN with a payload, -0.0, +inf, -inf
            4: [0x7FC0BEEF, 0x80000000, 0x7F800000, 0xFF800000]}


# ---------------------------------------------------------------------------------------------------------------- inputs

def values(rng, shape, elem):
    """normal variates as integer views; every seventh cell one of SPECIALS in turn"""
    a = rng.standard_normal(shape).astype(np.float64 if elem == 8 else np.float32).view(xr.UINT[elem])
    flat = a.reshape(-1)
    at = np.arange(3, flat.size, 7)
    flat[at] = np.array(SPECIALS[elem], dtype=xr.UINT[elem])[(at // 7) % 4]
    return a


def ensemble(n, dims, elem, seed):
    rng = np.random.default_rng(seed)
    return values(rng, (2 * n, dims), elem), values(rng, 2 * n, elem)


def counters(kind, n, sb, sc, color0, colors, seed=5):
    """(n_accept, seen) in which the walkers of `kind` moved; seen holds masked counters, four of them about to wrap"""
    rng = np.random.default_rng(seed)
    W = 2 * n
    seen = rng.integers(0, 2 ** 31, W, dtype=np.uint32)
    seen[rng.choice(W, 4, replace=False)] = MASK
    n_accept = seen.copy()
    S = xr.slice_walkers(n, sb, sc, color0, colors)

    def bump(w):
        n_accept[w] = (seen[w] + 1 + rng.integers(0, 1000, len(w), dtype=np.uint32)) & np.uint32(MASK)

    def mark(w):
        n_accept[w] |= np.uint32(TOP)

    if kind == "all":
        bump(S), mark(S[1::2])
    elif kind == "last":
        bump(S[-1:])
    elif kind == "third":
        bump(S[::3])
    elif kind == "second_colour":
        bump(n + sb + np.arange(sc))
    elif kind == "top_bit_only":
        mark(S[::2])
    elif kind == "top_bit_and_low":
        bump(S[::2]), mark(S[::2])
    elif kind == "outside":
        others = np.setdiff1d(np.arange(W), S)
        bump(others), mark(others[::2])
    else:
        assert kind == "none"
    return n_accept, seen


def moved_count(kind, sc, color0, colors):
    """how many walkers `kind` moves, stated without the restatement"""
    walkers = sc * colors
    return {"none": 0, "all": walkers, "last": 1, "third": -(-walkers // 3), "second_colour": sc if color0 + colors == 2 else 0, "top_bit_only": 0,
            "top_bit_and_low": -(-walkers // 2), "outside": 0}[kind]


def caps_for(count, sc):
    """1, 7 (odd: the idx and the fp64 logp array both end off a 16-byte boundary), the moved count exactly, one less, a whole slice"""
    return sorted(c for c in {1, 7, count, count - 1, 2 * sc} if c >= 1)


def scatter_case(dims, elem, ranks, rank, rotation, own_large=False, small=False, seed=17):
    """Gathered blocks and a replica.  The peers' counts go through 0, 1, a workgroup's rows exactly, one more, cap and above cap
    (rotated by `rotation`; `small`: one row each); this rank's own block names walkers of its own and carries rows, which must
    not arrive.  Slots past a block's count name `spare`, a walker no block names, and carry rows too."""
    rpb = 256 // xr.lanes_per_row(xr.row_pieces(dims, elem)[1])
    cap = rpb + 3
    palette = [1] * 6 if small else [0, 1, rpb, rpb + 1, cap, cap + 2]
    peers = [p for p in range(ranks) if p != rank]
    counts = {p: palette[(j + rotation) % 6] for j, p in enumerate(peers)}
    counts[rank] = 0 if small else (cap + 5 if own_large else 3)
    n = max(20, (ranks * cap + 1) // 2 + 3)
    rng = np.random.default_rng(seed + rotation)
    pos_a, logp_a = ensemble(n, dims, elem, seed + 100)
    pos_b, logp_b = ensemble(n, dims, elem, seed + 200)
    perm = rng.permutation(2 * n)
    spare, at = int(perm[-1]), 0
    lay = xr.Layout(cap, dims, elem)
    blocks = np.full(ranks * lay.bytes, PATTERN, np.uint8)
    named = {}
    for p in range(ranks):
        v = xr.BlockView(blocks, cap, dims, elem, p * lay.bytes)
        rows = min(counts[p], cap)
        v.header[:] = (counts[p], cap, 0, 0)
        v.idx[:] = spare
        v.idx[:rows] = named[p] = perm[at:at + rows]
        v.logp[:] = values(rng, cap, elem)
        v.rows[:] = values(rng, (cap, dims), elem)
        at += rows
    assert at < 2 * n
    return dict(dims=dims, elem=elem, ranks=ranks, rank=rank, cap=cap, rpb=rpb, n=n, counts=counts, named=named, spare=spare, blocks=blocks, pos_a=pos_a,
                pos_b=pos_b, logp_a=logp_a, logp_b=logp_b)


RANKS = [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (8, 0), (8, 3), (8, 7)]  # this rank first, in the middle, last


# ---------------------------------------------------------------------------------------------------------------- builds

@pytest.fixture(scope="module")
def plan_exe():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "exchange_plan_cases")
    # the host compiler alone, and no include path but the header's own directory: exchange_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "exchange_plan_cases.cpp"), "-I", CSRC])
    return exe


def plan_lines(exe, *args):
    out = subprocess.run([exe] + list(args), capture_output=True, text=True, check=True).stdout
    return [tuple(int(x) for x in line.split()) for line in out.splitlines()]


def build_shim():
    """tests/cpp/exchange_device.hip with the flags of mcmcpp_amd/csrc/Makefile"""
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "exchange_device.hip")
    out = os.path.join(BUILD, "libexchange_device.so")
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc", ".h")))
    if not os.path.exists(out) or os.path.getmtime(out) < max(newest, os.path.getmtime(src)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-mllvm", "-amdgpu-kernarg-preload-count=16", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-I" + CSRC, src, "-o", out])
    return out


@pytest.fixture(scope="module")
def dev():
    L = C.CDLL(build_shim())
    L.xd_sync_seen.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    for t in ("f64", "f32"):
        getattr(L, "xd_pack_" + t).argtypes = [C.c_void_p] * 5 + [C.c_size_t, C.c_uint32] + [C.c_int] * 6
        getattr(L, "xd_scatter_" + t).argtypes = [C.c_void_p, C.c_uint32] + [C.c_int] * 4 + [C.c_void_p] * 5
    L.xd_block_bytes.restype = C.c_size_t
    L.xd_block_bytes.argtypes = [C.c_uint32, C.c_int, C.c_int]
    return L


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def _t(elem):
    return "f64" if elem == 8 else "f32"


# ----------------------------------------------------------------------------------------------- CPU: exchange_plan.hpp

CAPS = [1, 2, 3, 7, 8, 15, 16, 17, 255, 256, 257, 1000, 16384]


def _earlier_row(dims, elem):
    """the lines exchange_pack_kernel, exchange_scatter_kernel and exchange_compact each held: (vec, pieces, lpr, rows_per_block)"""
    vec = (dims * elem) % 16 == 0
    pieces = dims * elem // 16 if vec else dims
    lpr = 1
    while lpr < pieces and lpr < 64:
        lpr <<= 1
    return int(vec), pieces, lpr, 256 // lpr


def _earlier_block(cap, dims, elem):
    """xblock_idx_offset, xblock_logp_offset<T>, xblock_rows_offset<T>, xblock_bytes<T> as exchange_kernels.hpp defined them"""
    def a16(b):
        return (b + 15) & ~15
    idx = 16
    logp = idx + a16(cap * 4)
    rows = logp + a16(cap * elem)
    return idx, logp, rows, rows + a16(cap * dims * elem)


def test_plan_header_includes_no_hip_header(plan_exe):
    """(plan_exe: g++ compiled the case program against the header with no HIP include path)"""
    for name, want in (("exchange_plan.hpp", ["<stddef.h>", "<stdint.h>", '"canonical.hpp"']), ("canonical.hpp", ["<stdint.h>"])):
        text = open(os.path.join(CSRC, name)).read()
        assert [line.split()[1] for line in text.split("\n") if line.startswith("#include")] == want, name


def _body(text, head):
    """the braces that follow the one occurrence of `head` in `text`, and what they hold"""
    assert text.count(head) == 1, head
    at = text.index("{", text.index(head))
    depth = 0
    for i in range(at, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[at:i + 1]
    raise AssertionError("unbalanced braces behind " + head)


def test_the_exchange_arithmetic_has_one_copy():
    """The three kernels, SplitExchange's exchange_compact and exchange_reset call exchange_plan.hpp; none of them states lanes per row, pieces or
    a grid itself.  (Only their own bodies are searched: the same idioms are at home elsewhere in these files.)"""
    kernels = open(os.path.join(CSRC, "exchange_kernels.hpp")).read()
    host = open(os.path.join(CSRC, "split_exchange.hpp")).read()  # (SplitExchange: the exchange side of a split handle)
    assert '#include "exchange_plan.hpp"' in kernels
    bodies = {
        "sync_seen": (_body(kernels, "exchange_sync_seen_kernel("), []),
        "pack": (_body(kernels, "exchange_pack_kernel("), ["exchange_row_pieces(dims, sizeof(T))", "exchange_lanes_per_row(pieces)"]),
        "scatter": (_body(kernels, "exchange_scatter_kernel("), ["exchange_row_pieces(dims, sizeof(T))", "exchange_lanes_per_row(pieces)",
                                                                 "exchange_scatter_rows_per_block(lpr)"]),
        "exchange_compact": (_body(host, "int exchange_compact("), ["exchange_pack_blocks(colors * shard_count)", "exchange_scatter_grid(cap, D, sizeof(T), world)",
                                                                    "dim3(kPackThreads)", "dim3(kScatterThreads)"]),
        "exchange_reset": (_body(host, "int exchange_reset("), ["exchange_sync_seen_blocks(shard_count)", "dim3(kSyncSeenThreads)"]),
    }
    for name, (body, calls) in bodies.items():
        for used in calls:
            assert used in body, (name, used)
        for gone in ("<<= 1", "% 16", "/ 16", "& ~", "256", "- 1) /"):
            assert gone not in body, (name, gone)
    shim = open(os.path.join(ROOT, "tests", "cpp", "exchange_device.hip")).read()
    for used in ("exchange_pack_blocks(colors * shard_count)", "exchange_scatter_grid(cap, dims, sizeof(T), ranks)", "exchange_sync_seen_blocks(shard_count)"):
        assert used in shim, used
    hdrs = [line for line in open(os.path.join(CSRC, "Makefile")).read().split("\n") if line.startswith("HDRS")]
    assert len(hdrs) == 1 and "exchange_plan.hpp" in hdrs[0].split() and "split_exchange.hpp" in hdrs[0].split()


def test_plan_constants(plan_exe):
    out = subprocess.run([plan_exe, "constants"], capture_output=True, text=True, check=True).stdout
    assert dict(kv.split("=") for kv in out.split()) == {"header": "16", "walkers_per_wave": "16", "waves_per_block": "16", "pack_threads": "1024",
                                                         "scatter_threads": "256", "sync_threads": "256", "max_lpr": "64"}


def test_rows_over_every_d_equal_the_inline_arithmetic(plan_exe):
    rows = plan_lines(plan_exe, "rows")
    assert [(e, d) for e, d, *_ in rows] == [(e, d) for e in (8, 4) for d in range(1, 1025)]
    for e, d, vec, pieces, lpr, rpb in rows:
        assert (vec, pieces, lpr, rpb) == _earlier_row(d, e), (e, d)
        assert (bool(vec), pieces) == xr.row_pieces(d, e) and lpr == xr.lanes_per_row(pieces)
        assert lpr in (1, 2, 4, 8, 16, 32, 64) and (lpr >= pieces or (lpr == 64 and pieces > 64))
        assert lpr == 1 or lpr // 2 < pieces  # and no more lanes than that
        assert rpb * lpr == 256
        assert pieces * (16 if vec else e) == d * e  # the pieces are the row
    # where the second trip starts: fp64 at D = 130 for rows of 16-byte pieces and D = 65 for scalar rows, fp32 at D = 260 and D = 65
    first = {(e, vec): min(d for ee, d, v, pieces, lpr, _ in rows if ee == e and v == vec and pieces > lpr) for e in (8, 4) for vec in (0, 1)}
    assert first == {(8, 1): 130, (8, 0): 65, (4, 1): 260, (4, 0): 65}
    got = {(d, e): (bool(vec), pieces, lpr, -(-pieces // lpr)) for e, d, vec, pieces, lpr, _ in rows}
    for key, want in ROWS.items():
        assert got[key] == want, key


def test_blocks_over_the_grid_are_aligned_disjoint_and_equal_the_inline_arithmetic(plan_exe):
    lines = plan_lines(plan_exe, "blocks", "cap=" + ",".join(map(str, CAPS)))
    assert [(e, d, cap) for e, d, cap, *_ in lines] == [(e, d, cap) for e in (8, 4) for d in range(1, 1025) for cap in CAPS]
    for e, d, cap, idx, logp, rows, total, gx in lines:
        key = (e, d, cap)
        assert (idx, logp, rows, total) == _earlier_block(cap, d, e), key
        lay = xr.Layout(cap, d, e)
        assert (idx, logp, rows, total) == (lay.idx, lay.logp, lay.rows, lay.bytes), key
        at = 0
        for name, first, used in lay.pieces():
            assert first % 16 == 0 and at <= first < at + 16, (key, name)  # aligned, behind the piece before, no more than padded
            at = first + used
        assert at <= total < at + 16 and total % 16 == 0, key
        # the scatter grid along x: workgroups of 256 / lpr slots, all of them needed
        rpb = _earlier_row(d, e)[3]
        assert gx == (cap + rpb - 1) // rpb and (gx - 1) * rpb < cap <= gx * rpb, key


def test_scatter_grid_covers_every_slot_and_every_peer_once(plan_exe):
    lines = plan_lines(plan_exe, "blocks", "cap=" + ",".join(map(str, CAPS)))
    by_lpr = {}
    for e, d, cap, *_rest, gx in lines:
        by_lpr.setdefault((_earlier_row(d, e)[2], cap), set()).add(gx)
    assert {k[0] for k in by_lpr} == {1, 2, 4, 8, 16, 32, 64}
    for (lpr, cap), gxs in by_lpr.items():
        assert len(gxs) == 1  # the grid depends on D and the element size through lanes per row alone
        gx, = gxs
        # thread t of workgroup b: slot b * (256 / lpr) + t / lpr, piece lane t % lpr -- as the kernel states it
        t = np.arange(256)
        slot = (np.arange(gx)[:, None] * (256 // lpr) + t[None, :] // lpr).ravel()
        sub = np.tile(t % lpr, gx)
        live = slot < cap
        pairs = slot[live] * 64 + sub[live]
        assert np.array_equal(np.sort(pairs), (np.arange(cap)[:, None] * 64 + np.arange(lpr)[None, :]).ravel()), (lpr, cap)
    ys = plan_lines(plan_exe, "scatter_y", "cap=" + ",".join(map(str, CAPS)))
    assert ys == [(ranks, ranks - 1) for ranks in range(2, 9)]
    for ranks, gy in ys:
        for rank in range(ranks):
            assert sorted(y + (1 if y >= rank else 0) for y in range(gy)) == [p for p in range(ranks) if p != rank]


def test_pack_and_sync_grids_cover_every_walker_of_the_slice_once(plan_exe):
    blocks = dict(plan_lines(plan_exe, "pack", "walkers=1200"))
    sync = dict(plan_lines(plan_exe, "sync", "shard=600"))
    n, sb = 700, 61
    for sc in range(1, 601):
        assert sync[sc] == (2 * sc + 255) // 256  # exchange_reset's launch
        i = np.arange(sync[sc] * 256)
        i = i[i < 2 * sc]
        assert np.array_equal((i // sc) * n + sb + i % sc, xr.slice_walkers(n, sb, sc)) and (sync[sc] - 1) * 256 < 2 * sc
        for colors in (1, 2):
            walkers = colors * sc
            pack_waves = (walkers + 16 - 1) // 16  # exchange_compact's launch
            assert blocks[walkers] == (pack_waves + 16 - 1) // 16
            # wavefront `wave` of the grid looks at walkers wave * 16 + lane, lane < 16, of the slice -- as the kernel states it
            i = (np.arange(blocks[walkers] * 16)[:, None] * 16 + np.arange(16)[None, :]).ravel()
            i = i[i < walkers]
            for color0 in range(0, 3 - colors):
                assert np.array_equal((color0 + i // sc) * n + sb + i % sc, xr.slice_walkers(n, sb, sc, color0, colors))
            assert (blocks[walkers] - 1) * 256 < walkers  # no idle workgroup


# --------------------------------------------------------------------------- CPU: the inputs have what they are there for

def test_rows_table_matches_the_restatement():
    for (d, e), (vec, pieces, lpr, trips) in ROWS.items():
        assert xr.row_pieces(d, e) == (vec, pieces) and xr.lanes_per_row(pieces) == lpr and xr.trips(d, e) == trips, (d, e)
    f64 = [d for d, e in ROWS if e == 8]
    f32 = [d for d, e in ROWS if e == 4]
    assert f64 == [1, 3, 2, 6, 64, 128, 130, 131, 1023, 1024] and f32 == [4, 5, 12, 256, 260, 1022, 1024]
    assert {xr.trips(d, e) for d, e in ROWS} == {1, 2, 3, 4, 8, 16}
    assert all(key in ROWS for key in TWO_ROWS)


def test_slices_are_what_they_are_named_for():
    sb, sc, c0, cs = ROW_SLICE
    walkers = sc * cs
    assert walkers == 406 and -(-walkers // 256) == 2 and walkers - 256 == 150 and 150 % 16 == 6
    assert {(sc * cs) for _, sc, _, cs in SLICES} >= {1, 2, 16, 32, 256, 257, 512, 514, 300, 600}  # one walker ... exact and ragged workgroups
    for sb, sc, c0, cs in SLICES:
        assert 0 <= sb and sb + sc <= N and 0 <= c0 and c0 + cs <= 2


def test_moved_sets_have_their_counts_and_their_caps():
    seen_kinds = set()
    for sb, sc, c0, cs in SLICES:
        S = xr.slice_walkers(N, sb, sc, c0, cs)
        for kind in MOVED_SETS:
            n_accept, seen = counters(kind, N, sb, sc, c0, cs)
            moved, seen_after, count = xr.pack(n_accept, seen, N, sb, sc, c0, cs)
            assert count == moved_count(kind, sc, c0, cs), (sb, sc, c0, cs, kind)
            assert np.all(seen <= MASK) and np.all(seen_after <= MASK)
            changed = np.flatnonzero(seen_after != seen)
            assert np.array_equal(changed, moved) and np.all(np.isin(moved, S))
            caps = caps_for(count, sc)
            assert {1, 7, 2 * sc} <= set(caps) and (count in caps or count == 0) and (count - 1 in caps or count <= 1)
            top_only = S[(n_accept[S] != seen[S]) & ((n_accept[S] & np.uint32(MASK)) == seen[S])]
            if kind == "top_bit_only":
                assert top_only.size == -(-S.size // 2) and count == 0        # they exist, and none of them moved
            if kind == "top_bit_and_low":
                assert np.all(n_accept[moved] & np.uint32(TOP)) and np.all(seen_after[moved] == n_accept[moved] & np.uint32(MASK))
            if kind in ("outside", "second_colour") and count == 0 and S.size < 2 * N:
                assert np.any(n_accept != seen)                              # counters did change, all outside the slice's colours
            if count > 7:
                seen_kinds.add(kind)
    assert seen_kinds == {"all", "third", "second_colour", "top_bit_and_low"}  # these overflow a cap of 7 (and of count - 1) somewhere


def test_scatter_inputs_have_their_counts_and_special_values():
    for (dims, elem) in ROWS:
        seen_counts = set()
        for rot in range(6):
            c = scatter_case(dims, elem, 3, 1, rot)
            cap, rpb = c["cap"], c["rpb"]
            seen_counts |= {c["counts"][p] for p in (0, 2)}
            assert c["counts"][1] == 3 and len(c["named"][1]) == 3
            everyone = np.concatenate([c["named"][p] for p in range(3)])
            assert len(set(everyone.tolist())) == everyone.size and c["spare"] not in everyone and everyone.max() < 2 * c["n"]
            v = xr.BlockView(c["blocks"], cap, dims, elem, 0)
            if c["counts"][0] >= cap:
                for special in SPECIALS[elem]:
                    assert special in v.logp.tolist() or cap < 28
                    assert special in v.rows.ravel().tolist() or cap * dims < 28
        assert seen_counts == {0, 1, rpb, rpb + 1, cap, cap + 2} and rpb + 1 < cap
    c = scatter_case(130, 8, 8, 3, 0, own_large=True)
    assert c["counts"][3] == max(c["counts"].values()) > c["cap"]
    specials = set(SPECIALS[8])
    assert specials <= set(xr.BlockView(c["blocks"], c["cap"], 130, 8, 0).rows.ravel().tolist())


def test_the_restatement_on_a_case_worked_by_hand():
    # n = 4: walkers 0..3 colour 0, 4..7 colour 1; the slice is walkers {1, 2} of each colour
    seen = np.array([5, 5, 5, 5, 5, 5, 5, MASK], np.uint32)
    n_accept = np.array([6, 6, 5 | TOP, 5, 5, 5, 7 | TOP, 0], np.uint32)
    moved, after, count = xr.pack(n_accept, seen, 4, 1, 2, 0, 2)
    assert moved.tolist() == [1, 6] and count == 2 and after.tolist() == [5, 6, 5, 5, 5, 5, 7, MASK]
    assert xr.pack(n_accept, seen, 4, 1, 2, 1, 1)[0].tolist() == [6]
    assert xr.sync_seen(n_accept, seen, 4, 0, 1).tolist() == [6, 5, 5, 5, 5, 5, 5, MASK]
    assert xr.sync_seen(n_accept, seen, 4, 3, 1).tolist() == [5, 5, 5, 5, 5, 5, 5, 0]
    lay = xr.Layout(7, 3, 8)  # 28 bytes of idx -> 32; 56 of logp -> 64; 168 of rows -> 176
    assert (lay.idx, lay.logp, lay.rows, lay.bytes) == (16, 48, 112, 288)
    # two ranks, this one is rank 1: rank 0's two rows arrive, rank 1's own do not; rank 0 packed 3 into 2 slots
    blocks = np.zeros(2 * xr.Layout(2, 1, 4).bytes, np.uint8)
    for p, (count, idx, logp, rows) in enumerate([(3, [2, 0], [10, 11], [20, 21]), (1, [1, 3], [12, 13], [22, 23])]):
        v = xr.BlockView(blocks, 2, 1, 4, p * xr.Layout(2, 1, 4).bytes)
        v.header[:] = (count, 2, 0, 0)
        v.idx[:], v.logp[:], v.rows[:, 0] = idx, logp, rows
    pos = np.arange(4, dtype=np.uint32).reshape(4, 1)
    logp = np.arange(4, dtype=np.uint32) + 100
    pa, pb, la, lb, stats, headers = xr.scatter(blocks, 2, 2, 1, 1, 4, pos, None, logp, logp, (0, 1))
    assert pa.ravel().tolist() == [21, 1, 20, 3] and pb is None and la.tolist() == lb.tolist() == [11, 101, 10, 103]
    assert stats == (1, 3) and headers[:, 0].tolist() == [3, 0]


# ------------------------------------------------------------------------------------------------------- GPU: sync_seen

@pytest.mark.gpu
def test_shim_lays_blocks_out_as_the_host_build_does(dev):
    for e in (8, 4):
        for d in (1, 5, 130, 1024):
            for cap in CAPS:
                assert dev.xd_block_bytes(cap, d, e) == xr.Layout(cap, d, e).bytes


@pytest.mark.gpu
@pytest.mark.parametrize("sb,sc", SLICE_RANGES)
def test_sync_seen(dev, sb, sc):
    for kind in ("all", "top_bit_and_low", "outside"):
        n_accept, seen = counters(kind, N, sb, sc, 0, 2)
        if kind == "outside":
            n_accept[xr.slice_walkers(N, sb, sc)[::2]] |= np.uint32(TOP)
        got = seen.copy()
        assert dev.xd_sync_seen(_p(n_accept), _p(got), N, sb, sc) == 0
        assert np.array_equal(got, xr.sync_seen(n_accept, seen, N, sb, sc)), kind


# ------------------------------------------------------------------------------------------------------------ GPU: pack

def run_pack(dev, elem, pos, logp, n_accept, seen, cap, n, dims, sb, sc, c0, cs, pattern=PATTERN):
    """-> (the buffer: block and guard, seen afterwards); the block holds `pattern` and a count of zero on entry"""
    buf = np.full(xr.Layout(cap, dims, elem).bytes + GUARD, pattern, np.uint8)
    buf[:4] = 0
    seen_after = seen.copy()
    rc = getattr(dev, "xd_pack_" + _t(elem))(_p(pos), _p(logp), _p(n_accept), _p(seen_after), _p(buf), buf.size, cap, n, dims, sb, sc, c0, cs)
    assert rc == 0, rc
    return buf, seen_after


def check_pack(buf, seen_after, elem, pos, logp, n_accept, seen, cap, n, dims, sb, sc, c0, cs, pattern=PATTERN):
    moved, want_seen, count = xr.pack(n_accept, seen, n, sb, sc, c0, cs)
    v = xr.BlockView(buf, cap, dims, elem)
    assert v.count == count                                  # on overflow too
    filled = min(count, cap)
    idx = v.idx[:filled].astype(np.int64)
    assert len(set(idx.tolist())) == filled and np.all(np.isin(idx, moved))
    if count <= cap:
        assert np.array_equal(np.sort(idx), moved)
    assert np.array_equal(v.logp[:filled], logp[idx])        # each slot's index, log-posterior and row are one walker's
    assert np.array_equal(v.rows[:filled], pos[idx])
    assert np.array_equal(seen_after, want_seen)
    # every byte but the count and the filled slots is as it was: the header's cap and padding, the slots from `filled` on, the
    # padding behind each array, and what lies behind the block
    lay = v.layout
    written = np.zeros(buf.size, bool)
    written[:4] = True
    written[lay.idx:lay.idx + 4 * filled] = True
    written[lay.logp:lay.logp + elem * filled] = True
    written[lay.rows:lay.rows + elem * dims * filled] = True
    assert np.all(buf[~written] == pattern), np.flatnonzero((buf != pattern) & ~written)[:8]
    return count


@pytest.mark.gpu
@pytest.mark.parametrize("dims,elem", list(ROWS), ids=ROW_IDS)
def test_pack_every_row_shape(dev, dims, elem):
    sb, sc, c0, cs = ROW_SLICE
    pos, logp = ensemble(N, dims, elem, 3)
    for kind, caps in (("third", lambda m: (m, 2 * sc)), ("all", lambda m: (7, m - 1))):
        n_accept, seen = counters(kind, N, sb, sc, c0, cs)
        m = moved_count(kind, sc, c0, cs)
        for cap in caps(m):
            args = (elem, pos, logp, n_accept, seen, cap, N, dims, sb, sc, c0, cs)
            assert check_pack(*run_pack(dev, *args), *args) == m


@pytest.mark.gpu
@pytest.mark.parametrize("dims,elem", TWO_ROWS, ids=["D6", "D130"])
@pytest.mark.parametrize("sb,sc,c0,cs", SLICES, ids=["%d+%d_c%d+%d" % s for s in SLICES])
def test_pack_every_slice_moved_set_and_cap(dev, dims, elem, sb, sc, c0, cs):
    pos, logp = ensemble(N, dims, elem, 4)
    for kind in MOVED_SETS:
        n_accept, seen = counters(kind, N, sb, sc, c0, cs)
        m = moved_count(kind, sc, c0, cs)
        for cap in caps_for(m, sc):
            args = (elem, pos, logp, n_accept, seen, cap, N, dims, sb, sc, c0, cs)
            assert check_pack(*run_pack(dev, *args), *args) == m, (kind, cap)


# --------------------------------------------------------------------------------------------------------- GPU: scatter

def run_scatter(dev, c, stats=(0, 0), second=(True, True)):
    """-> (blocks, pos_a, pos_b, logp_a, logp_b, stats) afterwards; second: whether pos_b / logp_b are given"""
    blocks, pos_a, logp_a = c["blocks"].copy(), c["pos_a"].copy(), c["logp_a"].copy()
    pos_b = c["pos_b"].copy() if second[0] else None
    logp_b = c["logp_b"].copy() if second[1] else None
    st = np.array(stats, np.uint32)
    rc = getattr(dev, "xd_scatter_" + _t(c["elem"]))(_p(blocks), c["cap"], c["ranks"], c["rank"], c["dims"], c["n"], _p(pos_a), _p(pos_b), _p(logp_a), _p(logp_b), _p(st))
    assert rc == 0, rc
    return blocks, pos_a, pos_b, logp_a, logp_b, (int(st[0]), int(st[1]))


def check_scatter(got, c, stats=(0, 0), second=(True, True)):
    blocks, pos_a, pos_b, logp_a, logp_b, st = got
    cap, ranks, rank, dims, elem = c["cap"], c["ranks"], c["rank"], c["dims"], c["elem"]
    want = xr.scatter(c["blocks"], cap, ranks, rank, dims, elem, c["pos_a"], c["pos_b"] if second[0] else None, c["logp_a"], c["logp_b"] if second[1] else None, stats)
    for name, a, b in zip(("pos_a", "pos_b", "logp_a", "logp_b"), (pos_a, pos_b, logp_a, logp_b), want[:4]):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), name
    # stated again without the restatement: what the peers name arrives, nothing else changes -- this rank's own rows least of all
    arrived = np.concatenate([c["named"][p] for p in range(ranks) if p != rank])
    stay = np.setdiff1d(np.arange(2 * c["n"]), arrived)
    assert np.all(np.isin(c["named"][rank], stay)) and c["spare"] in stay
    for a, before in ((pos_a, c["pos_a"]), (pos_b, c["pos_b"]), (logp_a, c["logp_a"]), (logp_b, c["logp_b"])):
        if a is not None:
            assert np.array_equal(a[stay], before[stay])
            assert arrived.size == 0 or not np.array_equal(a[arrived], before[arrived])
    counts = c["counts"]
    worst = max(counts.values())
    assert st == want[4] == (int(stats[0]) | int(worst > cap), max(int(stats[1]), worst))
    # the blocks: this rank's own count is zero, every other byte is as the all-gather left it
    bb = xr.Layout(cap, dims, elem).bytes
    headers = np.array([xr.BlockView(blocks, cap, dims, elem, p * bb).header for p in range(ranks)])
    assert np.array_equal(headers, want[5]) and headers[:, 0].tolist() == [0 if p == rank else counts[p] for p in range(ranks)]
    before = c["blocks"].copy()
    before[rank * bb:rank * bb + 4] = 0
    assert np.array_equal(blocks, before)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("dims,elem", list(ROWS), ids=ROW_IDS)
def test_scatter_every_row_shape(dev, dims, elem):
    for rot in range(6):
        c = scatter_case(dims, elem, 3, 1, rot, own_large=rot == 2)
        for second in ((True, True), (False, False)):
            check_scatter(run_scatter(dev, c, second=second), c, second=second)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,elem", TWO_ROWS + [(5, 4)], ids=["D6", "D130", "D5_f32"])
@pytest.mark.parametrize("ranks,rank", RANKS)
def test_scatter_every_rank_position_and_count(dev, dims, elem, ranks, rank):
    for rot in range(6):
        for own_large in (False, True):
            c = scatter_case(dims, elem, ranks, rank, rot, own_large=own_large)
            for second in ((True, True), (False, False), (True, False), (False, True)):
                st = check_scatter(run_scatter(dev, c, second=second), c, second=second)
            # the statistics stay raised over a second exchange with smaller blocks
            small = scatter_case(dims, elem, ranks, rank, rot, small=True)
            assert check_scatter(run_scatter(dev, small, stats=st), small, stats=st) == st
            assert check_scatter(run_scatter(dev, small), small) == (0, 1)


# ------------------------------------------------------------------------------------------------------ GPU: round trip

@pytest.mark.gpu
@pytest.mark.parametrize("dims,elem", [(130, 8), (5, 4)], ids=["D130", "D5_f32"])
def test_round_trip_pack_on_one_rank_scatter_on_another(dev, dims, elem):
    """Rank A packs its slice; its block goes where the all-gather would put it; rank B scatters.  B's copy of A's slice is then
    A's, in both buffers.  (No restatement takes part.)"""
    n, ranks, A, B = 301, 3, 2, 1
    sb, sc = 200, 101
    rng = np.random.default_rng(23)
    base_pos, base_logp = ensemble(n, dims, elem, 29)
    seen = rng.integers(0, 2 ** 31, 2 * n, dtype=np.uint32)
    S = xr.slice_walkers(n, sb, sc)
    movers = S[rng.random(S.size) < 0.4]
    assert 20 < movers.size < S.size - 20
    a_pos, a_logp, a_acc = base_pos.copy(), base_logp.copy(), seen.copy()
    a_pos[movers], a_logp[movers] = values(rng, (movers.size, dims), elem), values(rng, movers.size, elem)
    a_acc[movers] = ((seen[movers] + 1) & np.uint32(MASK)) | np.uint32(TOP)
    assert not np.array_equal(a_pos[movers], base_pos[movers])
    cap = 2 * sc
    # (a block of zeros: the slots the pack leaves alone then name walker 0, which the shim accepts and no rank may touch)
    buf, seen_after = run_pack(dev, elem, a_pos, a_logp, a_acc, seen, cap, n, dims, sb, sc, 0, 2, pattern=0)
    bb = xr.Layout(cap, dims, elem).bytes
    assert xr.BlockView(buf, cap, dims, elem).count == movers.size and np.array_equal(seen_after[S], a_acc[S] & np.uint32(MASK))
    gathered = np.zeros(ranks * bb, np.uint8)
    gathered[A * bb:(A + 1) * bb] = buf[:bb]
    own = xr.BlockView(gathered, cap, dims, elem, B * bb)   # B's own block: two of A's walkers with other rows -- must not arrive
    own.header[:2] = (2, cap)
    own.idx[:2] = movers[:2]
    own.rows[:2], own.logp[:2] = values(rng, (2, dims), elem), values(rng, 2, elem)
    xr.BlockView(gathered, cap, dims, elem, 0).header[:2] = (0, cap)
    c = dict(dims=dims, elem=elem, ranks=ranks, rank=B, cap=cap, n=n, blocks=gathered, pos_a=base_pos, pos_b=base_pos, logp_a=base_logp, logp_b=base_logp)
    _, pos_a, pos_b, logp_a, logp_b, st = run_scatter(dev, c)
    for got, want, before in ((pos_a, a_pos, base_pos), (pos_b, a_pos, base_pos), (logp_a, a_logp, base_logp), (logp_b, a_logp, base_logp)):
        assert np.array_equal(got[S], want[S])
        rest = np.setdiff1d(np.arange(2 * n), S)
        assert np.array_equal(got[rest], before[rest])
    assert st == (0, movers.size)
