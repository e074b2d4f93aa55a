"""How the histogram kernels are launched for one chunk of samples: the plan of mcmcpp_amd/csrc/hist_plan.hpp, checked on the CPU.
The GPU suite reaches this arithmetic only at the shapes its cases happen to use, and one part of it -- the split of the pair
launch at 65 535 tiles along grid.y, which needs 4.3 GB of counters and more -- at none: a mistake there gives pairs counted twice
or never, or a launch the runtime refuses.

tests/cpp/hist_plan_cases.cpp is compiled with the host compiler against hist_plan.hpp alone (no HIP header: that it compiles is
an assertion) and prints plans.  _earlier_plan below is a transcription of the arithmetic count_pass_t, bounds_pass,
steps_per_chunk and mcmcpp_hip_histograms_create held inline before it moved into the header, operation for operation (the
kernels index samples with 32-bit unsigned numbers; nothing in it wraps below 2^31 samples, which the transcription asserts).
The header has to reproduce it over the whole grid, and every plan has to cover every sample and every pair exactly once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

NS = [1, 255, 256, 257, 1024, 9000, 50000, 2 ** 31 - 1]
PS = [1, 2, 33, 46, 47, 92, 257, 258, 363, 1000]
BINS = [2, 4, 90, 91, 128, 129, 256, 257, 16384, 16385, 65536, 65537]
CUS = [1, 256, 304]
LDS = 65536
GRID_Y = 65535
U32 = 2 ** 32


def build_driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "hist_plan_cases")
    # the host compiler alone, and no include path but the header's own directory: hist_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "hist_plan_cases.cpp"), "-I", CSRC])
    return exe


def parse_plans(lines):
    """pairs of lines of the driver -> dicts of integers, `launches` a list of (t0, now, q0)"""
    assert len(lines) % 2 == 0
    plans = []
    for head, tail in zip(lines[::2], lines[1::2]):
        p = {k: int(v) for k, v in (f.split("=") for f in head.split())}
        assert tail.startswith("launches=")
        p["launches"] = [tuple(int(x) for x in l.split(":")) for l in tail[len("launches="):].split(",") if l]
        plans.append(p)
    return plans


def plan_of(exe, **args):
    out = subprocess.run([exe, "plan"] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout
    return parse_plans(out.strip().split("\n"))[0]


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def _earlier_plan(n, P, bins, pairs, cus, lds_limit):
    """the inline arithmetic of histograms.hip before hist_plan.hpp, for n >= 1 samples"""
    def u32(v):
        assert 0 <= v < U32, "a 32-bit sample count wrapped"
        return v

    out = dict(n=n, P=P, bins=bins, pairs=pairs, cus=cus, lds=lds_limit)
    # mcmcpp_hip_histograms_create
    npairs = P * (P - 1) // 2 if pairs else 0
    out["idx_bytes"] = 1 if bins <= 256 else (2 if bins <= 65536 else 4)
    # bounds_pass
    blocks = u32(cus * 2)
    if blocks > u32(n + 255) // 256:
        blocks = (n + 255) // 256
    per = u32(n + blocks - 1) // blocks
    blocks = u32(n + per - 1) // per
    out.update(bounds_blocks=blocks, bounds_per=per)
    # count_pass_t
    out["col"] = (n + 15) & ~15
    blocks = u32(n + 256 - 1) // 256
    if blocks > u32(cus * 8):
        blocks = cus * 8
    out["bin_blocks"] = blocks

    def slices_for(columns, flush_cells):
        want = (cus * 4 + columns - 1) // columns
        most = n // (flush_cells * 4 if flush_cells * 4 > 1024 else 1024)
        if want > most:
            want = most
        if want < 1:
            want = 1
        return u32(want)

    lds = 1 if bins * 4 <= lds_limit else 0
    slices = slices_for(P, bins if lds else 1)
    per = u32(n + slices - 1) // slices
    out.update(single_lds=lds, single_slices=slices, single_per=per, single_blocks=u32(n + per - 1) // per, single_lds_bytes=bins * 4 if lds else 0)
    out.update(npairs=npairs, pair_lds=0, tile=0, tiles=0, last_count=0, pair_slices=0, pair_per=0, pair_blocks=0, pair_lds_bytes=0, pair_launches=0,
               launches=[])
    if pairs and npairs > 0:
        b2 = bins * bins
        lds = 1 if b2 * 4 <= lds_limit else 0
        tile = lds_limit // (b2 * 4) if lds else 1
        if tile > 64:
            tile = 64
        while tile > 1 and (npairs + tile - 1) // tile < cus * 2:
            tile //= 2
        tiles = (npairs + tile - 1) // tile
        slices = slices_for(tiles, tile * b2 if lds else 1)
        per = u32(n + slices - 1) // slices
        launches = []
        for t0 in range(0, tiles, 65535):
            now = tiles - t0 if tiles - t0 < 65535 else 65535
            launches.append((t0, now, t0 * tile))
        out.update(pair_lds=lds, tile=tile, tiles=tiles, last_count=npairs - (tiles - 1) * tile, pair_slices=slices, pair_per=per,
                   pair_blocks=u32(n + per - 1) // per, pair_lds_bytes=tile * b2 * 4 if lds else 0, pair_launches=len(launches), launches=launches)
    return out


def _slices_cover(n, blocks, per):
    """block b of a kernel takes samples [b * per, min(n, (b + 1) * per)): every sample once, no block empty"""
    assert per >= 1 and blocks >= 1
    assert (blocks - 1) * per < n <= blocks * per
    assert blocks * per < U32  # blockIdx.x * per is a 32-bit product in the kernels


def _check(p):
    """what must hold for every plan, whatever its numbers"""
    n = p["n"]
    assert p["col"] >= n and p["col"] % 16 == 0 and p["col"] - n < 16
    _slices_cover(n, p["bounds_blocks"], p["bounds_per"])
    assert 1 <= p["bin_blocks"] <= (n + 255) // 256  # a grid-stride loop: any block count covers, none may be idle beyond the last
    _slices_cover(n, p["single_blocks"], p["single_per"])
    assert p["single_blocks"] <= p["single_slices"]
    assert p["single_lds_bytes"] == (p["bins"] * 4 if p["single_lds"] else 0) <= p["lds"]
    assert p["idx_bytes"] in (1, 2, 4) and p["bins"] - 1 < 256 ** p["idx_bytes"]  # the largest bin index fits its type
    if p["idx_bytes"] > 1:
        assert p["bins"] - 1 >= 256 ** (p["idx_bytes"] // 2)                      # and no narrower type would do
    if not p["npairs"]:
        assert p["launches"] == [] and p["pair_launches"] == 0
        assert p["npairs"] == 0
        return
    assert p["npairs"] == p["P"] * (p["P"] - 1) // 2
    b2 = p["bins"] ** 2
    tile, tiles = p["tile"], p["tiles"]
    _slices_cover(n, p["pair_blocks"], p["pair_per"])
    assert p["pair_blocks"] <= p["pair_slices"]
    assert 1 <= tile <= 64
    if p["pair_lds"]:
        assert tile * b2 * 4 <= p["lds"] and p["pair_lds_bytes"] == tile * b2 * 4
        assert tile * b2 < 2 ** 31  # `cells` is an int in the kernel
    else:
        assert b2 * 4 > p["lds"] and tile == 1 and p["pair_lds_bytes"] == 0
    # tiles cover the pairs once: all full but possibly the last
    assert (tiles - 1) * tile < p["npairs"] <= tiles * tile
    assert p["last_count"] == p["npairs"] - (tiles - 1) * tile and 1 <= p["last_count"] <= tile
    # the launches cover the tiles once, in order, each within grid.y; a launch sees pairs [q0, npairs) and `now` tiles of them
    assert len(p["launches"]) == p["pair_launches"] >= 1
    at = 0
    for t0, now, q0 in p["launches"]:
        assert t0 == at and 1 <= now <= GRID_Y and q0 == t0 * tile
        first, last = q0, min(p["npairs"], q0 + now * tile)  # the pairs this launch's blocks count
        assert first < last and (last == p["npairs"] or last == (t0 + now) * tile)
        at += now
    assert at == tiles


def test_hist_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "hist_plan.hpp")).read()
    includes = [line.split()[1] for line in text.split("\n") if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"]


def test_the_histogram_source_holds_no_launch_arithmetic():
    text = open(os.path.join(CSRC, "histograms.hip")).read()
    for gone in ("tile /= 2", "tile > 64", "t0 += 65535", "cus * 2", "cus * 4", "cus * 8", "+ 255) / 256", "+ 15) & ~", "flush_cells", "bins <= 256 ?",
                 "<= h->lds_limit", "(size_t)65536", "1 << 31", "slices_for", "(num_params - 1) / 2"):
        assert gone not in text, gone
    assert '#include "hist_plan.hpp"' in text and "hist_plan(" in text
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " hist_plan.hpp " in makefile.split("HDRS")[1].split("\n")[0]


def test_plan_over_the_grid_equals_the_inline_arithmetic_and_covers_everything_once(driver):
    args = ["n=" + ",".join(map(str, NS)), "P=" + ",".join(map(str, PS)), "bins=" + ",".join(map(str, BINS)), "cus=" + ",".join(map(str, CUS)), "lds=%d" % LDS]
    out = subprocess.run([driver, "grid"] + args, capture_output=True, text=True, check=True).stdout
    plans = parse_plans(out.strip().split("\n"))
    assert len(plans) == len(NS) * len(PS) * len(BINS) * len(CUS) * 2
    seen = set()
    for p in plans:
        key = (p["n"], p["P"], p["bins"], p["cus"], p["pairs"])
        seen.add(key)
        assert p == _earlier_plan(p["n"], p["P"], p["bins"], p["pairs"], p["cus"], LDS), key
        _check(p)
    assert seen == {(n, P, b, c, w) for n in NS for P in PS for b in BINS for c in CUS for w in (0, 1)}
    # the grid holds what it was chosen for
    tiles_seen = {p["tile"] for p in plans if p["npairs"]}
    assert tiles_seen >= {1, 2, 8, 64} and tiles_seen <= {1, 2, 4, 8, 16, 32, 64}
    assert any(p["pair_launches"] > 1 for p in plans) and any(p["npairs"] and not p["pair_lds"] for p in plans)
    assert any(p["npairs"] and p["last_count"] < p["tile"] for p in plans) and any(p["tile"] > 1 and p["last_count"] == p["tile"] for p in plans)
    assert any(not p["single_lds"] for p in plans) and any(p["single_blocks"] > 1 for p in plans) and any(p["pair_blocks"] > 1 for p in plans)


def test_a_smaller_lds_limit_bounds_the_tile(driver):
    # a device that offers 32 KiB: 90 x 90 counters (32 400 bytes) fit once, 91 x 91 (33 124 bytes) go to global memory
    for bins, lds, tile in ((90, 1, 1), (91, 0, 1), (4, 1, 64), (45, 1, 4)):
        p = plan_of(driver, n=9000, P=363, bins=bins, pairs=1, cus=256, lds=32768)
        assert p == _earlier_plan(9000, 363, bins, 1, 256, 32768)
        _check(p)
        assert (p["pair_lds"], p["tile"]) == (lds, tile)


def test_the_grid_y_split_of_65703_single_pair_tiles(driver):
    """P = 363, bins = 91: 65 703 pairs, one to a tile (two 91 x 91 histograms do not fit in LDS) -- 168 tiles past the grid.y limit.
    The second launch starts at pair 65 535: its pair table, its pair count and its counters are offset by that much."""
    p = plan_of(driver, n=600, P=363, bins=91, pairs=1, cus=256, lds=LDS)
    assert (p["npairs"], p["tile"], p["tiles"], p["pair_lds"]) == (65703, 1, 65703, 1)
    assert p["launches"] == [(0, 65535, 0), (65535, 168, 65535)]
    assert sum(now for _, now, _ in p["launches"]) == p["npairs"] and p["launches"][1][2] == p["launches"][0][1] * p["tile"]
    # with two pairs to a tile the same pairs need one launch; 499 500 single-pair tiles need eight, whose offsets still add up
    assert plan_of(driver, n=600, P=363, bins=90, pairs=1, cus=256, lds=LDS)["launches"] == [(0, 32852, 0)]
    p = plan_of(driver, n=600, P=1000, bins=91, pairs=1, cus=256, lds=LDS)
    assert p["launches"][:2] == [(0, 65535, 0), (65535, 65535, 65535)] and p["launches"][-1] == (7 * 65535, 499500 - 7 * 65535, 7 * 65535)
    _check(p)


@pytest.mark.parametrize("chunk_bytes,step_bytes,W,want", [
    (1 << 30, 2000 * 33 * 8, 2000, 2033),       # the chunk size bounds it
    (1 << 20, 2000 * 33 * 8, 2000, 1),          # one step at the least
    (1 << 20, 2000 * 33 * 4, 2000, 3),
    (1 << 40, 64 * 1 * 4, 64, 2 ** 25 - 1),     # 32-bit sample indexing bounds it: (2^25 - 1) x 64 samples < 2^31
    (1 << 40, 3 * 1 * 8, 3, 2 ** 31 // 3 - 1),
])
def test_steps_per_chunk(driver, chunk_bytes, step_bytes, W, want):
    out = subprocess.run([driver, "chunk", "chunk_bytes=%d" % chunk_bytes, "step_bytes=%d" % step_bytes, "W=%d" % W], capture_output=True, text=True, check=True)
    k = int(out.stdout)
    cap = (1 << 31) // W - 1
    assert k == want == max(1, min(chunk_bytes // step_bytes, cap))  # the inline arithmetic of steps_per_chunk
    assert k * W < 2 ** 31


def test_lds_limit_of_a_device(driver):
    for shared, want in ((65536, 65536), (163840, 65536), (32768, 32768)):
        assert int(subprocess.run([driver, "lds", "shared=%d" % shared], capture_output=True, text=True, check=True).stdout) == want
