"""The packed launch words and the per-chain strides of mcmcpp_amd/csrc/step_layout.hpp, pinned on the CPU.

The step kernels and the host agree on two 32-bit words (HotBits: the stretch kernels' hot_bits; DeHotBits: the
differential-evolution update kernels') and on the strides of every per-chain array (ChainGeometry).  A field that moves, or
an offset that changes, moves on both sides at once, so no GPU test would see it unless a kernel faulted; this test does.

tests/cpp/step_layout_cases.cpp is compiled with the host compiler against step_layout.hpp alone (no HIP header: that it
compiles is an assertion) and answers one question per line.  The expected numbers are literals worked out by hand from the
layout comment in the header:
    draw records 4 n x 32 B per chain | task_jump 3 n x 32 B, if built | jump_hi ceil(n / 256) x 32 B | jump_lo 256 x 32 B,
    every piece rounded up to 256 bytes;   log-posteriors + counters: [2][2n] T, [2n] u32 = 40 n bytes (fp64), 24 n (fp32)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")

# field: (smallest, largest), in the order of HotBits::pack's arguments and of the driver's answer
HOT_FIELDS = [("dims", 0, 4095), ("passes", 0, 255), ("color", 0, 1), ("vec_ok", 0, 1), ("n_is_pow2", 0, 1), ("use_ctl_save", 0, 1),
              ("draw_parity", 0, 1), ("draw_wave", 0, 1), ("pos_parity", 0, 1), ("direct_jump", 0, 1), ("chains", 1, 16)]
DE_FIELDS = [("dims", 0, 4095), ("color", 0, 1), ("vec_ok", 0, 1), ("step", 0, 65535)]

# (n, task table built, chains) -> tables_offset_task, tables_offset_hi, tables_offset_lo, tables_total_bytes
TABLES = {
    # n = 100: records 12 800; task table 9 600 -> 9 728; jump_hi 1 entry -> 256; jump_lo 8 192
    (100, 1, 1): (12800, 22528, 22784, 30976),
    (100, 0, 1): (12800, 12800, 13056, 21248),
    (100, 1, 3): (38400, 48128, 48384, 56576),
    (100, 0, 3): (38400, 38400, 38656, 46848),
    (100, 1, 16): (204800, 214528, 214784, 222976),
    (100, 0, 16): (204800, 204800, 205056, 213248),
    # n = 256: records 32 768; task table 24 576; jump_hi 1 entry -> 256
    (256, 1, 1): (32768, 57344, 57600, 65792),
    (256, 0, 1): (32768, 32768, 33024, 41216),
    (256, 1, 3): (98304, 122880, 123136, 131328),
    (256, 0, 3): (98304, 98304, 98560, 106752),
    (256, 1, 16): (524288, 548864, 549120, 557312),
    (256, 0, 16): (524288, 524288, 524544, 532736),
    # n = 257: records 32 896 -> 33 024 (one chain), 98 688 -> 98 816 (three), 526 336 (sixteen); task table 24 672 -> 24 832;
    #          jump_hi 2 entries -> 256
    (257, 1, 1): (33024, 57856, 58112, 66304),
    (257, 0, 1): (33024, 33024, 33280, 41472),
    (257, 1, 3): (98816, 123648, 123904, 132096),
    (257, 0, 3): (98816, 98816, 99072, 107264),
    (257, 1, 16): (526336, 551168, 551424, 559616),
    (257, 0, 16): (526336, 526336, 526592, 534784),
    # n = 70 000: records 8 960 000; task table 6 720 000; jump_hi 274 entries = 8 768 -> 8 960
    (70000, 1, 1): (8960000, 15680000, 15688960, 15697152),
    (70000, 0, 1): (8960000, 8960000, 8968960, 8977152),
    (70000, 1, 3): (26880000, 33600000, 33608960, 33617152),
    (70000, 0, 3): (26880000, 26880000, 26888960, 26897152),
    (70000, 1, 16): (143360000, 150080000, 150088960, 150097152),
    (70000, 0, 16): (143360000, 143360000, 143368960, 143377152),
}
LOGP = {100: (4000, 2400), 256: (10240, 6144), 257: (10280, 6168), 70000: (2800000, 1680000)}
# (parity, colour, n) -> first record of that buffer: (parity * 2 + colour) * n
DRAWBUF = {(0, 0, 100): 0, (0, 1, 100): 100, (1, 0, 100): 200, (1, 1, 100): 300,
           (0, 0, 256): 0, (0, 1, 256): 256, (1, 0, 256): 512, (1, 1, 256): 768,
           (0, 0, 257): 0, (0, 1, 257): 257, (1, 0, 257): 514, (1, 1, 257): 771,
           (0, 0, 70000): 0, (0, 1, 70000): 70000, (1, 0, 70000): 140000, (1, 1, 70000): 210000}
# (chain, slots, slot, colour, waves, wave) -> ((chain * slots + slot) * 2 + colour) * waves + wave; chains of 1, 3 and 16: the last one
PARTIAL = {
    (0, 300, 299, 1, 1024, 1023): 614399,     # 599 * 1024 + 1023
    (2, 300, 299, 1, 1024, 1023): 1843199,    # 1799 * 1024 + 1023
    (15, 300, 299, 1, 1024, 1023): 9830399,   # 9599 * 1024 + 1023
    (1, 7, 3, 0, 36, 5): 725,                 # 20 * 36 + 5
    (0, 1, 0, 0, 4096, 0): 0,
    (15, 300, 299, 1, 1 << 20, 5): 10065281029,  # 9599 * 2^20 + 5: beyond 32 bits
}


def _hot_cases():
    """Every field at its smallest and its largest value, with all other fields at their smallest and at their largest."""
    cases = []
    for k, (_, lo, hi) in enumerate(HOT_FIELDS):
        for mine in (lo, hi):
            for others in (1, 2):
                cases.append(tuple(mine if j == k else f[others] for j, f in enumerate(HOT_FIELDS)))
    return cases


def _de_cases():
    cases = []
    for k, (_, lo, hi) in enumerate(DE_FIELDS):
        for mine in (lo, hi):
            for others in (1, 2):
                cases.append(tuple(mine if j == k else f[others] for j, f in enumerate(DE_FIELDS)))
    return cases


HOT_PINNED = (32, 2, 1, 1, 1, 1, 1, 1, 1, 1, 16)
DE_PINNED = (32, 1, 1, 299)


@pytest.fixture(scope="module")
def answers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "step_layout_cases")
    # the host compiler alone, and no include path but the header's own directory: step_layout.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "step_layout_cases.cpp"), "-I", CSRC])
    questions = ([("hot",) + c for c in _hot_cases() + [HOT_PINNED]] + [("de",) + c for c in _de_cases() + [DE_PINNED]] + [("tables",) + k for k in TABLES]
                 + [("logp", n) for n in LOGP] + [("drawbuf",) + k for k in DRAWBUF] + [("partial",) + k for k in PARTIAL] + [("consts",)])
    text = "".join(" ".join(str(x) for x in q) + "\n" for q in questions)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(questions) + 1 and out[-1] == ""
    return {q: tuple(int(x, 0) for x in line.split()) for q, line in zip(questions, out)}


def test_step_layout_header_includes_no_hip_header():
    def includes(name):
        return [line.split()[1] for line in open(os.path.join(CSRC, name)).read().split("\n") if line.startswith("#include")]
    assert includes("step_layout.hpp") == ["<stddef.h>", "<stdint.h>", '"canonical.hpp"', '"step_plan.hpp"']
    assert includes("canonical.hpp") == ["<stdint.h>"]
    # (step_plan.hpp: tests/test_step_plan.py)


def test_hot_bits_fields_round_trip(answers):
    cases = _hot_cases()
    assert len(cases) == 4 * len(HOT_FIELDS)
    for c in cases:
        assert answers[("hot",) + c][1:] == c, c
    # no field at its largest leaves a bit unset, none at its smallest sets one
    assert answers[("hot",) + tuple(f[2] for f in HOT_FIELDS)][0] == 0xFFFFFFFF
    assert answers[("hot",) + tuple(f[1] for f in HOT_FIELDS)][0] == 0


def test_de_hot_bits_fields_round_trip(answers):
    cases = _de_cases()
    assert len(cases) == 4 * len(DE_FIELDS)
    for c in cases:
        assert answers[("de",) + c][1:] == c, c
    assert answers[("de",) + tuple(f[2] for f in DE_FIELDS)][0] == 0xFFFF5FFF  # (bits 13 and 15 are unused)
    assert answers[("de",) + tuple(f[1] for f in DE_FIELDS)][0] == 0


def test_packed_literals_are_pinned(answers):
    assert answers[("hot",) + HOT_PINNED][0] == 0xFFF02020
    assert answers[("de",) + DE_PINNED][0] == 0x012B5020
    assert answers[("consts",)] == (512, 256, 16, 32)


def test_table_offsets(answers):
    for key, want in TABLES.items():
        assert answers[("tables",) + key] == want, key


def test_logp_stride(answers):
    for n, want in LOGP.items():
        assert answers[("logp", n)] == want, n


def test_record_buffer_index(answers):
    for key, want in DRAWBUF.items():
        assert answers[("drawbuf",) + key] == (want,), key


def test_partial_index(answers):
    for key, want in PARTIAL.items():
        assert answers[("partial",) + key] == (want,), key
