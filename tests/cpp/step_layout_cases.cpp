// step_layout_cases.cpp -- answers questions about the packed launch words and the per-chain strides (tests/test_step_layout.py).
// Built with the host compiler against mcmcpp_amd/csrc/step_layout.hpp alone: that it compiles without HIP is part of the test.
// One question per line of standard input, one answer per line of output:
//   hot dims passes colour vec_ok n_is_pow2 use_ctl_save draw_parity draw_wave pos_parity direct_jump chains
//                                        -> the packed word and every field decoded from it, in that order
//   de dims colour vec_ok step           -> likewise for DeHotBits
//   tables n direct chains               -> tables_offset_task, _hi, _lo, tables_total_bytes
//   logp n                               -> logp_chain_stride_bytes<double>, <float>
//   drawbuf parity colour n              -> draw_buffer_index
//   partial chain slots slot colour waves wave -> partial_index
//   consts                               -> kCtlChainStride kRunBehindCtlBytes kMaxChains kDrawRecBytes
#include <cstdio>
#include <cstring>

#include "step_layout.hpp"

using namespace mcmcpp;

int main()
{
    char line[256], cmd[32];
    while (std::fgets(line, sizeof line, stdin))
    {
        long v[11] = {};
        const int got = std::sscanf(line, "%31s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", cmd, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10);
        if (got < 1) continue;
        const int have = got - 1;
        if (!std::strcmp(cmd, "hot") && have == 11)
        {
            const uint32_t b = HotBits::pack((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9], (int)v[10]);
            std::printf("0x%08X %d %d %d %d %d %d %d %d %d %d %d\n", (unsigned)b, HotBits::dims(b), HotBits::passes(b), HotBits::color(b), HotBits::vec_ok(b),
                        HotBits::n_is_pow2(b), HotBits::use_ctl_save(b), HotBits::draw_parity(b), HotBits::draw_wave(b), HotBits::pos_parity(b), HotBits::direct_jump(b),
                        HotBits::chains(b));
        }
        else if (!std::strcmp(cmd, "de") && have == 4)
        {
            const uint32_t b = DeHotBits::pack((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
            std::printf("0x%08X %d %d %d %d\n", (unsigned)b, DeHotBits::dims(b), DeHotBits::color(b), DeHotBits::vec_ok(b), DeHotBits::step(b));
        }
        else if (!std::strcmp(cmd, "tables") && have == 3)
            std::printf("%zu %zu %zu %zu\n", tables_offset_task((int)v[0], (int)v[2]), tables_offset_hi((int)v[0], v[1] != 0, (int)v[2]),
                        tables_offset_lo((int)v[0], v[1] != 0, (int)v[2]), tables_total_bytes((int)v[0], v[1] != 0, (int)v[2]));
        else if (!std::strcmp(cmd, "logp") && have == 1)
            std::printf("%zu %zu\n", logp_chain_stride_bytes<double>((int)v[0]), logp_chain_stride_bytes<float>((int)v[0]));
        else if (!std::strcmp(cmd, "drawbuf") && have == 3)
            std::printf("%zu\n", draw_buffer_index((int)v[0], (int)v[1], (int)v[2]));
        else if (!std::strcmp(cmd, "partial") && have == 6)
            std::printf("%zu\n", partial_index((int)v[0], (int)v[1], (uint32_t)v[2], (int)v[3], (int)v[4], (int)v[5]));
        else if (!std::strcmp(cmd, "consts") && have == 0)
            std::printf("%d %d %d %zu\n", kCtlChainStride, kRunBehindCtlBytes, kMaxChains, kDrawRecBytes);
        else
            return 2;
    }
    return 0;
}
