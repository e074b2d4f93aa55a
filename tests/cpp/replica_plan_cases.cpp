// replica_plan_cases.cpp -- mcmcpp_amd/csrc/replica_plan.hpp exercised on the CPU (tests/test_replica_plan.py).  Built with the
// host compiler against the header alone: that it compiles without a HIP header is an assertion.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <vector>

#include "replica_plan.hpp"

using namespace mcmcpp;

static double from_bits(uint64_t b)
{
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string_view what = argv[1];
    if (what == "pairs")  // K round slot lower_chain
    {
        for (int K = 2; K <= 16; ++K)
            for (uint64_t r = 0; r < 4; ++r)
                for (int j = 0; j < replica_pairs(K, r); ++j) std::printf("%d %" PRIu64 " %d %d %d\n", K, r, j, replica_lower_chain(r, j), replica_slot_of(replica_lower_chain(r, j)));
        return 0;
    }
    if (what == "positions" && argc == 3)  // W -> round slot w position, for all 8 slots
    {
        const int W = std::atoi(argv[2]);
        const uint64_t rounds[3] = {0, 1, kReplicaMaxRound - 1};
        for (uint64_t r : rounds)
            for (int j = 0; j < kReplicaMaxSlots; ++j)
                for (int w = 0; w < W; ++w) std::printf("%" PRIu64 " %d %d %" PRIu64 "\n", r, j, w, replica_draw_position(r, j, W, w));
        return 0;
    }
    if (what == "accept")  // stdin: draw and the bit patterns of lp_aa lp_bb lp_ab lp_ba -> accept near_tie
    {
        uint64_t d, b[4];
        while (std::scanf("%" SCNu64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &d, &b[0], &b[1], &b[2], &b[3]) == 5)
        {
            bool tie = false;
            const bool acc = replica_accept(d, from_bits(b[0]), from_bits(b[1]), from_bits(b[2]), from_bits(b[3]), &tie);
            std::printf("%d %d\n", acc ? 1 : 0, tie ? 1 : 0);
        }
        return 0;
    }
    if (what == "table" && argc == 7)  // seed stream W round slot -> entries, then per walker: state_hi state_lo draw
    {
        const uint64_t seed = std::strtoull(argv[2], nullptr, 10), stream = std::strtoull(argv[3], nullptr, 10), round = std::strtoull(argv[5], nullptr, 10);
        const int W = std::atoi(argv[4]), slot = std::atoi(argv[6]);
        ReplicaU128 state0, inc;
        replica_seed(seed, stream, &state0, &inc);
        std::vector<ReplicaJump> t((size_t)replica_table_entries(W));
        replica_fill_table(inc, W, t.data());
        const ReplicaU128 base = replica_slot_base(state0, inc, round, slot, W);
        std::printf("%d %" PRIu64 " %" PRIu64 "\n", replica_table_entries(W), inc.hi, inc.lo);
        for (int w = 0; w < W; ++w)
        {
            const ReplicaU128 s = replica_apply(t[(size_t)(w & 63)], replica_apply(t[(size_t)(kReplicaLaneEntries + (w >> 6))], base));
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s.hi, s.lo, replica_draw(t.data(), base, w));
        }
        return 0;
    }
    if (what == "shape" && argc == 7)  // W D elem_size vec_ok pairs
    {
        const ReplicaShape s = replica_shape(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
        std::printf("%d %d %d %d %u %u\n", s.lanes, s.units, s.unit_bytes, s.walkers_per_block, s.grid_x, s.grid_y);
        return 0;
    }
    return 2;
}
