// run_entry_cases.cpp -- prints the piece plans of the differential-evolution and the batch mover over a grid, and the verdict
// of the run entry for every combination of its facts (tests/test_run_entry.py).  Built with the host compiler against
// mcmcpp_amd/csrc/run_plan.hpp and run_refusal.hpp alone: that it compiles without HIP is part of the test.
//   run_entry_cases pieces step_bytes=a,b,.. n_saved=a,b,.. interval=a,b,.. budget=a,b,..
//     one line per mover (de, batch; de ignores the budget and is printed for the first one only) x step_bytes x n_saved x
//     interval x destination (0 none, 1 host, 2 device) x counters wanted: the plan's fields, pieces 0, 1 and the last, and
//     what a walk over every piece found (where it ended, how many pieces did not start where the one before ended, the
//     shortest and the longest piece)
//   run_entry_cases refusals
//     one line per mover x entry point x combination of the six facts: the refusal's name and its code
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "run_plan.hpp"
#include "run_refusal.hpp"

using namespace mcmcpp;

static std::vector<long long> list_of(const char* text)
{
    std::vector<long long> v;
    for (const char* p = text; *p;)
    {
        char* end = nullptr;
        v.push_back(std::strtoll(p, &end, 10));
        p = *end == ',' ? end + 1 : end;
    }
    return v;
}

static void print_plan(const char* mover, size_t budget, size_t step_bytes, int64_t n_saved, int32_t interval, int dest, int counters, const PiecePlan& p)
{
    int64_t at = 0, gaps = 0, shortest = -1, longest = 0;
    for (int64_t c = 0; c < p.n_pieces; ++c)
    {
        const StoredRange r = p.piece(c);
        if (r.from != at) ++gaps;
        const int64_t len = r.to - r.from;
        if (shortest < 0 || len < shortest) shortest = len;
        if (len > longest) longest = len;
        at = r.to;
    }
    const StoredRange none = {-1, -1};
    const StoredRange p0 = p.n_pieces > 0 ? p.piece(0) : none, p1 = p.n_pieces > 1 ? p.piece(1) : none, pl = p.n_pieces > 0 ? p.piece(p.n_pieces - 1) : none;
    std::printf("mover=%s budget=%zu step_bytes=%zu n_saved=%lld interval=%d dest=%d counters=%d piece_saved=%lld n_pieces=%lld chain_bytes=%zu acc_entries=%zu "
                "p0=%lld:%lld p1=%lld:%lld last=%lld:%lld walk_end=%lld gaps=%lld shortest=%lld longest=%lld\n",
                mover, budget, step_bytes, (long long)n_saved, (int)interval, dest, counters, (long long)p.piece_saved, (long long)p.n_pieces, p.chain_bytes, p.acc_entries,
                (long long)p0.from, (long long)p0.to, (long long)p1.from, (long long)p1.to, (long long)pl.from, (long long)pl.to, (long long)at, (long long)gaps, (long long)shortest,
                (long long)longest);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "pieces")
    {
        std::vector<long long> step_bytes, n_saved, interval, budget;
        for (int i = 2; i < argc; ++i)
        {
            const char* eq = std::strchr(argv[i], '=');
            if (!eq) return 2;
            const std::string key(argv[i], (size_t)(eq - argv[i]));
            (key == "step_bytes" ? step_bytes : key == "n_saved" ? n_saved : key == "interval" ? interval : budget) = list_of(eq + 1);
        }
        for (size_t b = 0; b < budget.size(); ++b)
            for (long long sb : step_bytes)
                for (long long ns : n_saved)
                    for (long long iv : interval)
                        for (int dest = 0; dest < 3; ++dest)
                            for (int counters = 0; counters < 2; ++counters)
                            {
                                if (b == 0)
                                    print_plan("de", 0, (size_t)sb, ns, (int32_t)iv, dest, counters, plan_de_pieces((size_t)sb, ns, (int32_t)iv, dest != 0, dest == 2, counters != 0));
                                print_plan("batch", (size_t)budget[b], (size_t)sb, ns, (int32_t)iv, dest, counters,
                                           plan_batch_pieces((size_t)budget[b], (size_t)sb, ns, (int32_t)iv, dest != 0, dest == 2, counters != 0));
                            }
        // where a piece lands: DE's piece in the caller's device array, a batch sub-chunk's slot base
        std::printf("device_piece_offset=%zu subchunk_slot_base=%lld\n", device_piece_offset(1000, 15), (long long)subchunk_slot_base(6));
        return 0;
    }
    if (what == "refusals")
    {
        static const char* const movers[] = {"stretch", "de", "batch"};
        static const char* const names[] = {"none", "device_with_communicator", "device_sharded", "no_callback", "no_state", "bad_arguments", "sharded", "half_done"};
        for (int m = 0; m < 3; ++m)
            for (int to_device = 0; to_device < 2; ++to_device)
                for (int bits = 0; bits < 64; ++bits)
                {
                    RunFacts f = {};
                    f.mover = (Mover)m;
                    f.to_device = to_device != 0;
                    f.have_state = (bits & 1) != 0, f.callback_set = (bits & 2) != 0, f.communicator = (bits & 4) != 0;
                    f.sharded = (bits & 8) != 0, f.half_done = (bits & 16) != 0, f.bad_arguments = (bits & 32) != 0;
                    const RunRefusal r = run_refusal(f);
                    std::printf("mover=%s to_device=%d have_state=%d callback_set=%d communicator=%d sharded=%d half_done=%d bad_arguments=%d refusal=%s code=%d collective=%d text=%d\n",
                                movers[m], to_device, (int)f.have_state, (int)f.callback_set, (int)f.communicator, (int)f.sharded, (int)f.half_done, (int)f.bad_arguments,
                                names[(int)r], run_refusal_code(r), (int)run_is_collective(f), (int)(run_refusal_text(r)[0] != 0));
                }
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
