// temper_plan_cases.cpp -- prints what mcmcpp_amd/csrc/temper_plan.hpp decides, for tests/test_temper_plan.py.  Compiled with
// the host compiler against the plan header alone (no HIP header on the include path).
//   pieces FIRST_ROUND   every (total <= 24, every <= 8, split of total into two or three enqueue calls): one line
//                        "total every c1 c2 c3 : steps/follows/round ..." with the pieces in the order the run enqueues them
//                        (c3 = 0: two calls, c2 = 0: one); the pieces of a call are asked with `left` = what is left of that call
//   counts TOTAL EVERY FIRST_ROUND K     "rounds" and the number of rounds that pair (k, k + 1), k = 0 .. K - 2
//   refusal TOTAL EVERY FIRST_ROUND K    the refusal as a number and its text
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "temper_plan.hpp"

using namespace mcmcpp;

static void print_pieces(const TemperSchedule& s, const int64_t* calls, int n_calls)
{
    int64_t run_step = 0;
    std::printf("%lld %lld %lld %lld %lld :", (long long)s.total, (long long)s.every, (long long)calls[0], (long long)(n_calls > 1 ? calls[1] : 0),
                (long long)(n_calls > 2 ? calls[2] : 0));
    for (int c = 0; c < n_calls; ++c)
        for (int64_t left = calls[c]; left > 0;)
        {
            const TemperPiece p = temper_next_piece(s, run_step, left);
            std::printf(" %lld/%d/%llu", (long long)p.steps, p.round_follows ? 1 : 0, (unsigned long long)(p.round_follows ? p.round : 0));
            if (p.steps < 1 || p.steps > left) std::abort();  // (the loop must end)
            left -= p.steps;
            run_step += p.steps;
        }
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "pieces"))
    {
        TemperSchedule s = {};
        s.first_round = std::strtoull(argv[2], nullptr, 10);
        s.K = 4;
        for (s.total = 1; s.total <= 24; ++s.total)
            for (s.every = 1; s.every <= 8; ++s.every)
            {
                print_pieces(s, &s.total, 1);
                for (int64_t a = 1; a < s.total; ++a)
                {
                    const int64_t two[2] = {a, s.total - a};
                    print_pieces(s, two, 2);
                    for (int64_t b = 1; a + b < s.total; ++b)
                    {
                        const int64_t three[3] = {a, b, s.total - a - b};
                        print_pieces(s, three, 3);
                    }
                }
            }
        return 0;
    }
    if (argc == 6)
    {
        TemperSchedule s = {};
        s.total = std::strtoll(argv[2], nullptr, 10);
        s.every = std::strtoll(argv[3], nullptr, 10);
        s.first_round = std::strtoull(argv[4], nullptr, 10);
        s.K = std::atoi(argv[5]);
        if (!std::strcmp(argv[1], "counts"))
        {
            std::printf("%lld", (long long)temper_rounds(s));
            for (int k = 0; k + 1 < s.K; ++k) std::printf(" %lld", (long long)temper_rounds_pairing(s, k));
            std::printf("\n");
            return 0;
        }
        if (!std::strcmp(argv[1], "refusal"))
        {
            const TemperRefusal r = temper_refusal(s);
            std::printf("%d %s\n", (int)r, temper_refusal_text(r));
            return 0;
        }
    }
    std::fprintf(stderr, "usage: temper_plan_cases pieces FIRST_ROUND | counts|refusal TOTAL EVERY FIRST_ROUND K\n");
    return 2;
}
