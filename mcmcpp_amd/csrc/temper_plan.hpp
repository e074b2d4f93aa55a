// temper_plan.hpp -- the schedule of a tempered run (mcmcpp_hip_run_tempered): a run of the K chains of one handle whose
// replica-exchange rounds (replica_plan.hpp) lie inside its launch sequence.  This header decides
//   where the step launches are cut     a piece ends at the next multiple of exchange_every, counted in ensemble steps from the
//                                       start of the run, or where the caller stops enqueueing, whichever comes first
//   whether a round follows a piece     exactly when the run has reached a multiple of exchange_every: a run that ends on one
//                                       still exchanges, a shorter tail does not (the rule of HipSampler.run_exchanging)
//   the round's number                  first_round + run_step / exchange_every - 1, run_step counted behind the piece
//   the counters that need no device    rounds of the run, and how many of them pair (k, k + 1): proposed[k] = W x that count
//   what only a tempered run refuses    exchange_every < 1, K < 2, first_round + rounds > kReplicaMaxRound
// exchange_every counts ensemble steps and need not be a multiple of the storing interval: the trajectory does not depend on
// which steps are stored.
//
// Plain C++ (no HIP header), like run_plan.hpp and replica_plan.hpp: tests/cpp/temper_plan_cases.cpp compiles it with the
// host compiler alone.
#pragma once

#include <stdint.h>

#include "replica_plan.hpp"

namespace mcmcpp
{

struct TemperSchedule
{
    int64_t total;         // ensemble steps of the run
    int64_t every;         // exchange_every
    uint64_t first_round;  // the number of the run's first round
    int K;                 // chains of the handle
};

enum class TemperRefusal { None, BadEvery, OneChain, RoundOutOfRange };

MCMCPP_HD int64_t temper_rounds(const TemperSchedule& s) { return s.every >= 1 && s.total > 0 ? s.total / s.every : 0; }

// the first check that fails (the run's own refusals, run_refusal.hpp, come in front of these)
MCMCPP_HD TemperRefusal temper_refusal(const TemperSchedule& s)
{
    if (s.every < 1) return TemperRefusal::BadEvery;
    if (s.K < 2) return TemperRefusal::OneChain;
    // (rounds <= 2^63 / every: the sum cannot wrap once first_round itself is in range)
    if (s.first_round > kReplicaMaxRound || s.first_round + (uint64_t)temper_rounds(s) > kReplicaMaxRound) return TemperRefusal::RoundOutOfRange;
    return TemperRefusal::None;
}

inline const char* temper_refusal_text(TemperRefusal r)
{
    switch (r)
    {
    case TemperRefusal::BadEvery: return "exchange_every must be at least 1";
    case TemperRefusal::OneChain: return "the handle has one chain (num_chains must be at least 2)";
    case TemperRefusal::RoundOutOfRange: return "the run's last round is out of range (rounds are below 2^40)";
    default: return "";
    }
}

// The next piece of step launches, seen from run_step (ensemble steps enqueued in this run so far) with `left` > 0 steps
// still to enqueue now.
struct TemperPiece
{
    int64_t steps;       // 1 .. left
    bool round_follows;  // the piece ends on an exchange point
    uint64_t round;      // (round_follows) that round's number
};
MCMCPP_HD TemperPiece temper_next_piece(const TemperSchedule& s, int64_t run_step, int64_t left)
{
    TemperPiece p;
    const int64_t to_point = s.every - run_step % s.every;  // 1 .. every
    p.steps = left < to_point ? left : to_point;
    p.round_follows = p.steps == to_point;
    p.round = s.first_round + (uint64_t)((run_step + p.steps) / s.every) - 1u;
    return p;
}

// how many rounds of the run pair chains (k, k + 1): those whose number has k's parity
MCMCPP_HD int64_t temper_rounds_pairing(const TemperSchedule& s, int k)
{
    if (k < 0 || k + 1 >= s.K) return 0;
    const int64_t rounds = temper_rounds(s);
    const bool first_matches = ((s.first_round ^ (uint64_t)k) & 1u) == 0;
    return first_matches ? (rounds + 1) / 2 : rounds / 2;
}

}  // namespace mcmcpp
