// run_refusal.hpp -- which run() or run_device() call a handle refuses before it touches the device, and with which code:
// one pure function over plain facts, for the three movers and both entry points.  The order of the checks is the table;
// tests/test_run_entry.py walks every combination of the facts on the CPU.  No HIP header: this file compiles with the
// host compiler alone.  SamplerHost::run_entry (sampler_host.hpp) asks here, and so does the rank-local preparation of a
// split run.
#pragma once

#include "../../include/mcmcpp_hip.h"

namespace mcmcpp
{
enum class Mover { Stretch, DiffEvo, Batch };

struct RunFacts
{
    Mover mover;
    bool to_device;      // run_device
    bool have_state;
    bool callback_set;   // Batch: set_batch_calculator has been called
    bool communicator;   // Stretch: one ensemble split over the ranks of a communicator
    bool sharded;        // Stretch: the handle updates a slice of the ensemble
    bool half_done;      // Stretch: half_step_async has left an ensemble step half done
    bool bad_arguments;  // n_saved < 0 || interval < 1
};

enum class RunRefusal { None, DeviceWithCommunicator, DeviceSharded, NoCallback, NoState, BadArguments, Sharded, HalfDone };

// The first check that fails, in the order the movers have always made them.  The fused sampler's run_device turns away
// the handles it is not for before anything else; the batch mover misses its callback before it misses a state; a handle
// with a communicator is sharded by construction and run() is how it is driven.
inline RunRefusal run_refusal(const RunFacts& f)
{
    const bool stretch = f.mover == Mover::Stretch;
    if (stretch && f.to_device && f.communicator) return RunRefusal::DeviceWithCommunicator;
    if (stretch && f.to_device && f.sharded) return RunRefusal::DeviceSharded;
    if (f.mover == Mover::Batch && !f.callback_set) return RunRefusal::NoCallback;
    if (!f.have_state) return RunRefusal::NoState;
    if (f.bad_arguments) return RunRefusal::BadArguments;
    if (stretch && f.sharded && !f.communicator) return RunRefusal::Sharded;
    if (stretch && f.half_done) return RunRefusal::HalfDone;
    return RunRefusal::None;
}

inline int run_refusal_code(RunRefusal r)
{
    switch (r)
    {
    case RunRefusal::None: return MCMCPP_HIP_OK;
    case RunRefusal::BadArguments: return MCMCPP_HIP_E_ARG;
    case RunRefusal::DeviceWithCommunicator:
    case RunRefusal::DeviceSharded:
    case RunRefusal::Sharded: return MCMCPP_HIP_E_UNSUPPORTED;
    default: return MCMCPP_HIP_E_STATE;
    }
}

// the message behind the entry point's name ("run: ", "run_device: ")
inline const char* run_refusal_text(RunRefusal r)
{
    switch (r)
    {
    case RunRefusal::DeviceWithCommunicator: return "not for a handle with a communicator (run delivers a split ensemble's stored steps)";
    case RunRefusal::DeviceSharded: return "a sharded handle stores into the chain given to bind_device_chain";
    case RunRefusal::NoCallback: return "no batch calculator (mcmcpp_hip_set_batch_calculator)";
    case RunRefusal::NoState: return "set_state has not been called (or a run failed half way)";
    case RunRefusal::BadArguments: return "n_saved >= 0 and interval >= 1 required";
    case RunRefusal::Sharded: return "a sharded handle is driven with half_step_async";
    case RunRefusal::HalfDone: return "an ensemble step is half done (half_step_async)";
    default: return "";
    }
}

// A handle with a communicator runs collectively: a rank's verdict, its zero-step runs included, goes through the
// all-reduce of run_split before any rank returns, so the entry must not return in front of it
inline bool run_is_collective(const RunFacts& f) { return f.mover == Mover::Stretch && f.communicator && !f.to_device; }
}  // namespace mcmcpp
