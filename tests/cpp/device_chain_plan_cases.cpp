// device_chain_plan_cases.cpp -- prints the schedule of a run whose stored steps stay in device memory
// (tests/test_device_chain_plan.py).  Built with the host compiler against mcmcpp_amd/csrc/run_plan.hpp alone.
//   device_chain_plan_cases WHAT key=value ...
// WHAT: device (the plan of a run_device request, chain k's offsets in the destination and the simulated host loop of
// Sampler::run_into_device_chain) or host (the plan of the same request with a host destination, printed as run_plan_cases
// prints its `chain` case).  The simulated run prints what the window said:
//   E enq now announced in_flight     a chunk of `now` steps is enqueued, with the window's state in front of it
//   O from to end                     the chunk that ended at step `end` has finished: stored steps [from, to) are announced
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "run_plan.hpp"

using namespace mcmcpp;

static void simulate(int64_t n_saved, int64_t interval, const ChainPlan& cp)
{
    DeviceWindow w(n_saved, interval, cp);
    std::printf("sim interval=%lld n_saved=%lld chunk_steps=%lld", (long long)interval, (long long)n_saved, (long long)cp.chunk_steps);
    auto process = [&]() {
        const int64_t end = w.chunk_end[DeviceWindow::event_slot(w.oldest)];
        const StoredRange r = w.process_oldest();
        std::printf(" | O %lld %lld %lld", (long long)r.from, (long long)r.to, (long long)end);
    };
    while (!w.all_enqueued())
    {
        while (w.must_process_oldest_first()) process();
        const int64_t now = w.next_length();
        std::printf(" | E %lld %lld %lld %lld", (long long)w.enq, (long long)now, (long long)w.announced, (long long)(w.next_chunk - w.oldest));
        if (DeviceWindow::event_slot(w.next_chunk) != (int)(w.next_chunk % 4)) std::abort();
        w.enqueued(now);
    }
    while (w.in_flight()) process();
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    std::map<std::string, long long> a;
    for (int i = 2; i < argc; ++i)
    {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        a[std::string(argv[i], (size_t)(eq - argv[i]))] = std::atoll(eq + 1);
    }
    auto get = [&](const char* key, long long fallback) { return a.count(key) ? a[key] : fallback; };

    // (the request as tests/cpp/run_plan_cases.cpp builds it, field by field, and the destination on top)
    ChainRequest r = {};
    r.step_bytes = (size_t)get("step_bytes", 0), r.chains = (int)get("chains", 1), r.n_saved = get("n_saved", 0), r.interval = (int32_t)get("interval", 1);
    r.chain_out = get("chain_out", 1) != 0, r.want_accepted = get("want_accepted", 1) != 0, r.full_step = get("full_step", 1) != 0;
    r.subchunk_bytes = (size_t)get("subchunk_mb", 32) << 20, r.graph_steps = (int)get("graph_steps", 300);
    r.trickle = (long)get("trickle", 1), r.pinned_direct = (long)get("pinned_direct", 1);
    r.device_dest = what == "device";
    if (what != "device" && what != "host") return 2;

    const bool ask = pinned_question_matters(r);
    const ChainPlan cp = plan_chain(r, get("pinned", 0) != 0);
    static const char* const modes[] = {"nothing", "subchunks", "trickle", "device"};
    std::printf("mode=%s ask_pinned=%d direct=%d sub_saved=%lld n_sub=%lld ring=%lld chunk_steps=%lld acc_entries=%zu half_bytes=%zu ring_bytes=%zu need_host_ring=%d slice_bytes=%lld\n",
                modes[(int)cp.mode], (int)ask, (int)cp.direct, (long long)cp.sub_saved, (long long)cp.n_sub, (long long)cp.ring, (long long)cp.chunk_steps, cp.acc_entries,
                cp.half_bytes, cp.ring_bytes, (int)cp.need_host_ring, (long long)cp.slice_bytes);
    if (what == "host") return 0;
    std::printf("offsets=");
    for (int k = 0; k < r.chains; ++k) std::printf("%s%zu", k ? "," : "", device_chain_offset(r.step_bytes, r.n_saved, k));
    std::printf("\n");
    if (cp.mode == ChainMode::Device) simulate(r.n_saved, r.interval, cp);
    return 0;
}
