// run_plan_cases.cpp -- prints the run schedule of one case (tests/test_run_plan.py).  Built with the host compiler against
// mcmcpp_amd/csrc/run_plan.hpp alone: that it compiles without HIP is part of the test.
//   run_plan_cases WHAT key=value ...
// WHAT: chain (the delivery plan of a whole-ensemble run and, for a trickle run, the simulated host loop), sweep (the
// simulated host loop over a range of intervals, run lengths, rings and both destinations), subchunk, offsets, split_chunks,
// split_stage, cap, bytes.  A simulated run plays Sampler::run_trickle with "process the oldest chunk" as the only way to make
// progress and prints what the window said:
//   E enq now copied in_flight     a chunk of `now` steps is enqueued, with the window's state in front of it
//   O from to end                  the chunk that ended at step `end` has finished: stored steps [from, to) are announced
//   T from to                      behind the final synchronisation: [from, to) is fetched from the device ring
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "run_plan.hpp"

using namespace mcmcpp;

static void simulate(int64_t n_saved, int64_t interval, const ChainPlan& cp)
{
    TrickleWindow w(n_saved, interval, cp);
    std::printf("sim interval=%lld n_saved=%lld ring=%lld chunk_steps=%lld direct=%d", (long long)interval, (long long)n_saved, (long long)cp.ring, (long long)cp.chunk_steps, (int)cp.direct);
    auto process = [&]() {
        const int64_t end = w.chunk_end[TrickleWindow::event_slot(w.oldest)];
        const StoredRange r = w.process_oldest();
        std::printf(" | O %lld %lld %lld", (long long)r.from, (long long)r.to, (long long)end);
    };
    while (!w.all_enqueued())
    {
        const int64_t now = w.next_length();
        while (w.must_process_oldest_before(now)) process();
        std::printf(" | E %lld %lld %lld %lld", (long long)w.enq, (long long)now, (long long)w.copied, (long long)(w.next_chunk - w.oldest));
        if (TrickleWindow::event_slot(w.next_chunk) != (int)(w.next_chunk % 4)) std::abort();
        w.enqueued(now);
    }
    while (w.in_flight()) process();
    const StoredRange t = w.tail();
    std::printf(" | T %lld %lld\n", (long long)t.from, (long long)t.to);
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

    if (what == "chain" || what == "sweep")
    {
        ChainRequest r = {};
        r.step_bytes = (size_t)get("step_bytes", 0), r.chains = (int)get("chains", 1), r.n_saved = get("n_saved", 0), r.interval = (int32_t)get("interval", 1);
        r.chain_out = get("chain_out", 1) != 0, r.want_accepted = get("want_accepted", 1) != 0, r.full_step = get("full_step", 1) != 0;
        r.subchunk_bytes = (size_t)get("subchunk_mb", 32) << 20, r.graph_steps = (int)get("graph_steps", 300);
        r.trickle = (long)get("trickle", 1), r.pinned_direct = (long)get("pinned_direct", 1);
        if (what == "sweep")
        {
            // rings 4 .. 64 by the budget: the ring doubles while it fits the budget, so one byte less than `ring` slots ends it there
            r.step_bytes = 16;
            for (int64_t ring = 4; ring <= 64; ring *= 2)
                for (r.interval = 1; r.interval <= 7; ++r.interval)
                    for (r.n_saved = 1; r.n_saved <= 40; ++r.n_saved)
                        for (int pinned = 0; pinned < 2; ++pinned)
                        {
                            r.subchunk_bytes = (size_t)ring * r.step_bytes - 1;
                            const ChainPlan cp = plan_chain(r, pinned != 0);
                            if (cp.ring != ring) return 3;
                            simulate(r.n_saved, r.interval, cp);
                        }
            return 0;
        }
        const bool ask = pinned_question_matters(r);
        const ChainPlan cp = plan_chain(r, get("pinned", 0) != 0);
        static const char* const modes[] = {"nothing", "subchunks", "trickle"};
        std::printf("mode=%s ask_pinned=%d direct=%d sub_saved=%lld n_sub=%lld ring=%lld chunk_steps=%lld acc_entries=%zu half_bytes=%zu ring_bytes=%zu need_host_ring=%d slice_bytes=%lld\n",
                    modes[(int)cp.mode], (int)ask, (int)cp.direct, (long long)cp.sub_saved, (long long)cp.n_sub, (long long)cp.ring, (long long)cp.chunk_steps, cp.acc_entries,
                    cp.half_bytes, cp.ring_bytes, (int)cp.need_host_ring, (long long)cp.slice_bytes);
        if (cp.mode == ChainMode::Trickle)
        {
            simulate(r.n_saved, r.interval, cp);
            std::printf("ring_slot_of_last=%lld\n", (long long)TrickleWindow(r.n_saved, r.interval, cp).ring_slot(r.n_saved - 1));
        }
        else
        {
            std::printf("subchunks=");
            for (int64_t c = 0; c < cp.n_sub; ++c) std::printf("%s%lld:%lld", c ? "," : "", (long long)cp.subchunk(c).from, (long long)cp.subchunk(c).to);
            std::printf("\n");
        }
        return 0;
    }
    if (what == "subchunk")
    {
        std::printf("%lld\n", (long long)stored_steps_per_subchunk((size_t)get("budget", 0), (size_t)get("stored_step_bytes", 1), get("n_saved", 0)));
        return 0;
    }
    if (what == "offsets")
    {
        const SubchunkCopy c = subchunk_copy((size_t)get("step_bytes", 0), get("sub_saved", 0), get("n_saved", 0), get("first", 0), get("count", 0), (int)get("k", 0));
        std::printf("dst=%zu src=%zu bytes=%zu chain_offset=%zu half_used=%zu\n", c.dst, c.src, c.bytes, subchunk_chain_offset((size_t)get("step_bytes", 0), get("sub_saved", 0), (int)get("k", 0)),
                    subchunk_half_used((size_t)get("step_bytes", 0), get("sub_saved", 0), get("now", 0), (int)get("chains", 1)));
        return 0;
    }
    if (what == "split_chunks")
    {
        // the chunks of one split run (the first one learning when the case says so, none of them rolled back)
        bool learning = get("learning", 0) != 0;
        std::printf("chunks=");
        for (int64_t s0 = 0; s0 < get("total", 0);)
        {
            const int64_t len = split_chunk_length(get("total", 0), s0, get("compact", 0) != 0, learning, (long)get("compact_chunk", 256), get("stores", 0) != 0, (int32_t)get("interval", 1),
                                                   get("stage_slots", 1));
            if (len < 1) return 3;
            std::printf("%s%lld", s0 ? "," : "", (long long)len);
            s0 += len;
            learning = false;
        }
        std::printf("\n");
        return 0;
    }
    if (what == "split_stage")
    {
        std::printf("%lld\n", (long long)split_stage_slots((size_t)get("step_bytes", 1), get("n_saved", 0)));
        return 0;
    }
    if (what == "cap")
    {
        const uint32_t cap_full = (uint32_t)get("cap_full", 0), cap_set = split_cap_set((long)get("knob", 0), cap_full);
        std::printf("cap_set=%u first=%u next=%u\n", cap_set, split_first_cap(get("compact", 1) != 0, cap_set, (uint32_t)get("learned", 0), cap_full),
                    split_next_cap((uint32_t)get("max_count", 0), cap_full));
        return 0;
    }
    if (what == "bytes")
    {
        std::printf("compact=%.0f whole=%.0f\n", split_bytes_compact(get("len", 0), get("full_step", 0) != 0, (int)get("world", 1), (size_t)get("block_bytes", 0)),
                    split_bytes_whole(get("len", 0), get("full_step", 0) != 0, (int)get("world", 1), (int)get("shard_count", 0), (int)get("dims", 0), (size_t)get("elem_size", 8)));
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
