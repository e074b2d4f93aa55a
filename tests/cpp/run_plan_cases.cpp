// run_plan_cases.cpp -- prints the run schedule of one case (tests/test_run_plan.py).  Built with the host compiler against
// mcmcpp_amd/csrc/run_plan.hpp alone: that it compiles without HIP is part of the test.
//   run_plan_cases WHAT key=value ...
// WHAT: chain (the delivery plan of a whole-ensemble run and, for a trickle run, the simulated host loop), sweep (the
// simulated host loop over a range of intervals, run lengths, rings and both destinations), subchunk, offsets, split_chunks,
// split_stage, cap, bytes, split_sim, split_sweep.  A simulated run plays Sampler::run_trickle with "process the oldest chunk"
// as the only way to make progress and prints what the window said:
//   E enq now copied in_flight     a chunk of `now` steps is enqueued, with the window's state in front of it
//   O from to end                  the chunk that ended at step `end` has finished: stored steps [from, to) are announced
//   T from to                      behind the final synchronisation: [from, to) is fetched from the device ring
// split_sim plays Sampler::run_split through SplitWindow.  Its only inputs besides the request are the chunk tries that
// overflow (overflow=3,7: the tries of the run counted from 0) and what each held chunk reports (max_counts=900,40: the last
// one repeats).  It prints
//   C s0 len cap                   a try of the chunk [s0, s0 + len) with blocks of cap slots
//   X slot s                       step s's exchange is timed by the events of sample slot `slot`
//   S s slot                       step s is stored into staging slot `slot`
//   R s0                           the try overflowed: the stream goes back in front of step s0
//   K max_count cap_next           the try held
//   H from to                      stored steps [from, to) leave the staging buffer
// and the figures of the end of the run.  split_sweep plays the sweep of tests/test_run_plan.py and writes one row of twelve
// 32-bit integers per schedule, try, hand-out and end of run to stdout (the columns: see emit below).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include <vector>

#include "run_plan.hpp"

using namespace mcmcpp;

// the block of the moved-rows exchange as exchange_plan.hpp lays it out (this driver includes run_plan.hpp alone):
// [header 16][idx: cap x u32][logp: cap x T][rows: cap x D x T], every piece rounded up to 16 bytes
static size_t a16(size_t b) { return (b + 15) & ~(size_t)15; }
static size_t block_bytes(uint32_t cap, int dims, size_t elem) { return 16 + a16((size_t)cap * 4) + a16((size_t)cap * elem) + a16((size_t)cap * (size_t)dims * elem); }

static void emit(int32_t kind, int64_t sid, std::initializer_list<int64_t> v)
{
    int32_t row[12] = {kind, (int32_t)sid};
    int k = 2;
    for (int64_t x : v) row[k++] = (int32_t)x;
    std::fwrite(row, sizeof row, 1, stdout);
}

// One schedule of the sweep.  pattern: the first try of every chunk (1), of every 2nd (2) or of every 3rd (3) overflows, or none
// (0); a held chunk reports a count that depends on where it starts, not on who stores.  Rows:
//   0 sid total interval compact compact_chunk stage_slots any_rank_stores stores knob pattern cap_full
//   1 sid s0 len cap overflowed samples_before samples_after staged_at_end staged_left max_count cap_next
//   2 sid from to
//   3 sid rollbacks cap_slots cap_to_keep xbytes samples full_step
static void sweep_one(int64_t sid, SplitRequest q, int pattern)
{
    emit(0, sid, {q.total, q.interval, q.compact, q.comm_compact_chunk, q.stage_slots, q.any_rank_stores, q.stores, q.comm_compact_cap, pattern, q.cap_full});
    SplitWindow w(q);
    for (int64_t chunk = 0; !w.done(); ++chunk)
        for (int attempt = 0;; ++attempt)
        {
            if (w.end() <= w.first() || w.end() > q.total) std::abort();
            const int before = w.samples;
            for (int64_t s = w.first(); s < w.end(); ++s)
            {
                (void)w.take_sample(s);
                if (w.stores_step(s) && w.take_stage_slot() != w.staged - w.handed - 1) std::abort();
            }
            const int64_t s0 = w.first(), len = w.end() - w.first(), cap = w.cap, staged = w.staged - w.handed, after = w.samples;
            const bool overflow = attempt == 0 && q.compact && pattern > 0 && chunk % pattern == pattern - 1;
            if (overflow)
            {
                if (w.chunk_overflowed() != s0) std::abort();
                if (w.samples != before) std::abort();  // (forgotten; the row says what the try had sampled)
                emit(1, sid, {s0, len, cap, 1, before, after, staged, w.staged - w.handed, 0, w.cap});
                continue;
            }
            const uint32_t max_count = (uint32_t)((q.total * 31 + q.interval * 17 + s0 * 13 + 5) % (cap + 1));
            w.chunk_held(max_count);
            const StoredRange out = w.hand_out();
            emit(1, sid, {s0, len, cap, 0, before, w.samples, staged, w.staged - w.handed, max_count, w.cap});
            if (out.to > out.from) emit(2, sid, {out.from, out.to});
            break;
        }
    emit(3, sid, {w.rollbacks, w.cap_slots(), w.cap_learned, (int64_t)w.xbytes, w.samples, q.full_step});
}

static std::vector<long long> list_of(const char* text)
{
    std::vector<long long> v;
    for (const char* p = text; p && *p;)
    {
        v.push_back(std::atoll(p));
        p = std::strchr(p, ',');
        if (p) ++p;
    }
    return v;
}

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
    std::map<std::string, std::string> text;  // (the same arguments as written: split_sim's lists)
    for (int i = 2; i < argc; ++i)
    {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        a[std::string(argv[i], (size_t)(eq - argv[i]))] = std::atoll(eq + 1);
        text[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
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
    // a split run's request from the arguments (a run that stores: any_rank_stores unless the case says otherwise)
    auto split_request = [&]() {
        SplitRequest q = {};
        q.total = get("total", 0), q.interval = (int32_t)get("interval", 1), q.stores = get("stores", 0) != 0, q.any_rank_stores = get("any_rank_stores", q.stores) != 0;
        q.stage_slots = get("stage_slots", 1), q.compact = get("compact", 0) != 0, q.cap_full = (uint32_t)get("cap_full", 4096);
        q.comm_compact_cap = (long)get("knob", 0), q.comm_compact_chunk = (long)get("compact_chunk", 256);
        // (the earlier cases say `learning`: a run that knows no bound -- or, without it, one that has learned some)
        q.cap_learned = (uint32_t)get("learned", a.count("learning") && !get("learning", 0) ? q.cap_full : 0);
        q.full_step = get("full_step", 1) != 0, q.comm_world = (int)get("world", 4), q.shard_count = (int)get("shard_count", 100), q.dims = (int)get("dims", 5);
        q.elem_size = (size_t)get("elem_size", 8), q.block_bytes = &block_bytes;
        return q;
    };
    if (what == "split_chunks")
    {
        // the chunks of one split run (the first one learning when the case says so, none of them rolled back)
        SplitRequest q = split_request();
        if (!a.count("learning")) q.cap_learned = q.cap_full;
        std::printf("chunks=");
        for (SplitWindow w(q); !w.done(); w.chunk_held(0))
        {
            if (w.end() <= w.first()) return 3;
            std::printf("%s%lld", w.first() ? "," : "", (long long)(w.end() - w.first()));
        }
        std::printf("\n");
        return 0;
    }
    if (what == "split_sim")
    {
        const SplitRequest q = split_request();
        const std::vector<long long> overflow = list_of(text.count("overflow") ? text["overflow"].c_str() : ""), counts = list_of(text.count("max_counts") ? text["max_counts"].c_str() : "0");
        SplitWindow w(q);
        size_t held = 0;
        for (long long attempt = 0; !w.done(); ++attempt)
        {
            std::printf("C %lld %lld %u | ", (long long)w.first(), (long long)(w.end() - w.first()), w.cap);
            for (int64_t s = w.first(); s < w.end(); ++s)
            {
                const int slot = w.take_sample(s);
                if (slot >= 0) std::printf("X %d %lld | ", slot, (long long)s);
                if (w.stores_step(s)) std::printf("S %lld %lld | ", (long long)s, (long long)w.take_stage_slot());
            }
            bool fails = false;
            for (long long t : overflow) fails = fails || t == attempt;
            if (fails)
            {
                std::printf("R %lld | ", (long long)w.chunk_overflowed());
                continue;
            }
            const uint32_t max_count = (uint32_t)counts[held < counts.size() ? held : counts.size() - 1];
            ++held;
            w.chunk_held(max_count);
            std::printf("K %u %u | ", max_count, w.cap);
            const StoredRange out = w.hand_out();
            if (out.to > out.from) std::printf("H %lld %lld | ", (long long)out.from, (long long)out.to);
        }
        std::printf("end rollbacks=%lld cap_slots=%lld cap_to_keep=%u samples=%d bytes_per_step=%.17g\n", (long long)w.rollbacks, (long long)w.cap_slots(), w.cap_learned, w.samples, w.bytes_per_step());
        return 0;
    }
    if (what == "split_sweep")
    {
        // total 1..60 x interval 1..7 (total / interval stored steps) x how the exchanges go x who stores x the staging buffer
        int64_t sid = 0;
        for (int64_t total = 1; total <= 60; ++total)
            for (int32_t interval = 1; interval <= 7; ++interval)
                for (int scheme = 0; scheme < 9; ++scheme)  // 0: whole slices; 1..8: moved rows, the bound set (odd) or learned, overflow pattern (scheme - 1) / 2
                    for (long chunk : {3L, 4L, 7L, 256L})
                        for (int slots_case = 0; slots_case < 4; ++slots_case)
                            for (int stores_case = 0; stores_case < 3; ++stores_case)  // nobody stores; this rank stores; another rank does
                            {
                                if (scheme == 0 && chunk != 3) continue;            // (whole slices: no chunk knob)
                                if (stores_case == 0 && slots_case != 0) continue;  // (nobody stores: no staging buffer)
                                const int64_t n_saved = total / interval > 0 ? total / interval : 1;
                                SplitRequest q = {};
                                q.total = total, q.interval = interval, q.any_rank_stores = stores_case != 0, q.stores = stores_case == 1;
                                q.stage_slots = slots_case == 0 ? 1 : slots_case == 1 ? 2 : slots_case == 2 ? 4 : n_saved;
                                if (q.stage_slots > n_saved) q.stage_slots = n_saved;  // (split_stage_slots never exceeds the run's)
                                q.compact = scheme > 0, q.cap_full = 200, q.comm_compact_cap = scheme % 2 ? 96 : 0, q.comm_compact_chunk = chunk, q.cap_learned = 0;
                                q.full_step = total % 2 != 0, q.comm_world = 4, q.shard_count = q.full_step ? 100 : 200, q.dims = 5, q.elem_size = 8, q.block_bytes = &block_bytes;
                                sweep_one(sid++, q, scheme > 0 ? (scheme - 1) / 2 : 0);
                            }
        return 0;
    }
    if (what == "split_stage")
    {
        std::printf("%lld\n", (long long)split_stage_slots((size_t)get("step_bytes", 1), get("n_saved", 0)));
        return 0;
    }
    if (what == "cap")
    {
        SplitRequest q = split_request();
        q.total = 1, q.compact = get("compact", 1) != 0, q.cap_full = (uint32_t)get("cap_full", 0), q.cap_learned = (uint32_t)get("learned", 0);
        const SplitWindow w(q);
        std::printf("cap_set=%u first=%u next=%u\n", w.cap_set, w.cap, split_next_cap((uint32_t)get("max_count", 0), q.cap_full));
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
