// de_batch_plan_cases.cpp -- prints the plans of mcmcpp_amd/csrc/de_batch_plan.hpp for tests/test_de_batch_plan.py.
// Built with the host compiler alone and no include path but the header's directory: that it compiles is an assertion.
//   de_batch_plan_cases constants
//   de_batch_plan_cases plan N D BATCH SCAN_RUN      (BATCH, SCAN_RUN: a number, or - where the environment names none)
//   de_batch_plan_cases grid                         (the same line for every shape on standard input: "N D BATCH SCAN_RUN")
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "de_batch_plan.hpp"

using namespace mcmcpp;

static void print_plan(int n, int dims, const char* batch, const char* run)
{
    const bool hb = strcmp(batch, "-") != 0, hr = strcmp(run, "-") != 0;
    const DeBatchPlan p = plan_de_batch(n, dims, hb, hb ? atol(batch) : 0, hr, hr ? atol(run) : 0);
    printf("n=%d dims=%d ok=%d bound=%d per=%d by_positions=%lld by_lists=%lld by_records=%lld threshold=%llu scan_run=%d", p.n, p.dims, p.ok ? 1 : 0, p.bound, p.per,
           p.by_positions, p.by_lists, p.by_records, (unsigned long long)p.threshold, p.scan_run);
    if (p.ok)
    {
        const DeLaunchPlan l = plan_de_launch(n, dims, p.batch_max, p.resolve_capacity);
        printf(" batch_max=%d updates_max=%lld positions_max=%lld expected=%lld bad_capacity=%d resolve_capacity=%d scan_lanes=%lld scan_blocks=%d small_len=%zu "
               "scan_lo_len=%zu lo_len=%zu hi_len=%zu scan_hi_len=%zu updates=%d positions=%d scan_positions=%d seg_len=%d record_blocks=%d resolve_lds=%zu records_lds=%zu "
               "lds_both=%zu lds_resolve=%zu lds_records=%zu lds_scan=%zu",
               p.batch_max, p.updates_max, p.positions_max, p.expected, p.bad_capacity, p.resolve_capacity, p.scan_lanes, p.scan_blocks, p.small_len, p.scan_lo_len, p.lo_len,
               p.hi_len, p.scan_hi_len, l.updates, l.positions, l.scan_positions, l.seg_len, l.record_blocks, l.resolve_lds, l.records_lds, de_launch_lds(l, true, true),
               de_launch_lds(l, true, false), de_launch_lds(l, false, true), de_launch_lds(l, false, false));
    }
    printf(" text=%s\n", de_batch_bound_text(p.bound));
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "constants"))
    {
        printf("batch_max=%d shift_max=%d window=%d overrun=%d segments=%d count_stride=%d max_bad=%d max_events=%d scan_run=%d threads=%d record_updates=%lld event_bytes=%zu\n",
               kDeBatchMax, kDeShiftMax, kDeWindow, kDeOverrun, kDeSegments, kDeCountStride, kDeMaxBad, kDeMaxEvents, kDeScanRun, kDePlanThreads, kDeRecordUpdates,
               kDeEventBytes);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "plan"))
    {
        print_plan(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5]);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "grid"))
    {
        int n, dims;
        char batch[32], run[32];
        while (scanf("%d %d %31s %31s", &n, &dims, batch, run) == 4) print_plan(n, dims, batch, run);
        return 0;
    }
    fprintf(stderr, "usage: de_batch_plan_cases constants | plan N D BATCH SCAN_RUN | grid\n");
    return 2;
}
