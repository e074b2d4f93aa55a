// evidence_plan_cases.cpp -- prints what mcmcpp_amd/csrc/evidence_plan.hpp plans for the evidence ratios
// (tests/test_evidence_plan.py).  Built with the host compiler against evidence_plan.hpp (and the rhat_plan.hpp and
// step_chunks.hpp it includes) alone: that it compiles without HIP is part of the test.
//   evidence_plan_cases pairs K=..                     "d p index draws_rung other_rung" per line, in output order
//   evidence_plan_cases rungs K=..                     "k evals=a,b,.. uses=d:p,.." per rung
//   evidence_plan_cases chunks n=.. step_bytes=.. on_device=.. slice=..   (the knob from the environment)
//                                                      "per" and then "k0 now" per chunk, as for_each_step_chunk walks them
//   evidence_plan_cases weights N=..                   slen, slices, tiles per slice, blocks, diff blocks, then "t first count"
//   evidence_plan_cases limits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "evidence_plan.hpp"

using namespace mcmcpp;

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string what = argv[1];
    std::map<std::string, std::string> a;
    for (int i = 2; i < argc; ++i)
    {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        a[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    auto get = [&](const char* key, long long fallback) { return a.count(key) ? std::atoll(a[key].c_str()) : fallback; };

    if (what == "pairs")
    {
        const int K = (int)get("K", 2);
        for (int d = 0; d < 2; ++d)
            for (int p = 0; p < evidence_pairs(K); ++p)
                std::printf("%d %d %d %d %d\n", d, p, evidence_index(K, d, p), evidence_draws_rung(d, p), evidence_other_rung(d, p));
        return 0;
    }
    if (what == "rungs")
    {
        const int K = (int)get("K", 2);
        for (int k = 0; k < K; ++k)
        {
            const EvidenceRung r = evidence_rung(K, k);
            std::printf("%d evals=", k);
            for (int j = 0; j < r.n_evals; ++j) std::printf("%s%d", j ? "," : "", r.evals[j]);
            std::printf(" uses=");
            for (int j = 0; j < r.n_uses; ++j) std::printf("%s%d:%d", j ? "," : "", r.use_d[j], r.use_p[j]);
            std::printf("\n");
        }
        return 0;
    }
    if (what == "chunks")
    {
        const long long per = evidence_steps_per_chunk(chunk_bytes_from_env("MCMCPP_HIP_EVIDENCE_CHUNK_MB", 1024), (size_t)get("step_bytes", 8), get("on_device", 0) != 0,
                                                       get("slice", 1));
        std::printf("%lld\n", per);
        return for_each_step_chunk(get("n", 1), per, [](long long k0, long long now) {
            std::printf("%lld %lld\n", k0, now);
            return 0;
        });
    }
    if (what == "weights")
    {
        const long long N = get("N", 1);
        const EvidenceWeightsPlan p = evidence_weights_plan(N);
        std::printf("slen=%lld slices=%d tiles=%d blocks=%u diff_blocks=%lld fits=%d\n", p.slen, p.slices, p.tiles_per_slice, p.blocks, evidence_diff_blocks(N),
                    (int)evidence_grid_fits(N));
        for (int t = 0; t < p.slices; ++t)
        {
            long long first, count;
            evidence_slice_span(N, p.slen, t, &first, &count);
            std::printf("%d %lld %lld\n", t, first, count);
        }
        return 0;
    }
    if (what == "limits")
    {
        std::printf("threads=%d tile=%d grid_x=%lld\n", kEvidenceThreads, kEvidenceTile, kRhatGridXMax);
        return 0;
    }
    std::fprintf(stderr, "unknown case %s\n", what.c_str());
    return 2;
}
