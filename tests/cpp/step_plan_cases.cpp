// step_plan_cases.cpp -- prints the step plan of one shape (tests/test_step_plan.py).  Built with the host compiler against
// mcmcpp_amd/csrc/step_plan.hpp alone: that it compiles without HIP is part of the test.
//   step_plan_cases key=value ...
// Shape keys: mover (stretch | de), elem_size, calc, W, D, chains, shard_begin, shard_count (0: the whole half), comm_world,
// comm_rank (its equal slice, when shard_count is 0), num_cus, graph_steps, can_capture.  Every other key is a member of Knobs
// (opt:: ones empty unless given); the knobs are set here, never through the environment.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "step_plan.hpp"

using namespace mcmcpp;

int main(int argc, char** argv)
{
    std::map<std::string, long> shape = {{"elem_size", 8}, {"calc", MCMCPP_HIP_CALC_DENSE_GAUSSIAN}, {"W", 0}, {"D", 0}, {"chains", 1}, {"shard_begin", 0},
                                         {"shard_count", 0}, {"comm_world", 0}, {"comm_rank", 0}, {"num_cus", 256}, {"graph_steps", 0}, {"can_capture", 1}};
    // the library's defaults (Knobs::from_environment with nothing set)
    Knobs k;
    k.passes = 0, k.waves_per_simd = 2, k.matrix_core_min_walkers = 0, k.matrix_core_late = 49152, k.full_step = 1, k.full_step_max_walkers = -1;
    k.task_table_mb = 16, k.chain_subchunk_mb = 32, k.graph_steps = -1, k.trickle = 1, k.no_draw_wave = 0, k.batch_draws = -1, k.pinned_direct = 1;
    k.comm_full_step = 1, k.comm_compact = 1, k.comm_compact_cap = 0, k.comm_compact_chunk = 256;
    const std::map<std::string, long*> knob = {{"passes", &k.passes}, {"waves_per_simd", &k.waves_per_simd}, {"matrix_core_min_walkers", &k.matrix_core_min_walkers},
                                               {"matrix_core_late", &k.matrix_core_late}, {"full_step", &k.full_step}, {"full_step_max_walkers", &k.full_step_max_walkers},
                                               {"task_table_mb", &k.task_table_mb}, {"knob_graph_steps", &k.graph_steps}, {"no_draw_wave", &k.no_draw_wave},
                                               {"batch_draws", &k.batch_draws}, {"comm_full_step", &k.comm_full_step}, {"comm_compact", &k.comm_compact}};
    std::string mover = "stretch";
    for (int i = 1; i < argc; ++i)
    {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string key(argv[i], (size_t)(eq - argv[i])), val(eq + 1);
        if (key == "mover")
            mover = val;
        else if (key == "matrix_core_4pass")
            k.matrix_core_4pass = std::atol(val.c_str());
        else if (shape.count(key))
            shape[key] = std::atol(val.c_str());
        else if (knob.count(key))
            *knob.at(key) = std::atol(val.c_str());
        else
        {
            std::fprintf(stderr, "unknown key %s\n", key.c_str());
            return 2;
        }
    }
    StepShape s = {};
    s.W = (int)shape["W"], s.D = (int)shape["D"], s.n = s.W / 2, s.elem_size = (int)shape["elem_size"], s.calc_id = (int)shape["calc"];
    const LaneMap m = lane_map(s.D, s.elem_size);
    s.lpw = m.lpw;
    s.chains = (int)shape["chains"], s.comm_world = (int)shape["comm_world"], s.num_cus = (int)shape["num_cus"];
    s.shard_begin = (int)shape["shard_begin"], s.shard_count = shape["shard_count"] > 0 ? (int)shape["shard_count"] : s.n;
    if (s.comm_world >= 1 && shape["shard_count"] == 0)
    {
        s.shard_count = s.n / s.comm_world;
        s.shard_begin = (int)shape["comm_rank"] * s.shard_count;
    }
    s.graph_steps = (int)shape["graph_steps"], s.can_capture = shape["can_capture"] != 0;
    // the slots of the library's launch tables (launch_build.hpp: put): the plain kernels everywhere, the matrix-core ones
    // where DenseGaussianFn::MatrixCore (calculators.hpp) says so -- 16 lanes x 2 elements in fp64, 8 lanes x 4 elements in fp32
    const bool mc = s.calc_id == MCMCPP_HIP_CALC_DENSE_GAUSSIAN && ((s.elem_size == 8 && m.epl == 2 && m.lpw == 16) || (s.elem_size == 4 && m.epl == 4 && m.lpw == 8));
    s.half_step_mc[0] = s.half_step_mc[1] = s.half_step_mc[2] = s.full_step_mc = s.de_update_mc = mc;
    s.full_step = true;
    std::printf("lpw=%d epl=%d ", m.lpw, m.epl);
    if (mover == "de")
    {
        std::printf("de_walkers_per_wave=%d\n", plan_de_update(s, k));
        return 0;
    }
    const StepPlan p = plan_stretch_step(s, k);
    static const char* const half_names[] = {"plain", "mc8", "mc16", "mc16late"};
    static const char* const full_names[] = {"none", "plain", "mc"};
    std::printf("half=%s full=%s passes=%d step_lpw=%d full_wpb=%d graph_steps=%d batch_draws=%d partial_slots=%d partial_waves=%d have_task_table=%d "
                "compact_exchange=%d half_draw_wave=%d full_draw_wave=%d grid_blocks=%u full_grid_blocks=%u\n",
                half_names[(int)p.half], full_names[(int)p.full], p.passes, p.step_lpw, p.full_wpb, p.graph_steps, p.batch_draws, p.partial_slots, p.partial_waves,
                (int)p.have_task_table, (int)p.compact_exchange, p.half_draw_wave, p.full_draw_wave, p.grid_blocks_for(s.shard_count), p.full_grid_blocks_for(s.shard_count));
    return 0;
}
