// lane_map_cases.cpp -- prints the lane mapping of every walker width the library takes (tests/test_lane_mappings.py).
// Built with the host compiler against mcmcpp_amd/csrc/step_plan.hpp alone, as step_plan_cases.cpp is.
//   lane_map_cases          one line "elem_size D lpw epl vec_ok" for D = 1..1024 in fp64 (8) and then in fp32 (4)
#include <cstdio>

#include "step_plan.hpp"

int main()
{
    for (int elem_size : {8, 4})
        for (int D = 1; D <= 1024; ++D)
        {
            const mcmcpp::LaneMap m = mcmcpp::lane_map(D, elem_size);
            std::printf("%d %d %d %d %d\n", elem_size, D, m.lpw, m.epl, m.vec_ok);
        }
    return 0;
}
