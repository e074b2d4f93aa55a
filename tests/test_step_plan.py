"""Which kernels step a handle of a given shape, and with what launch geometry: the policy of mcmcpp_amd/csrc/step_plan.hpp,
checked on the CPU.  The variant tests of the GPU suite (test_hip_parity, test_chain_params, test_chains, test_split_*) force a
kernel through an MCMCPP_HIP_* knob and compare bits with the oracle; every variant produces the same bits by design, so it is
this test that says the knob selects the variant the test's name promises.

tests/cpp/step_plan_cases.cpp is compiled with the host compiler against step_plan.hpp alone (no HIP header: that it compiles
is an assertion) and prints the plan of one shape; the knobs are constructed there from its command line, not read from the
environment.  Every field of the printed plan is compared with the values below.  num_cus is 256, the knobs are the library's
defaults, the calculator is the dense Gaussian in fp64 and the handle holds one whole ensemble unless the case says otherwise.

Fields: lpw, epl (the shape's launch-table slot); half = plain | mc8 | mc16 | mc16late (matrix-core kernels: 8 / 16 walkers per
wavefront / 16 with the next draws behind the accept); full = none | plain | mc; grid_blocks / full_grid_blocks are
StepPlan::grid_blocks_for / full_grid_blocks_for of the handle's shard (the latter means nothing where full = none)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmcpp_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
ISO, DENSE, ROSENBROCK = 0, 1, 2  # (MCMCPP_HIP_CALC_*)

CASES = [
    # ---- the shapes the design documents speak of
    ("f64_dense_16384x32_headline", dict(W=16384, D=32),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=1024 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=256 full_grid_blocks=256"),
    ("f64_dense_32768x32", dict(W=32768, D=32),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=2048 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=512 full_grid_blocks=16384"),
    ("f64_dense_65536x32", dict(W=65536, D=32),
     "lpw=16 epl=2 half=mc16 full=none passes=4 step_lpw=16 full_wpb=1 graph_steps=128 batch_draws=0 partial_slots=128 partial_waves=2048 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=512 full_grid_blocks=32768"),
    ("f64_dense_131072x32", dict(W=131072, D=32),
     "lpw=16 epl=2 half=mc16late full=none passes=4 step_lpw=16 full_wpb=1 graph_steps=128 batch_draws=0 partial_slots=128 partial_waves=4096 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=1024 full_grid_blocks=65536"),
    ("f64_iso_32768x32", dict(W=32768, D=32, calc=ISO),
     "lpw=16 epl=2 half=plain full=plain passes=2 step_lpw=16 full_wpb=16 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=4096 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=512 full_grid_blocks=1024"),
    ("f64_iso_65536x32", dict(W=65536, D=32, calc=ISO),
     "lpw=16 epl=2 half=plain full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=128 batch_draws=0 partial_slots=128 partial_waves=4096 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=1024 full_grid_blocks=32768"),
    ("f32_dense_16384x32", dict(W=16384, D=32, elem_size=4),
     "lpw=8 epl=4 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=1024 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=256 full_grid_blocks=256"),
    ("f64_dense_D16", dict(W=16384, D=16),
     "lpw=8 epl=2 half=plain full=plain passes=1 step_lpw=8 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=1024 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=256 full_grid_blocks=256"),
    ("f64_dense_D31_odd", dict(W=16384, D=31),
     "lpw=16 epl=2 half=plain full=plain passes=1 step_lpw=16 full_wpb=16 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=2048 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=512 full_grid_blocks=512"),
    ("f64_dense_D34", dict(W=16384, D=34),
     "lpw=32 epl=2 half=plain full=plain passes=2 step_lpw=32 full_wpb=8 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=4096 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=512 full_grid_blocks=1024"),
    # ---- the knobs the variant tests set, on the shapes of the tests that set them ("parity_": tests/test_hip_parity.py)
    ("parity_mc_on_4102x32", dict(W=4102, D=32, matrix_core_min_walkers=0),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=260 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=65 full_grid_blocks=65"),
    ("parity_mc_on_4102x32_half_steps", dict(W=4102, D=32, matrix_core_min_walkers=0, full_step=0),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=260 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=65 full_grid_blocks=2051"),
    ("parity_mc_on_600x18_f32", dict(W=600, D=18, elem_size=4, matrix_core_min_walkers=0),
     "lpw=8 epl=4 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=40 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=10 full_grid_blocks=10"),
    ("parity_mc_off_8202x32_f32", dict(W=8202, D=32, elem_size=4, full_step=0, matrix_core_4pass=1, matrix_core_min_walkers=-1),
     "lpw=8 epl=4 half=plain full=none passes=1 step_lpw=8 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=516 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=129 full_grid_blocks=4101"),
    ("parity_mc16_8202x32_f32", dict(W=8202, D=32, elem_size=4, full_step=0, matrix_core_4pass=1),
     "lpw=8 epl=4 half=mc16 full=none passes=4 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=260 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=65 full_grid_blocks=4101"),
    ("parity_late_draws_8266x32", dict(W=8266, D=32, full_step=0, matrix_core_min_walkers=0, matrix_core_4pass=1, matrix_core_late=0),
     "lpw=16 epl=2 half=mc16late full=none passes=4 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=260 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=65 full_grid_blocks=4133"),
    ("parity_late_draws_off_8266x32", dict(W=8266, D=32, full_step=0, matrix_core_min_walkers=0, matrix_core_4pass=1, matrix_core_late=-1),
     "lpw=16 epl=2 half=mc16 full=none passes=4 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=260 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=65 full_grid_blocks=4133"),
    ("parity_late_draws_3_chains_1062x32", dict(W=1062, D=32, chains=3, full_step=0, matrix_core_min_walkers=0, matrix_core_4pass=1, matrix_core_late=0),
     "lpw=16 epl=2 half=mc16late full=none passes=4 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=36 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=9 full_grid_blocks=531"),
    ("parity_batch_draws_0", dict(W=2054, D=32, batch_draws=0),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("parity_batch_draws_7", dict(W=2054, D=32, batch_draws=7),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=7 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("parity_batch_draws_128", dict(W=2054, D=32, batch_draws=128),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=128 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("parity_graph_steps_8", dict(W=2054, D=32, knob_graph_steps=8),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=8 batch_draws=8 partial_slots=8 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("parity_task_table_0_rosenbrock_1000x9", dict(W=1000, D=9, calc=ROSENBROCK, task_table_mb=0),
     "lpw=8 epl=2 half=plain full=plain passes=1 step_lpw=8 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=64 have_task_table=0 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=16 full_grid_blocks=16"),
    # ---- test_hip_parity.py::test_wave_mapping_and_chunking_do_not_change_results, 2050 x 32 dense fp64, each of its settings that
    #      reaches the plan.  MCMCPP_HIP_PASSES selects nothing on this shape: the matrix-core half-step kernel fixes its own
    #      passes (2) and run() steps by full steps, so those four settings run what the default runs.  The knob does act on
    #      the plain half-step kernels (passes_*_iso_4096x32_half_steps below, a shape no GPU test runs).
    ("wave_mapping_default", dict(W=2050, D=32),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_passes_1", dict(W=2050, D=32, passes=1),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_passes_4", dict(W=2050, D=32, passes=4),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_passes_16", dict(W=2050, D=32, passes=16),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_graph_steps_7", dict(W=2050, D=32, knob_graph_steps=7),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=7 batch_draws=7 partial_slots=7 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_task_table_0", dict(W=2050, D=32, task_table_mb=0),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=132 have_task_table=0 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_task_table_0_passes_8", dict(W=2050, D=32, task_table_mb=0, passes=8),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=132 have_task_table=0 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_mc_min_walkers_0", dict(W=2050, D=32, matrix_core_min_walkers=0),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=300 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_full_step_0", dict(W=2050, D=32, full_step=0),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=33 full_grid_blocks=1025"),
    ("wave_mapping_full_step_0_no_draw_wave", dict(W=2050, D=32, full_step=0, no_draw_wave=1),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=33 full_grid_blocks=1025"),
    ("wave_mapping_no_draw_wave", dict(W=2050, D=32, no_draw_wave=1),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=33 full_grid_blocks=33"),
    ("wave_mapping_mc_min_walkers_off", dict(W=2050, D=32, matrix_core_min_walkers=-1),
     "lpw=16 epl=2 half=plain full=plain passes=1 step_lpw=16 full_wpb=16 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=260 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=65 full_grid_blocks=65"),
    # ---- knobs on shapes chosen so that they act
    ("passes_1_iso_4096x32_half_steps", dict(W=4096, D=32, calc=ISO, full_step=0, passes=1),
     "lpw=16 epl=2 half=plain full=none passes=1 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=512 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=128 full_grid_blocks=2048"),
    ("passes_16_iso_4096x32_half_steps", dict(W=4096, D=32, calc=ISO, full_step=0, passes=16),
     "lpw=16 epl=2 half=plain full=none passes=16 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=32 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=8 full_grid_blocks=2048"),
    ("no_draw_wave_4096x32", dict(W=4096, D=32, no_draw_wave=1),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=256 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=64 full_grid_blocks=64"),
    ("no_draw_wave_4096x32_half_steps", dict(W=4096, D=32, full_step=0, no_draw_wave=1),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=256 have_task_table=1 compact_exchange=0 half_draw_wave=0 full_draw_wave=0 grid_blocks=64 full_grid_blocks=2048"),
    ("full_step_max_walkers_65536", dict(W=65536, D=32, calc=ISO, full_step_max_walkers=65536),
     "lpw=16 epl=2 half=plain full=plain passes=2 step_lpw=16 full_wpb=16 graph_steps=128 batch_draws=0 partial_slots=128 partial_waves=8192 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=1024 full_grid_blocks=2048"),
    ("full_step_max_walkers_1000", dict(W=4096, D=32, full_step_max_walkers=1000),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=256 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=64 full_grid_blocks=2048"),
    ("config_graph_steps_64", dict(W=16384, D=32, graph_steps=64),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=64 batch_draws=64 partial_slots=64 partial_waves=1024 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=256 full_grid_blocks=256"),
    # ---- several chains per launch (what fills the chip is shard_count x chains), split ensembles, shards, streams
    ("c4_8_chains_of_4096x32", dict(W=4096, D=32, chains=8),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=256 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=64 full_grid_blocks=2048"),
    ("chains_4_of_2054x32_mc_on", dict(W=2054, D=32, chains=4, matrix_core_min_walkers=0),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=132 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=33 full_grid_blocks=33"),
    ("comm_world_1", dict(W=16384, D=32, comm_world=1),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=1024 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=256 full_grid_blocks=256"),
    ("comm_world_2", dict(W=16384, D=32, comm_world=2, comm_rank=1),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=512 have_task_table=1 compact_exchange=1 half_draw_wave=1 full_draw_wave=1 grid_blocks=128 full_grid_blocks=128"),
    ("comm_world_2_exchange_per_half_step", dict(W=16384, D=32, comm_world=2, comm_full_step=0),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=512 have_task_table=1 compact_exchange=1 half_draw_wave=1 full_draw_wave=0 grid_blocks=128 full_grid_blocks=4096"),
    ("comm_world_2_full_step_0", dict(W=16384, D=32, comm_world=2, full_step=0),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=512 have_task_table=1 compact_exchange=1 half_draw_wave=1 full_draw_wave=0 grid_blocks=128 full_grid_blocks=4096"),
    ("comm_world_2_whole_slices", dict(W=16384, D=32, comm_world=2, comm_compact=0),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=512 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=128 full_grid_blocks=128"),
    ("comm_world_1_compact_has_nobody_to_exchange_with", dict(W=16384, D=32, comm_world=1, comm_compact=1),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=1024 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=256 full_grid_blocks=256"),
    ("comm_world_4_iso_8192x64", dict(W=8192, D=64, calc=ISO, comm_world=4, comm_compact=0),
     "lpw=32 epl=2 half=plain full=plain passes=1 step_lpw=32 full_wpb=8 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=512 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=128 full_grid_blocks=128"),
    ("shard_of_a_whole_ensemble", dict(W=16384, D=32, shard_begin=4096, shard_count=4096),
     "lpw=16 epl=2 half=mc8 full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=300 batch_draws=0 partial_slots=300 partial_waves=512 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=128 full_grid_blocks=4096"),
    ("legacy_default_stream", dict(W=16384, D=32, can_capture=0),
     "lpw=16 epl=2 half=mc8 full=mc passes=2 step_lpw=16 full_wpb=32 graph_steps=-1 batch_draws=0 partial_slots=1 partial_waves=1024 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=1 grid_blocks=256 full_grid_blocks=256"),
    ("num_cus_104", dict(W=65536, D=32, calc=ISO, num_cus=104),
     "lpw=16 epl=2 half=plain full=none passes=2 step_lpw=16 full_wpb=1 graph_steps=128 batch_draws=0 partial_slots=128 partial_waves=4096 have_task_table=1 compact_exchange=0 half_draw_wave=1 full_draw_wave=0 grid_blocks=1024 full_grid_blocks=32768"),
    # ---- differential evolution: walkers per wavefront of the matrix-core update kernel, 0 = the plain kernel
    ("de_dense_32768x32", dict(mover='de', W=32768, D=32),
     "lpw=16 epl=2 de_walkers_per_wave=8"),
    ("de_dense_65536x32", dict(mover='de', W=65536, D=32),
     "lpw=16 epl=2 de_walkers_per_wave=16"),
    ("de_dense_65534x32", dict(mover='de', W=65534, D=32),
     "lpw=16 epl=2 de_walkers_per_wave=8"),
    ("de_dense_D34", dict(mover='de', W=32768, D=34),
     "lpw=32 epl=2 de_walkers_per_wave=0"),
    ("de_dense_D31", dict(mover='de', W=32768, D=31),
     "lpw=16 epl=2 de_walkers_per_wave=0"),
    ("de_iso", dict(mover='de', W=32768, D=32, calc=ISO),
     "lpw=16 epl=2 de_walkers_per_wave=0"),
    ("de_mc_off", dict(mover='de', W=32768, D=32, matrix_core_min_walkers=-1),
     "lpw=16 epl=2 de_walkers_per_wave=0"),
    ("de_4pass_1", dict(mover='de', W=4096, D=32, matrix_core_4pass=1),
     "lpw=16 epl=2 de_walkers_per_wave=16"),
    ("de_f32_dense_32768x32", dict(mover='de', W=32768, D=32, elem_size=4),
     "lpw=8 epl=4 de_walkers_per_wave=8"),
]


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "step_plan_cases")
    # the host compiler alone, and no include path but the header's own directory: step_plan.hpp must not need HIP
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "step_plan_cases.cpp"), "-I", CSRC])
    return exe


def test_step_plan_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "step_plan.hpp")).read()
    includes = [line.split()[1] for line in text.split("\n") if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdlib>", "<optional>", '"../../include/mcmcpp_hip.h"']
    assert "hip_runtime" not in open(os.path.join(ROOT, "include", "mcmcpp_hip.h")).read()


@pytest.mark.parametrize("name,args,expected", CASES, ids=[c[0] for c in CASES])
def test_plan_of_shape(driver, name, args, expected):
    got = subprocess.run([driver] + ["%s=%s" % kv for kv in args.items()], capture_output=True, text=True, check=True).stdout.strip()
    want = dict(f.split("=") for f in expected.split())
    have = dict(f.split("=") for f in got.split())
    assert have == want, "%s: %s" % (name, {k: (have.get(k), want.get(k)) for k in sorted(set(have) | set(want)) if have.get(k) != want.get(k)})
