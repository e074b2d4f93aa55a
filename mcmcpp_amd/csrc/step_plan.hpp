// step_plan.hpp -- which kernels step a handle of a given shape, and with what launch geometry: the library's tuning knobs
// and the policy that reads them, as pure functions of plain numbers.  No HIP header: this file compiles with the host
// compiler alone, and tests/test_step_plan.py checks the policy there, shape by shape.  The samplers (mcmcpp_hip.hip,
// diffevo.hip) turn a plan into launch-table entries and buffer sizes; nothing else in the library holds a threshold.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <optional>

#include "../../include/mcmcpp_hip.h"

namespace mcmcpp
{
constexpr int kWavesPerBlock = 4;  // updating wavefronts per workgroup
constexpr size_t kJumpEntryBytes = 32;  // sizeof(Affine128): one entry of a jump table

inline int pow2_at_least(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int ilog2(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// The lane mapping of the kernels: lpw lanes x epl elements cover the walker's D-vector padded to a power of two (16 bytes
// per lane until a walker fills a wavefront).  The shape's launch-table slot is [ilog2(lpw)][ilog2(epl / base)], base =
// 16 bytes / elem_size.
struct LaneMap { int lpw, epl, vec_ok; };
inline LaneMap lane_map(int D, int elem_size)
{
    const int base = 16 / elem_size, n2 = pow2_at_least(D > base ? D : base), lpw = n2 / base < 64 ? n2 / base : 64;
    return {lpw, n2 / lpw, (D % base == 0) ? 1 : 0};
}

inline std::optional<long> env_long(const char* name)
{
    const char* v = std::getenv(name);
    if (v && *v) return std::strtol(v, nullptr, 10);
    return std::nullopt;
}
inline long env_long(const char* name, long fallback) { return env_long(name).value_or(fallback); }

// The library's tuning knobs (environment variables, DESIGN.md section 9 lists them).  Read ONCE, when a handle is
// created; nothing on the launch path touches the environment.  Negative "unset" values mean "library default"; a knob
// whose default differs between the movers is left empty when unset (-1 is one of its values).
struct Knobs
{
    long passes;                  // MCMCPP_HIP_PASSES                   walkers-per-wavefront rounds of the half-step kernels (0: chosen from the size)
    long waves_per_simd;          // MCMCPP_HIP_WAVES_PER_SIMD           wavefronts per SIMD to reach before a wavefront takes more walkers (2)
    long matrix_core_min_walkers; // MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS  smallest shard stepped by the matrix-core kernels (0; -1: never)
    std::optional<long> matrix_core_4pass;  // MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS from this many updates per launch on: 16 walkers per wavefront
                                            //                                      (stretch 18432, differential evolution 32768)
    long matrix_core_late;        // MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS    from this many updates per launch on: the 16-walker wavefronts make their next draws behind the accept, four to a SIMD (49152; -1: never)
    long full_step;               // MCMCPP_HIP_FULL_STEP                1: one launch per ensemble step for small ensembles (1)
    long full_step_max_walkers;   // MCMCPP_HIP_FULL_STEP_MAX_WALKERS    largest ensemble stepped that way (-1: 32768; 32767 where the matrix-core
                                  //                                     half-step kernel is the alternative)
    long task_table_mb;           // MCMCPP_HIP_TASK_TABLE_MB            size limit of the one-entry-per-draw jump table (16)
    long chain_subchunk_mb;       // MCMCPP_HIP_CHAIN_SUBCHUNK_MB        device chain staging per sub-chunk / ring budget (32)
    long graph_steps;             // MCMCPP_HIP_GRAPH_STEPS              ensemble steps per hipGraph replay (-1 here: 300 up to 32768 walkers, else 128)
    long trickle;                 // MCMCPP_HIP_TRICKLE                  1: stored steps forwarded to pinned memory by the launches (1)
    long no_draw_wave;            // MCMCPP_HIP_NO_DRAW_WAVE             1: no extra draw wavefronts (0)
    long batch_draws;             // MCMCPP_HIP_BATCH_DRAWS              ensemble steps whose draw records one launch makes ahead of the matrix-core full-step launches; 0: the launches make them themselves; -1: as many as a graph replays (-1)
    long pinned_direct;           // MCMCPP_HIP_PINNED_DIRECT            1: stored steps forwarded straight into a pinned chain_out (1)
    long comm_full_step;          // MCMCPP_HIP_COMM_FULL_STEP           split ensembles: 1 = one exchange per ensemble step (1), 0 = one per half-step
    long comm_compact;            // MCMCPP_HIP_COMM_COMPACT             split ensembles of more than one rank: 1 = exchange only the rows that moved (1), 0 = all-gather the slices
    long comm_compact_cap;        // MCMCPP_HIP_COMM_COMPACT_CAP         slots of an exchange block (0: learned from the run; a bound that is too small costs
                                  //                                     a repeated chunk, never a wrong chain)
    long comm_compact_chunk;      // MCMCPP_HIP_COMM_COMPACT_CHUNK       ensemble steps between two looks at the overflow flag (256)
    std::optional<long> de_scan_run;  // MCMCPP_HIP_DE_SCAN_RUN          differential evolution: stream positions one scanning lane steps through (kDeScanRun)
    std::optional<long> de_batch;     // MCMCPP_HIP_DE_BATCH             differential evolution: half-steps planned together (kDeBatchMax)
    static Knobs from_environment()
    {
        Knobs k;
        k.passes = env_long("MCMCPP_HIP_PASSES", 0);
        k.waves_per_simd = env_long("MCMCPP_HIP_WAVES_PER_SIMD", 2);
        k.matrix_core_min_walkers = env_long("MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS", 0);
        k.matrix_core_4pass = env_long("MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS");
        k.matrix_core_late = env_long("MCMCPP_HIP_MATRIX_CORE_LATE_DRAWS", 49152);
        k.full_step = env_long("MCMCPP_HIP_FULL_STEP", 1);
        k.full_step_max_walkers = env_long("MCMCPP_HIP_FULL_STEP_MAX_WALKERS", -1);
        k.task_table_mb = env_long("MCMCPP_HIP_TASK_TABLE_MB", 16);
        k.chain_subchunk_mb = env_long("MCMCPP_HIP_CHAIN_SUBCHUNK_MB", 32);
        k.graph_steps = env_long("MCMCPP_HIP_GRAPH_STEPS", -1);
        k.trickle = env_long("MCMCPP_HIP_TRICKLE", 1);
        k.no_draw_wave = env_long("MCMCPP_HIP_NO_DRAW_WAVE", 0);
        k.batch_draws = env_long("MCMCPP_HIP_BATCH_DRAWS", -1);
        k.pinned_direct = env_long("MCMCPP_HIP_PINNED_DIRECT", 1);
        k.comm_full_step = env_long("MCMCPP_HIP_COMM_FULL_STEP", 1);
        k.comm_compact = env_long("MCMCPP_HIP_COMM_COMPACT", 1);
        k.comm_compact_cap = env_long("MCMCPP_HIP_COMM_COMPACT_CAP", 0);
        k.comm_compact_chunk = env_long("MCMCPP_HIP_COMM_COMPACT_CHUNK", 256);
        if (k.comm_compact_chunk < 1) k.comm_compact_chunk = 1;
        k.de_scan_run = env_long("MCMCPP_HIP_DE_SCAN_RUN");
        k.de_batch = env_long("MCMCPP_HIP_DE_BATCH");
        return k;
    }
};

// What the choice of step kernels may depend on, and nothing else.  The launch-table slots are those of the shape's
// [log2(lpw)][log2(epl / base)] (LaunchTable): a sampler states which of them its calculator's table holds.
struct StepShape
{
    int W, D, n;                   // walkers, dimensions, walkers of one colour (W / 2)
    int lpw;                       // lanes per walker (lane_map)
    int elem_size;                 // sizeof(T)
    int calc_id;
    int shard_begin, shard_count;  // the walkers of each colour this handle updates
    int chains;                    // K: independent ensembles stepped by one launch
    int comm_world;                // < 1: no communicator
    int num_cus;
    int graph_steps;               // as configured (0: the library's default)
    bool can_capture;              // the handle's own stream, or a caller's that is not the NULL / legacy default stream
    bool half_step_mc[3], full_step, full_step_mc, de_update_mc;  // launch-table slots that exist (de_update_mc: [0] and [1])
};

// The matrix-core half-step kernels: 8 walkers per wavefront (half_step_mc[0]), 16 ([1]), 16 with the next draws behind the
// accept ([2]) -- in the order of LaunchTable::half_step_mc, which Sampler::init indexes by the enum.  FullStepKernel::None:
// run() steps with one launch per half-step.
enum class HalfStepKernel { Plain, MatrixCore8, MatrixCore16, MatrixCore16Late };
enum class FullStepKernel { None, Plain, MatrixCore };

struct StepPlan
{
    HalfStepKernel half = HalfStepKernel::Plain;
    FullStepKernel full = FullStepKernel::None;
    int passes = 1;              // walkers-per-wavefront rounds of the half-step kernel
    int step_lpw = 1;            // lanes per walker of the step kernels in use
    int full_wpb = 1;            // walkers of each colour per full-step workgroup
    int graph_steps = 32;        // ensemble steps per hipGraph replay; < 1: plain launches
    int batch_draws = 0;         // ensemble steps whose draw records one launch makes ahead; 0: the step launches make their own next records
    int partial_slots = 1, partial_waves = 0;  // the per-wavefront accepted counts: [partial_slots][2][partial_waves]
    bool have_task_table = false;   // the one-entry-per-draw jump table
    bool compact_exchange = false;  // split ensembles: exchange only the rows that moved (exchange_kernels.hpp)
    int half_draw_wave = 0, full_draw_wave = 0;  // HalfStepArgs::draw_wave of a half-step / a full-step launch

    bool matrix_core_half() const { return half != HalfStepKernel::Plain; }
    unsigned grid_blocks_for(int count) const
    {
        const long per_wave = (long)(64 / step_lpw) * passes;
        const long waves = (count + per_wave - 1) / per_wave;
        return (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
    }
    unsigned full_grid_blocks_for(int count) const { return (unsigned)((count + full_wpb - 1) / full_wpb); }
};

// May this shape use the matrix-core kernels at all (the dense Gaussian's product as MFMA tiles: even D; which D and
// element types have such a kernel is the launch table's matter)?  `updates`: what MCMCPP_HIP_MATRIX_CORE_MIN_WALKERS
// is compared against.
inline bool matrix_core_shape(const StepShape& s, const Knobs& knobs, long updates)
{
    const long mc_min = knobs.matrix_core_min_walkers;
    return s.D % 2 == 0 && mc_min >= 0 && updates >= mc_min && s.calc_id == MCMCPP_HIP_CALC_DENSE_GAUSSIAN;  // (they read the padded matrix the sampler prepares)
}
// (the stretch move's matrix-core kernels address a chain's arrays with 32-bit byte offsets)
inline bool offsets_fit_32_bits(const StepShape& s) { return (size_t)s.W * (size_t)s.D * (size_t)s.elem_size < (1ull << 32); }

// Ensemble steps per hipGraph replay.  A boundary between two replays costs a few microseconds of the launch
// sequence: ensembles small enough for one launch per step (5.6 us each) take 300 per replay -- with the bench's
// slicing interval of 100 that is three stored steps per replay, as many as the forwarding ring allows; measured 1.5 %
// over 128 -- larger ones, whose launches are long and whose per-step counters grow with the walker count, 128.
inline long default_graph_steps(const StepShape& s, const Knobs& knobs) { return knobs.graph_steps >= 0 ? knobs.graph_steps : (s.W <= 32768 ? 300 : 128); }

// The stretch move (Sampler, mcmcpp_hip.hip).
inline StepPlan plan_stretch_step(const StepShape& s, const Knobs& knobs)
{
    StepPlan p;
    // Walkers per wavefront: fill the chip first (about two wavefronts per SIMD), then up to 8 per wavefront (still
    // served by the draw wavefront) and 16 for the largest ensembles.  Measured, 32 dims fp64 (tools/sweep_passes.txt):
    // 65 536 walkers 5.2 / 5.8 / 4.4e9 walker-steps/s with 4 / 8 / 16 walkers per wavefront, 262 144: 7.4e9 with 8,
    // 1 M: 6.7 / 8.0 / 7.8 / 7.4e9 with 8 / 16 / 32 / 64.
    // Independent ensembles stepped by the same launches (BASELINE config 4 on one GPU): chain k is seeded with
    // seed + k on the same stream, so all chains share the jump tables; see ChainGeometry for the layout.  What a
    // launch has to fill the chip with is the walkers of all chains together.
    const long launch_walkers = (long)s.shard_count * s.chains;  // walkers of one colour a launch updates
    const int wpp = 64 / s.lpw;
    if (knobs.passes > 0)
        p.passes = (int)knobs.passes;
    else
    {
        const long target_waves = (long)s.num_cus * 4 * knobs.waves_per_simd;
        const int per_wave_cap = launch_walkers > 196608 ? 16 : 8;
        while (p.passes * 2 <= s.lpw && wpp * p.passes * 2 <= per_wave_cap && launch_walkers / ((long)wpp * p.passes * 2) >= target_waves) p.passes *= 2;
    }
    if (p.passes < 1) p.passes = 1;
    if (p.passes > s.lpw) p.passes = s.lpw;
    p.step_lpw = s.lpw;
    // Matrix-core variants of the half-step kernel (dense calculators, fp64, even D in 18..32): the wavefront's
    // walkers are rows of one MFMA tile -- 8 walkers (2 passes) until the chip is full, 16 (4 passes) beyond.
    const bool mc_stretch = matrix_core_shape(s, knobs, s.shard_count) && offsets_fit_32_bits(s);
    if (s.half_step_mc[0] && mc_stretch)
    {
        // (measured after the round-3 rework, us per launch with 8 / 16 walkers per wavefront: 16 384 updates 5.04 / 5.23,
        //  20 480: 7.37 / 6.57, 24 576: 7.54 / 6.63, 28 672: 9.97 / 6.72, 32 768: 10.02 / 6.78 -- profiles/r03_mc_p2_p4.txt)
        p.half = launch_walkers >= knobs.matrix_core_4pass.value_or(18432) ? HalfStepKernel::MatrixCore16 : HalfStepKernel::MatrixCore8;
        // (about as many updates as one round of wavefront slots holds at three wavefronts per SIMD, or more: four per SIMD,
        //  draws behind the accept -- profiles/r03_mc_threshold.txt)
        if (p.half == HalfStepKernel::MatrixCore16 && knobs.matrix_core_late >= 0 && launch_walkers >= knobs.matrix_core_late && s.half_step_mc[2])
            p.half = HalfStepKernel::MatrixCore16Late;
        p.passes = p.half == HalfStepKernel::MatrixCore8 ? 2 : 4;
        p.step_lpw = 16;  // (the matrix-core kernels map a walker to 16 lanes x 2 elements in either element type)
    }

    // One launch per ensemble step (full_step_kernel.hpp) while the ensemble is small enough that a half-step
    // launch is bounded by its launch boundary and latencies rather than by HBM; needs the whole ensemble here.
    // A rank of a split ensemble takes the same kernels for its slice (they repeat red updates owned by other ranks,
    // so the ranks exchange rows once per ensemble step), by the size of what it updates.
    const bool whole = s.shard_count == s.n && s.shard_begin == 0;
    // (measured, 32 dims fp64, us per ensemble step full / half: isotropic 32 768 walkers 7 % in favour of full steps;
    //  dense with the matrix-core half-step kernel 10.75 / 10.06 at 32 768, 5.47 / 7.28 at 16 384: profiles/r03_mc_probe_e.txt)
    const long full_step_max = knobs.full_step_max_walkers >= 0 ? knobs.full_step_max_walkers : (p.matrix_core_half() ? 32767 : 32768);
    if ((s.comm_world >= 1 ? (knobs.comm_full_step != 0 && knobs.full_step != 0) : (whole && knobs.full_step != 0)) && 2 * launch_walkers <= full_step_max)
    {
        // (a calculator without the kernel has an empty slot: such a handle steps by half-steps)
        p.full = s.full_step ? FullStepKernel::Plain : FullStepKernel::None;
        p.full_wpb = kWavesPerBlock * (64 / s.lpw);
        if (s.full_step_mc && mc_stretch && s.W < (1 << 24))  // (it addresses rows by 24-bit products)
        {
            p.full = FullStepKernel::MatrixCore;
            p.full_wpb = kWavesPerBlock * 8;
        }
    }
    p.compact_exchange = s.comm_world > 1 && knobs.comm_compact != 0;
    p.have_task_table = (size_t)3 * s.n * kJumpEntryBytes <= ((size_t)knobs.task_table_mb << 20);

    p.graph_steps = s.graph_steps == 0 ? (int)default_graph_steps(s, knobs) : s.graph_steps;
    // HIP cannot capture on the legacy default stream (hipErrorStreamCaptureUnsupported): a caller that hands over
    // NULL / hipStreamLegacy gets plain launches instead of graph replays
    if (!s.can_capture) p.graph_steps = -1;
    // Draw records made ahead of the step launches, a batch of steps per launch (fill_draws_batch_kernel): for the
    // matrix-core full-step kernel of one whole ensemble on one device.
    // (only for handles that step by graph replays: with plain launches -- the caller's legacy default stream -- every
    //  step would drag a fill launch of its own along, and a replay's worth of record memory would sit unused)
    if (p.full == FullStepKernel::MatrixCore && s.chains == 1 && s.comm_world < 1 && whole && knobs.batch_draws != 0 && knobs.no_draw_wave == 0 && p.graph_steps >= 1)
    {
        // (by default as many steps as a graph replays: one fill launch per replay)
        const long want = knobs.batch_draws > 0 ? knobs.batch_draws : (long)p.graph_steps;
        p.batch_draws = (int)(want > 512 ? 512 : want);
    }
    p.partial_slots = p.graph_steps >= 1 ? p.graph_steps : 1;
    const unsigned half_blocks = p.grid_blocks_for(s.shard_count), full_blocks = p.full_grid_blocks_for(s.shard_count);
    p.partial_waves = (int)(p.full != FullStepKernel::None && full_blocks > half_blocks ? full_blocks : half_blocks) * kWavesPerBlock;
    // a fifth wavefront per workgroup computes the next draws when that is at most two rounds of 64 draws
    p.half_draw_wave = (3 * kWavesPerBlock * (64 / p.step_lpw) * p.passes <= 128 && knobs.no_draw_wave == 0) ? 1 : 0;
    // the next draws by four extra wavefronts (two per colour) when that is one round of 64 draws each
    p.full_draw_wave = (p.full != FullStepKernel::None && 3 * ((p.full_wpb + 1) / 2) <= 64 && knobs.no_draw_wave == 0) ? 1 : 0;
    return p;
}

// Mover::DifferentialEvolution (DeSampler, diffevo.hip): the dense Gaussian's product on the matrix cores
// (de_update_mfma_kernel: fp64, even D up to 32).  Walkers per wavefront of the matrix-core update kernel, or 0: the
// plain kernel.  A launch updates the n walkers of one colour.
inline int plan_de_update(const StepShape& s, const Knobs& knobs)
{
    if (!(s.de_update_mc && matrix_core_shape(s, knobs, s.n) && s.D <= 32)) return 0;
    // 16 walkers per wavefront once the chip is full (as the stretch kernels: MCMCPP_HIP_MATRIX_CORE_4PASS_WALKERS)
    return s.n >= knobs.matrix_core_4pass.value_or(32768) ? 16 : 8;
}
}  // namespace mcmcpp
