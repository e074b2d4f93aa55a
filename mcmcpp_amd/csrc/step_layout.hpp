// step_layout.hpp -- where the step kernels and the host agree on bits and bytes: the packed launch words (HotBits,
// DeHotBits) and the strides of the per-chain arrays (ChainGeometry).  No HIP header: this file compiles with the host
// compiler alone, and tests/test_step_layout.py pins every packed value and every offset there.  The kernels
// (stretch_kernel.hpp, full_step_kernel.hpp, diffevo_kernel.hpp, batch.hip) and the host (launch_build.hpp, mcmcpp_hip.hip)
// take them from here; nobody else shifts a hot bit or multiplies out a chain stride.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "canonical.hpp"  // MCMCPP_HD
#include "step_plan.hpp"  // kJumpEntryBytes

namespace mcmcpp
{

// One field of a packed 32-bit launch word.
template <int SHIFT, int WIDTH>
struct BitField
{
    static_assert(SHIFT >= 0 && WIDTH >= 1 && SHIFT + WIDTH <= 32, "inside the word");
    static constexpr int shift = SHIFT, width = WIDTH;
    static constexpr uint32_t low = WIDTH == 32 ? ~0u : (1u << (WIDTH % 32)) - 1u;  // the largest value
    static constexpr uint32_t mask = low << SHIFT;
    static MCMCPP_HD uint32_t put(int v) { return (uint32_t)v << SHIFT; }
    static MCMCPP_HD int get(uint32_t bits) { return (int)((bits >> SHIFT) & low); }
};
// All fields of a word: the bits they occupy between them, and whether no two of them overlap (sum and union agree)
template <class... F>
struct FieldList
{
    static constexpr uint32_t mask = (F::mask | ...);
    static constexpr bool disjoint = ((uint64_t)F::mask + ...) == (uint64_t)mask;
};

// Hot scalars of a stretch launch, packed so that the arguments every wavefront needs before its first memory
// access fit the 16 dwords the command processor preloads into SGPRs (-amdgpu-kernarg-preload-count=16);
// everything else stays in the by-value HalfStepArgs and is fetched from the kernarg segment on demand.
struct HotBits
{
    typedef BitField<0, 12> Dims;
    typedef BitField<12, 8> Passes;
    typedef BitField<20, 1> Color;       // (matrix-core full-step launches: the draw records were made ahead, HalfStepArgs::draw_wave == 2)
    typedef BitField<21, 1> VecOk;
    typedef BitField<22, 1> NIsPow2;     // (packed, read by no kernel: the draws take it from HalfStepArgs)
    typedef BitField<23, 1> UseCtlSave;
    typedef BitField<24, 1> DrawParity;
    typedef BitField<25, 1> DrawWave;
    typedef BitField<26, 1> PosParity;   // full-step kernels' position-buffer parity
    typedef BitField<27, 1> DirectJump;  // the one-entry-per-draw jump table exists
    typedef BitField<28, 4> Chains;      // chains - 1

    static MCMCPP_HD uint32_t pack(int dims, int passes, int color, int vec_ok, int n_is_pow2, int use_ctl_save, int draw_parity, int draw_wave,
                                   int pos_parity, int direct_jump, int chains)
    {
        return Dims::put(dims) | Passes::put(passes) | Color::put(color) | VecOk::put(vec_ok) | NIsPow2::put(n_is_pow2) | UseCtlSave::put(use_ctl_save) |
               DrawParity::put(draw_parity) | DrawWave::put(draw_wave) | PosParity::put(pos_parity) | DirectJump::put(direct_jump) | Chains::put(chains - 1);
    }
    static MCMCPP_HD int dims(uint32_t b) { return Dims::get(b); }
    static MCMCPP_HD int passes(uint32_t b) { return Passes::get(b); }
    static MCMCPP_HD int color(uint32_t b) { return Color::get(b); }
    static MCMCPP_HD int vec_ok(uint32_t b) { return VecOk::get(b); }
    static MCMCPP_HD int n_is_pow2(uint32_t b) { return NIsPow2::get(b); }
    static MCMCPP_HD int use_ctl_save(uint32_t b) { return UseCtlSave::get(b); }
    static MCMCPP_HD int draw_parity(uint32_t b) { return DrawParity::get(b); }
    static MCMCPP_HD int draw_wave(uint32_t b) { return DrawWave::get(b); }
    static MCMCPP_HD int pos_parity(uint32_t b) { return PosParity::get(b); }
    static MCMCPP_HD int direct_jump(uint32_t b) { return DirectJump::get(b); }
    static MCMCPP_HD int chains(uint32_t b) { return Chains::get(b) + 1; }

    typedef FieldList<Dims, Passes, Color, VecOk, NIsPow2, UseCtlSave, DrawParity, DrawWave, PosParity, DirectJump, Chains> All;
};
static_assert(HotBits::All::disjoint && HotBits::All::mask == 0xFFFFFFFFu, "HotBits fields overlap or leave a bit of the word unnamed");
constexpr int kMaxChains = 16;
static_assert(kMaxChains == 1 << HotBits::Chains::width, "kMaxChains is what the chains field holds");

// hot_bits of the differential-evolution update kernels (step: ensemble step inside the graph replay, matrix-core kernel only)
struct DeHotBits
{
    typedef BitField<0, 12> Dims;
    typedef BitField<12, 1> Color;
    typedef BitField<14, 1> VecOk;
    typedef BitField<16, 16> Step;

    static MCMCPP_HD uint32_t pack(int dims, int color, int vec_ok, int step = 0) { return Dims::put(dims) | Color::put(color) | VecOk::put(vec_ok) | Step::put(step); }
    static MCMCPP_HD int dims(uint32_t b) { return Dims::get(b); }
    static MCMCPP_HD int color(uint32_t b) { return Color::get(b); }
    static MCMCPP_HD int vec_ok(uint32_t b) { return VecOk::get(b); }
    static MCMCPP_HD int step(uint32_t b) { return Step::get(b); }

    typedef FieldList<Dims, Color, VecOk, Step> All;
};
static_assert(DeHotBits::All::disjoint && DeHotBits::All::mask == 0xFFFF5FFFu, "DeHotBits fields overlap, or name more than all bits but 13 and 15");

// ---- ChainGeometry ----------------------------------------------------------------------------------------------------
// Several independent ensembles ("chains": BASELINE config 4 on one GPU) stepped by ONE launch: workgroup row
// blockIdx.y is chain blockIdx.y.  Every per-chain array is the single-chain array repeated with a fixed stride that
// follows from n and D alone, so the kernels need no further arguments (the chain count travels in the hot bits):
//   positions (both buffers)   [chains][2n][D]
//   log-posteriors + counters  [chains]{[2][2n] T, [2n] u32}
//   control + run records      [chains]{StepCtl[2], pad to kRunBehindCtlBytes, RunInfo, pad to kCtlChainStride}
//   draw records               [chains][2][2][n], then the shared jump tables
//   partial accepted counts    [chains][partial_slots][2][partial_waves]
// The chains differ in their seed (seed + chain: same stream increment, hence the same jump tables) and, once the host has
// given any chain a parameter block of its own (mcmcpp_hip_set_chain_params), in their calculator parameters:
//   calculator parameters      [chains][params_chain_stride]: the block (P^T for the dense target), zero padding to 256 bytes,
//                              then -- dense target, D <= 32 -- the matrix-core kernels' zero-padded 32 x 32 P^T
// calc_params and calc_params_padded point into row 0 and the MC kernels step both by chain * params_chain_stride (0: shared).
constexpr int kCtlChainStride = 512;
constexpr int kRunBehindCtlBytes = 256;
constexpr size_t kDrawRecBytes = 32;  // sizeof(DrawRec<T>)

// `p` moved on by `bytes`
template <class P>
MCMCPP_HD P* offset_bytes(P* p, size_t bytes) { return (P*)((char*)p + bytes); }
// elements (records) in front of chain `chain`'s positions (draw records); bytes between two chains' log-posterior pieces
MCMCPP_HD size_t pos_chain_offset(int chain, int n, int dims) { return (size_t)chain * 2 * (size_t)n * (size_t)dims; }
MCMCPP_HD size_t draws_chain_offset(int chain, int n) { return (size_t)chain * 4 * (size_t)n; }
// how many draw records / partial accepted counts `chains` chains have between them
MCMCPP_HD size_t draws_count(int chains, int n) { return draws_chain_offset(chains, n); }
MCMCPP_HD size_t partials_count(int chains, int slots, int waves) { return (size_t)chains * (size_t)slots * 2 * (size_t)waves; }
template <class T>
MCMCPP_HD size_t logp_chain_stride_bytes(int n) { return (size_t)4 * (size_t)n * sizeof(T) + (size_t)2 * (size_t)n * sizeof(uint32_t); }
// a control or run record of chain 0 -> the same record of chain `chain`
template <class P>
MCMCPP_HD P* ctl_of_chain(P* p, int chain) { return offset_bytes(p, (size_t)chain * kCtlChainStride); }
// the same as offsets of a load from the first control record of chain 0: chain `chain`'s first control record, and its run
// record seen from its control record `ctl_index` (0 or 1)
constexpr int kStepCtlBytes = 64;  // sizeof(StepCtl)
MCMCPP_HD unsigned ctl_chain_offset(int chain) { return (unsigned)chain * (unsigned)kCtlChainStride; }
MCMCPP_HD unsigned run_behind_ctl_offset(int chain, int ctl_index) { return ctl_chain_offset(chain) + (unsigned)kRunBehindCtlBytes - (unsigned)ctl_index * (unsigned)kStepCtlBytes; }
// a pointer into the log-posterior piece (log-posteriors or counters) of chain 0 -> the same place of chain `chain`
template <class T, class P>
MCMCPP_HD P* logp_of_chain(P* p, int n, int chain) { return offset_bytes(p, (size_t)chain * logp_chain_stride_bytes<T>(n)); }
// first record of the buffer of (parity, colour) inside a chain's draw records
MCMCPP_HD size_t draw_buffer_index(int parity, int color, int n) { return ((size_t)parity * 2 + (size_t)color) * (size_t)n; }
// a wavefront's accepted count of one colour of one ensemble step
MCMCPP_HD size_t partial_index(int chain, int slots, uint32_t slot, int color, int waves, int wave) { return (((size_t)chain * (size_t)slots + (size_t)slot) * 2 + (size_t)color) * (size_t)waves + (size_t)wave; }

// The jump tables live right behind the draw records, at offsets that follow from the number of walkers per colour
// alone, so that a kernel can reach them from its preloaded record pointer without touching the kernarg segment
// (a draw wavefront's first loads would otherwise wait for a cold scalar miss):
//   [records: 4 n x 32 B][task_jump: 3 n entries, if built][jump_hi: ceil(n / 256) entries][jump_lo: 256 entries]
// every piece rounded up to 256 bytes.
// (`chains` independent ensembles stepped by one launch share the tables: same stream increment)
MCMCPP_HD size_t round_up_256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
MCMCPP_HD size_t tables_offset_task(int n, int chains = 1) { return round_up_256((size_t)4 * (size_t)n * kDrawRecBytes * (size_t)chains); }
MCMCPP_HD size_t tables_offset_hi(int n, bool direct, int chains = 1) { return tables_offset_task(n, chains) + (direct ? round_up_256((size_t)3 * (size_t)n * kJumpEntryBytes) : 0); }
MCMCPP_HD size_t tables_offset_lo(int n, bool direct, int chains = 1) { return tables_offset_hi(n, direct, chains) + round_up_256((size_t)((n + 255) / 256) * kJumpEntryBytes); }
MCMCPP_HD size_t tables_total_bytes(int n, bool direct, int chains = 1) { return tables_offset_lo(n, direct, chains) + 256 * kJumpEntryBytes; }

}  // namespace mcmcpp
