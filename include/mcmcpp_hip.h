/*
 * mcmcpp_hip.h -- C ABI of libmcmcpp_hip.so, the MI355X (gfx950) implementation of the reference's
 * stretch-move ensemble step.
 *
 * The reference (jmatta1/MCMCpp) is a header-only C++ template library and has no FFI of its own; the
 * boundary below is what its sampler facade would bind for this path.  Each entry point names the
 * reference interface it stands in for (paths relative to /root/reference).  The header-only host
 * facade in include/MCMCpp/ (same class names and template parameters as the reference) is the only
 * intended caller; INTEGRATION.md shows the binding.
 *
 * Conventions: plain C types only; every function returns MCMCPP_HIP_OK (0) or a positive error code
 * and never throws; pointers are caller-owned HOST memory unless the name says `device`; a handle is
 * used from one host thread at a time (the facade keeps the reference's sampler mutex,
 * ParallelEnsembleSampler.h:184-210); the handle owns all device buffers, streams and graphs.
 *
 * Data layout (same as the reference's setInitialWalkerPos arguments and Chain cells,
 * EnsembleSampler.h:220-230, Chain/ChainBlock.h:125-131):
 *   positions[w*D + p]   walker-major, parameter-contiguous; walkers [0, W/2) are the red half,
 *                        [W/2, W) the black half (EnsembleSampler.h:211-215)
 *   logp[w]              the walker's auxiliary value = log-posterior of its position
 *   chain[s*W*D + w*D + p]  stored step s
 */
#ifndef MCMCPP_HIP_H
#define MCMCPP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCMCPP_HIP_ABI_VERSION 2

/* return codes */
enum {
    MCMCPP_HIP_OK = 0,
    MCMCPP_HIP_E_ARG = 1,         /* bad argument (the reference asserts: EnsembleSampler.h:207-208,327,335) */
    MCMCPP_HIP_E_HIP = 2,         /* a HIP runtime call failed; see mcmcpp_hip_last_error */
    MCMCPP_HIP_E_NO_DEVICE = 3,   /* no gfx950 device / device ordinal out of range */
    MCMCPP_HIP_E_UNSUPPORTED = 4, /* configuration outside what the kernels were built for */
    MCMCPP_HIP_E_STATE = 5,       /* run/get before set_state */
    MCMCPP_HIP_E_NOMEM = 6,
    MCMCPP_HIP_E_COMM = 7,        /* the collective library (RCCL) is missing or one of its calls failed */
    MCMCPP_HIP_E_CALLBACK = 8     /* the batch log-posterior callback returned non-zero (mcmcpp_hip_set_batch_calculator) */
};

/* ParamType of the reference templates */
enum { MCMCPP_HIP_F64 = 0, MCMCPP_HIP_F32 = 1 };

/* device Calculators (reference concept: ParamType calcLogPostProb(ParamType*),
 * Utility/UserOjbectsTest.h:144-145); host twins live in include/MCMCpp/Device/Calculators.h */
enum {
    MCMCPP_HIP_CALC_ISO_GAUSSIAN = 0,      /* params: none                    */
    MCMCPP_HIP_CALC_DENSE_GAUSSIAN = 1,    /* params: P[D*D] row-major        */
    MCMCPP_HIP_CALC_ROSENBROCK = 2,        /* params: a, b, c                 */
    MCMCPP_HIP_CALC_SKEWED_GAUSSIAN_2D = 3, /* params: epsilon; requires D == 2 */
    MCMCPP_HIP_CALC_BATCH = 4               /* params: none; a host callback evaluates each half-step's proposals in one
                                               batch (mcmcpp_hip_set_batch_calculator) */
};

/* calculator ids from here on belong to user plug-ins (mcmcpp_hip_register_calculator) */
#define MCMCPP_HIP_CALC_USER_BASE 1000

typedef struct mcmcpp_hip_sampler mcmcpp_hip_sampler;

/* Stands in for the constructor arguments of EnsembleSampler (EnsembleSampler.h:66-67,199-218),
 * ParallelEnsembleSampler (ParallelEnsembleSampler.h:119-120) and StretchMove (Movers/StretchMove.h:62-66). */
typedef struct mcmcpp_hip_config {
    uint32_t struct_size;    /* sizeof(mcmcpp_hip_config) */
    int32_t dtype;           /* MCMCPP_HIP_F64 / MCMCPP_HIP_F32 */
    int32_t num_walkers;     /* W: even and > 2*D */
    int32_t num_params;      /* D: 1..1024 */
    int32_t calc_id;         /* MCMCPP_HIP_CALC_* */
    int32_t calc_params_len; /* number of dtype elements behind calc_params */
    const void* calc_params; /* host pointer, copied */
    uint64_t seed;           /* randSeed, sign-extended to 64 bit (MultiSampler.h:54) */
    uint64_t stream;         /* pcg stream; EnsembleSampler uses 0 (EnsembleSampler.h:217) */
    int32_t device;          /* HIP device ordinal, -1 = the current device */
    /* Walkers of each half updated by this handle: [shard_begin, shard_begin + shard_count) of W/2.
     * shard_count == 0 means the whole half.  A sharded handle still holds the full ensemble (the
     * complementary half must be readable); the caller exchanges the updated rows between handles
     * after every half-step (see mcmcpp_hip_half_step_async). */
    int32_t shard_begin;
    int32_t shard_count;
    int32_t graph_steps;     /* ensemble steps per hipGraph replay; 0 = library default, -1 = no graphs */
    /* stretch scale a = gw_alpha_num / gw_alpha_den of GwDistribution<ParamType, Num, Denom>
     * (Utility/GwDistribution.h:45-55; StretchMove's default is 2/1); 0/0 selects 2/1 */
    int32_t gw_alpha_num;
    int32_t gw_alpha_den;
    void* device_positions;  /* optional caller-owned DEVICE buffer of W*D elements used in place of an
                                internal one (e.g. memory registered with a collective library) */
    void* hip_stream;        /* hipStream_t to launch on when MCMCPP_HIP_FLAG_CALLER_STREAM is set; otherwise ignored and the
                                handle owns a private non-blocking stream.  NULL (the legacy default stream) is accepted,
                                but HIP cannot capture graphs on it: such a handle steps with plain launches */
    uint32_t flags;          /* MCMCPP_HIP_FLAG_* */
    uint32_t mover;          /* MCMCPP_HIP_MOVER_*: which Mover::updateWalker the kernels implement; 0 = StretchMove */
    /* One ensemble split over comm_world GPUs (one handle per GPU; stands in for ParallelEnsembleSampler's threadCount
     * workers, ParallelEnsembleSampler.h:119-120,285-291, and the red/black controller's two barriers per step,
     * Threading/RedBlkCtrlerSpinLock.h:240-322).  comm_world >= 1 makes this handle rank comm_rank of an RCCL
     * communicator (created from comm_id, or taken from comm) and lets mcmcpp_hip_run step the split ensemble: the
     * handle's shard must be the rank's slice, [comm_rank * (W/2) / comm_world, + (W/2) / comm_world) -- shard_count = 0
     * selects exactly that -- and W/2 must divide by comm_world.  Every rank calls set_state / run / get_state with the
     * same arguments; the exchanges (one ncclAllGather per ensemble step, see mcmcpp_hip_last_run_exchange) are enqueued on
     * the launch stream by run itself.  If the preparation of a run fails on one rank, every rank's run returns an error
     * and none has launched anything (the ranks agree on a status word first).  0 = no communicator. */
    int32_t comm_world;
    int32_t comm_rank;
    const void* comm_id;     /* MCMCPP_HIP_COMM_ID_BYTES bytes made by mcmcpp_hip_comm_unique_id on one rank and handed to
                                all ranks by the caller's own means (file, MPI, torch.distributed ...), or NULL */
    void* comm;              /* or: an existing ncclComm_t of comm_world ranks on this handle's device (borrowed) */
    /* Independent ensembles ("chains") stepped by the same kernel launches -- what several EnsembleSampler objects with
     * seeds randSeed, randSeed + 1, ... would compute one after the other (BASELINE config 4 on one GPU).  Chain k is an
     * ensemble of num_walkers walkers of its own, seeded with seed + k on the same stream.  0 or 1: one ensemble.  With
     * K = num_chains > 1 every array argument gains a leading chain dimension: set_state positions[K][W][D], logp[K][W];
     * run chain_out[K][n_saved][W][D] (chain k's stored steps are contiguous, like that sampler's own Chain),
     * accepted_per_step[K][steps]; get_state likewise.  Counters are summed over the chains.  Whole ensembles on one
     * device (no shards, no communicator); at most 16 chains.  All chains share calc_params until
     * mcmcpp_hip_set_chain_params gives a chain a block of its own (one model fitted to K data sets in the same launches). */
    int32_t num_chains;
    int32_t reserved0;
} mcmcpp_hip_config;

#define MCMCPP_HIP_COMM_ID_BYTES 128
/* ncclGetUniqueId: the rendezvous token of a new communicator (call on one rank). */
int mcmcpp_hip_comm_unique_id(void* id_out);

/* Movers (reference MCMCpp/Movers/).  DIFFERENTIAL_EVOLUTION = Mover::DifferentialEvolution
 * (Movers/DifferentialEvolution.h:80-112) with the gamma and jitter bounds its constructors set -- the samplers work on
 * a copy of the user's mover whose copy constructor re-initialises both, so overrideGamma / overrideRandBounds never
 * reach a sampler in the reference either.  Same stream, same draws, same chain as the reference, bit for bit
 * (tests/test_diffevo.py); one whole ensemble per handle: run / set_state / get_state / counters / calc_logp are
 * supported, seek, shards and half_step_async are not (the stream position depends on the draws thrown away so far). */
#define MCMCPP_HIP_MOVER_STRETCH 0u
#define MCMCPP_HIP_MOVER_DIFFERENTIAL_EVOLUTION 1u

/* launch every kernel and copy on the caller's stream (config.hip_stream), so that the caller's own work on
 * that stream -- e.g. RCCL collectives issued through torch.distributed -- is ordered with the half-steps */
#define MCMCPP_HIP_FLAG_CALLER_STREAM 1u

/* User-compiled device Calculators (the reference takes the Calculator as a template argument of the Mover,
 * Movers/StretchMove.h:42-43; here it is a device functor built with hipcc against
 * mcmcpp_amd/csrc/mcmcpp_hip_plugin.hpp).  table_f64 / table_f32 are what the plug-in's
 * mcmcpp_hip_plugin_<name>_f64() / _f32() return (either may be NULL); calc_id >= MCMCPP_HIP_CALC_USER_BASE;
 * params_len >= 0 makes mcmcpp_hip_create insist on exactly that many parameters, -1 accepts any.
 * Registering an id again replaces it (handles created earlier keep what they were created with). */
int mcmcpp_hip_register_calculator(int32_t calc_id, const void* table_f64, const void* table_f32, int32_t params_len);

/* Batch targets (calc_id MCMCPP_HIP_CALC_BATCH): the log-posterior is whatever the caller computes for a whole half-step
 * of proposals at once -- a GEMM over a dataset, a neural-network density, a torch function.  Every update of a half-step
 * reads only the other colour (StretchMove.h:105-113), so the W/2 proposals of a half-step are formed first (one kernel),
 * evaluated in one batch by the callback, and accepted (a second kernel): the reference's loop, operation for operation.
 * A callback that computes the same bits as a built-in Calculator reproduces that Calculator's chains bit for bit.
 *
 *   proposals  device memory, [count][num_params] row-major elements of the handle's dtype
 *   logp_out   device memory, [count] elements: the callback writes logp of every proposal here
 *   hip_stream the handle's launch stream (hipStream_t); the accept kernel follows on it
 *
 * Contract:
 *   - the callback runs on the thread that executes the run: for mcmcpp_hip_run_async that is the handle's worker thread;
 *   - it is called once per half-step with count = W/2; mcmcpp_hip_calc_logp calls it in chunks of at most W/2, and
 *     mcmcpp_hip_calc_logp_device likewise, with pointers into the caller's own device arrays instead of the handle's
 *     buffers (a callback must not assume it is handed device_proposals / device_logp);
 *   - it either enqueues its work on hip_stream or finishes that work before it returns;
 *   - it returns 0 on success.  Any other value ends the run with MCMCPP_HIP_E_CALLBACK (the message names the value), and
 *     the walker state counts as undefined until the next set_state.
 * Steps are plain launches on the handle's one stream (propose, callback, accept per half-step; the per-step accepted
 * count behind each black half-step): no graph capture, no parallel branches.  Refused at create: the differential-
 * evolution mover, num_chains > 1, shards and communicators; mcmcpp_hip_half_step_async returns MCMCPP_HIP_E_UNSUPPORTED.
 * set_state, run and calc_logp return MCMCPP_HIP_E_STATE until a callback has been set.
 */
typedef int (*mcmcpp_hip_batch_logp_fn)(void* user, const void* proposals, void* logp_out, int64_t count, int32_t num_params,
                                        void* hip_stream);

/* Set (or replace) the batch callback of a handle created with MCMCPP_HIP_CALC_BATCH.  device_proposals (W/2 * D elements)
 * and device_logp (W/2 elements) are optional caller-owned DEVICE buffers, 16-byte aligned, that the library forms the
 * proposals in and the callback writes into (e.g. the storage of two torch tensors); NULL: the library allocates its own. */
int mcmcpp_hip_set_batch_calculator(mcmcpp_hip_sampler* h, mcmcpp_hip_batch_logp_fn fn, void* user, void* device_proposals,
                                    void* device_logp);

/* EnsembleSampler::EnsembleSampler / ~EnsembleSampler */
int mcmcpp_hip_create(const mcmcpp_hip_config* cfg, mcmcpp_hip_sampler** out);
void mcmcpp_hip_destroy(mcmcpp_hip_sampler* h);

/* message of the last failure on this handle (h == NULL: last failure of mcmcpp_hip_create on this thread) */
const char* mcmcpp_hip_last_error(const mcmcpp_hip_sampler* h);

/* EnsembleSampler::setInitialWalkerPos (EnsembleSampler.h:220-230): uploads positions[W*D] and
 * auxValues[W], zeroes the per-walker counters and rewinds the random stream to its first draw. */
int mcmcpp_hip_set_state(mcmcpp_hip_sampler* h, const void* positions, const void* logp);

/* EnsembleSampler::runMCMC (EnsembleSampler.h:284-310) with the slicing mode of setSlicingMode folded in:
 * executes n_saved*interval ensemble steps (red half-step then black half-step each,
 * EnsembleSampler.h:341-354); the last step of every `interval` is a stored step.
 *   chain_out          n_saved*W*D elements receiving the stored steps, or NULL to store nothing
 *   accepted_per_step  n_saved*interval counters (accepted proposals of each executed ensemble step), or NULL
 * Synchronous: returns when the results are in host memory. */
int mcmcpp_hip_run(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* chain_out,
                   uint32_t* accepted_per_step);

/* The same run on a worker thread owned by the handle, so that the caller can look at stored steps while the device keeps
 * stepping -- what a PostStepAction needs (EnsembleSampler.h:356-359: called after every ensemble step with the chain as it
 * stands).  run_async returns at once; wait_stored(count) returns when the first `count` stored steps of this run are
 * complete in chain_out (or with the run's error code if it ended before that); run_wait joins the worker and returns what
 * mcmcpp_hip_run would have returned.  Between run_async and run_wait the handle accepts only wait_stored. */
int mcmcpp_hip_run_async(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* chain_out, uint32_t* accepted_per_step);
int mcmcpp_hip_wait_stored(mcmcpp_hip_sampler* h, int64_t count);
int mcmcpp_hip_run_wait(mcmcpp_hip_sampler* h);

/* mcmcpp_hip_run with the stored steps left in DEVICE memory: the same steps, the same stream, the same counters and the same
 * walker state afterwards, but the chain never crosses the host link.  What follows a run -- covariance, histograms,
 * autocorrelation times (the *_device entry points below), the log-posteriors of the stored rows
 * (mcmcpp_hip_calc_logp_device), the caller's own kernels or torch -- reads it where it was written.
 *   device_chain       caller-owned memory of the handle's device, 16-byte aligned, K*n_saved*W*D elements laid out
 *                      [K][n_saved][W][D] exactly as mcmcpp_hip_run lays out chain_out (K = max(num_chains, 1)).  Nothing
 *                      outside it is written.  NULL only with n_saved == 0.
 *   accepted_per_step  HOST memory as for mcmcpp_hip_run (it is small), or NULL
 * Synchronous: when it returns every stored step is complete in device_chain and visible to work on any stream.
 * The launch that makes a stored step writes it to its final place: there is no ring, no staging buffer, no copy and no
 * host wait for the chain inside the run, whichever kernels step the handle (every kernel forms the chain cell's address
 * in 64 bits, so device_chain may lie anywhere and be of any size).
 * Supported: stretch-move handles that hold a whole ensemble (several chains and per-chain parameters included), the
 * differential-evolution mover and batch targets.  Returns MCMCPP_HIP_E_ARG (with a message) for a NULL pointer with
 * n_saved > 0, a pointer that is not 16-byte aligned, one that hipPointerGetAttributes does not report as memory of the
 * handle's device -- a host pointer, pinned or not, is refused before anything is launched, never dereferenced -- and a
 * destination that does not end inside the allocation hipMemGetAddressRange reports around the pointer (the array lies
 * in ONE allocation); MCMCPP_HIP_E_UNSUPPORTED for sharded handles (they store through mcmcpp_hip_bind_device_chain) and
 * handles with a communicator; MCMCPP_HIP_E_STATE as mcmcpp_hip_run.
 * run_device_async pairs with mcmcpp_hip_wait_stored and mcmcpp_hip_run_wait like mcmcpp_hip_run_async: wait_stored(c)
 * returns when the first c stored steps of every chain are complete in device_chain; a copy or kernel enqueued on any
 * stream after it has returned reads them.  (Argument errors of the asynchronous form are reported by run_wait.) */
int mcmcpp_hip_run_device(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* device_chain, uint32_t* accepted_per_step);
int mcmcpp_hip_run_device_async(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, void* device_chain,
                                uint32_t* accepted_per_step);

/* Pinned (page-locked, device-visible) host memory for Chain blocks (stands in for the allocation of
 * Chain/ChainBlock.h:115-131).  When chain_out of mcmcpp_hip_run lies in such memory the step launches forward stored
 * steps straight into it: no staging ring on the host, no host copy.  NULL when the allocation fails. */
void* mcmcpp_hip_host_alloc(uint64_t bytes);
void mcmcpp_hip_host_free(void* p);

/* Device memory for a Chain that never leaves the GPU (the facade's MCMCPP_CHAIN_MEMORY=device: one contiguous allocation
 * [steps][W][D] that mcmcpp_hip_run_device writes and the *_device analysis entry points read).
 *   device_alloc   `bytes` of memory of device `device` (-1 = the current one), or NULL when the allocation fails
 *   device_free    gives it back (NULL is accepted)
 *   device_copy    `bytes` from src to dst, each host or device memory (the runtime tells them apart); returns when the copy
 *                  is done
 * device_chain_last_error: the message of the last failure of these and of device_chain_compact on the calling thread. */
void* mcmcpp_hip_device_alloc(int32_t device, uint64_t bytes);
void mcmcpp_hip_device_free(void* p);
int mcmcpp_hip_device_copy(void* dst, const void* src, uint64_t bytes);
const char* mcmcpp_hip_device_chain_last_error(void);

/* Chain::resetChainForSubSampling / sliceAndBurnChain (reference MCMCpp/Chain/Chain.h:268-305) on a chain in device memory:
 * n_steps contiguous stored steps of step_elems elements each ([n_steps][W][D], step_elems = W*D), compacted in place.  The
 * reference's selection: burn_in = 0 with interval = 1 changes nothing; no step is kept when none is left behind the burn-in
 * or fewer than `interval` are; otherwise step burn_in + j*interval becomes step j.  *kept = the stored steps afterwards
 * (may be NULL); steps behind them keep bytes of no meaning.  Destinations are moved in ascending waves, one launch each,
 * none of which writes a step that it or a later one reads (mcmcpp_amd/csrc/chain_compact_plan.hpp): the result equals a
 * copy into a fresh array, byte for byte.  Steps move in 16-byte pieces when a step is a whole number of them and
 * device_steps is 16-byte aligned, element by element otherwise.  device: the device the memory belongs to (-1 = current).
 * MCMCPP_HIP_E_ARG (with a message) for a pointer that is not memory of that device or n_steps steps that do not end inside
 * its allocation: nothing is launched then.  Returns when the chain is compacted. */
int mcmcpp_hip_device_chain_compact(int32_t dtype, int32_t device, void* device_steps, int64_t n_steps, int64_t step_elems,
                                    int64_t burn_in, int64_t interval, int64_t* kept);

/* Current walker state (what Walker::getCurrState / getCurrAuxData / getAcceptedProposals expose,
 * Walker/Walker.h:111-122).  n_accept[w] counts accepted proposals since set_state or reset_counters;
 * the reference additionally counts the initial placement (Walker.h:76,168) -- the facade adds it.
 * Counts stay below 2^31 (the reference's counters are 32-bit ints as well).  Any pointer may be NULL. */
int mcmcpp_hip_get_state(mcmcpp_hip_sampler* h, void* positions, void* logp, uint32_t* n_accept);

/* Checkpoint / resume.  The random stream has no per-walker state: (seed, stream, ensemble steps done) address
 * every draw, so a checkpoint is get_state's arrays plus one integer.  After set_state (which rewinds to the
 * first draw) this repositions the stream as if `ensemble_steps_done` steps had been executed, without touching
 * walkers or counters.  (The reference cannot do this: its engine state is private to the Mover.) */
int mcmcpp_hip_seek(mcmcpp_hip_sampler* h, uint64_t ensemble_steps_done);

/* EnsembleSampler::reset (EnsembleSampler.h:312-322): zero the counters, keep positions and stream. */
int mcmcpp_hip_reset_counters(mcmcpp_hip_sampler* h);

/* getAcceptedSteps / getTotalSteps material (EnsembleSampler.h:260-282), plus two parity diagnostics:
 *   accepted        sum of n_accept over the walkers this handle updates
 *   ensemble_steps  ensemble steps executed since set_state / reset_counters
 *   near_ties       accept decisions whose margin was within a few ulp (could flip under another libm log).
 *                   The rule: |ln U - delta| <= tie_eps * (|ln U| + |(D-1) ln z| + |logp_new| + |logp_old|) AND the
 *                   margin |ln U - delta| is finite, that is, every operand of the accept test is finite.  A
 *                   proposal outside the support (logp_new = -inf), a walker that still sits outside it
 *                   (logp_old = -inf) and +inf on either side are decided by the comparison alone, which no
 *                   rounding of a logarithm can flip: they are not counted.  Neither is a decision with a NaN
 *                   operand (the first comparison is false).
 *   redraws         pcg bounded_rand rejections met (only possible when W/2 is not a power of two; the
 *                   reference would have consumed one more draw there, so trajectories part)
 * Any pointer may be NULL. */
int mcmcpp_hip_get_counters(mcmcpp_hip_sampler* h, uint64_t* accepted, uint64_t* ensemble_steps,
                            uint64_t* near_ties, uint64_t* redraws);

/* Calculator::calcLogPostProb evaluated by the device functor for `count` D-vectors (host in, host out).  With per-chain
 * parameters (mcmcpp_hip_set_chain_params) this is chain 0's calculator. */
int mcmcpp_hip_calc_logp(mcmcpp_hip_sampler* h, const void* positions, int64_t count, void* logp_out);

/* Per-chain calculator parameters.  Give chain `chain` (0 <= chain < K, K = max(num_chains, 1)) its own calculator
 * parameters: `len` elements of the handle's dtype.  `len` must equal the handle's calc_params_len, and the block is checked
 * as at create.  The parameters take effect at the next run / calc_logp.  Stored log-posteriors are NOT recomputed: call
 * mcmcpp_hip_calc_logp_chain and then set_state (which rewinds the stream: mcmcpp_hip_seek puts it back).  Chains that never
 * get their own block keep the parameters given at create.  With K = 1 this changes the handle's target without a new handle.
 * Chain k then computes what a handle of its own with these parameters and seed + k would compute, bit for bit.
 * Returns MCMCPP_HIP_E_ARG (with a message) for a chain out of range, a wrong len, a calculator that takes no parameters
 * (IsoGaussian, the batch target), a block create would refuse, or a NULL pointer; MCMCPP_HIP_E_UNSUPPORTED for the
 * differential-evolution mover, sharded handles, handles with a communicator and handles with caller-owned positions;
 * MCMCPP_HIP_E_STATE while an asynchronous run is in progress.  The first block set allocates K rows of device memory
 * outside the handle's step buffers. */
int mcmcpp_hip_set_chain_params(mcmcpp_hip_sampler* h, int32_t chain, const void* params, int32_t len);

/* mcmcpp_hip_calc_logp with chain `chain`'s parameters (same refusals as mcmcpp_hip_set_chain_params, except that a
 * calculator without parameters is evaluated: all its chains are the same). */
int mcmcpp_hip_calc_logp_chain(mcmcpp_hip_sampler* h, int32_t chain, const void* positions, int64_t count, void* logp_out);

/* mcmcpp_hip_calc_logp_chain with device input and device output and no copies: `count` D-vectors at device_positions
 * (16-byte aligned when a row is a whole number of 16-byte pieces, element-aligned otherwise; e.g. the rows of a chain
 * written by mcmcpp_hip_run_device), their log-posteriors to device_logp_out[count].  Returns when they are there.
 * chain selects chain `chain`'s parameters (0 <= chain < K); differential-evolution handles evaluate with their create-time
 * parameters and batch handles call the callback directly on the caller's rows (both pointers 16-byte aligned), in chunks
 * of at most W/2 rows that are a whole number of 16-byte pieces of log-posteriors, so that the callback is handed 16-byte
 * aligned pointers as in a run (W/2 below 16 / sizeof(element) cannot be cut so: its later chunks are element-aligned)
 * -- for both, chain must be 0.  MCMCPP_HIP_E_ARG for a chain out of range or a pointer that is
 * not memory of the handle's device (checked as for mcmcpp_hip_run_device). */
int mcmcpp_hip_calc_logp_device(mcmcpp_hip_sampler* h, int32_t chain, const void* device_positions, int64_t count,
                                void* device_logp_out);

/* ---- parallel tempering: replica exchange among the chains of one handle ------------------------------- */

/* A ladder of targets is K chains with per-chain parameters (mcmcpp_hip_set_chain_params): chain k's block flattens chain
 * 0's target (dense Gaussian: P_k = beta_k P; Rosenbrock: c_k = beta_k c; a plug-in: beta in its parameter blob).  Between
 * runs, one round proposes to exchange the states of neighbouring chains:
 *   pairs     round r pairs chains (k, k+1) for k = r (mod 2), k+1 < K (pair slot j = k >> 1, at most 8); walker w of chain k
 *             is paired with walker w of chain k+1, for every w.
 *   draws     one pcg64 engine seeded (seed, 2^64 - 1 - stream), an increment no step stream of the handle has; the pair
 *             (round, slot j, walker w) consumes the one raw output at stream position (r*8 + j)*W + w, whatever K is and
 *             whatever was accepted.  `round` is the caller's: a checkpoint stays get_state plus integers.
 *   decision  in double, whatever the handle's dtype: u = canonical(draw), ln U = log(1 - u),
 *             delta = (logp_k(x_{k+1}) - logp_k(x_k)) + (logp_{k+1}(x_k) - logp_{k+1}(x_{k+1})), accept iff ln U < delta, by
 *             the IEEE comparison alone (a NaN delta rejects, +inf accepts).  logp_k(x_k) and logp_{k+1}(x_{k+1}) are the
 *             stored log-posteriors, the other two are evaluated by the calculator with the other chain's parameters.
 *             A near tie: |ln U - delta| <= 1e-12 (|ln U| + the four |logp|) and the margin finite.
 *   on accept the two rows swap; logp_k[w] <- logp_k(x_{k+1}), logp_{k+1}[w] <- logp_{k+1}(x_k).  n_accept (accepted
 *             stretch proposals of the slot), the step streams and the step count are not touched.
 * proposed/accepted/near_ties: [K-1] counters of pair (k, k+1), overwritten (pairs not in this round: 0).  Any pointer may
 * be NULL.  A round without a pair (K = 2, odd round) succeeds and changes nothing.  Returns when the round is applied.
 * MCMCPP_HIP_E_UNSUPPORTED for the differential-evolution mover, batch targets, sharded handles, handles with a communicator
 * and handles with caller-owned positions; MCMCPP_HIP_E_ARG for num_chains < 2 and round >= 2^40; MCMCPP_HIP_E_STATE before
 * set_state, after a failed run and while an asynchronous run is in progress.  The first round allocates its scratch
 * (16 W log-posteriors) outside the handle's step buffers. */
int mcmcpp_hip_exchange_chains(mcmcpp_hip_sampler* h, uint64_t round, uint64_t* proposed, uint64_t* accepted, uint64_t* near_ties);

/* A tempered run in one call: mcmcpp_hip_run (run_tempered_device: mcmcpp_hip_run_device) of n_saved * interval ensemble
 * steps with a round of mcmcpp_hip_exchange_chains behind every exchange_every-th ensemble step, counted from the start of the
 * run: rounds first_round, first_round + 1, ...  A run that ends on a multiple of exchange_every ends with a round; a shorter
 * tail has none behind it.  exchange_every need not be a multiple of interval.  It computes, bit for bit, what the loop
 * "run exchange_every steps, exchange_chains(round++)" computes -- chain, accepted_per_step, walker state, n_accept, the step
 * streams, every counter -- but the rounds lie inside the run's launch sequence: two launches per round (the cross
 * evaluations of all pairs, then the swaps), no host synchronisation, no copy between the segments.  The stored steps reach
 * chain_out / device_chain by the paths of mcmcpp_hip_run / mcmcpp_hip_run_device, laid out as there; a stored step that is
 * an exchange point holds the state in front of its round, as in the loop.
 *   proposed/accepted/near_ties  [K-1] counters of pair (k, k+1), summed over the rounds of this run, overwritten
 *   rounds_done                  the rounds of this run: n_saved * interval / exchange_every (the next run continues the same
 *                                tempered run with first_round + *rounds_done when this run's length is a multiple of
 *                                exchange_every)
 * Any of the four and accepted_per_step may be NULL.  n_saved == 0 succeeds with zero rounds.  Refusals: those of
 * mcmcpp_hip_run (run_tempered_device: mcmcpp_hip_run_device) and of mcmcpp_hip_exchange_chains with their codes;
 * MCMCPP_HIP_E_ARG for exchange_every < 1 and for first_round + rounds > 2^40; MCMCPP_HIP_E_STATE while an asynchronous run is
 * in progress.  The first tempered run allocates the scratch of a round (16 W log-posteriors) outside the step buffers. */
int mcmcpp_hip_run_tempered(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, int64_t exchange_every, uint64_t first_round,
                            void* chain_out, uint32_t* accepted_per_step, uint64_t* proposed, uint64_t* accepted, uint64_t* near_ties,
                            uint64_t* rounds_done);
int mcmcpp_hip_run_tempered_device(mcmcpp_hip_sampler* h, int64_t n_saved, int32_t interval, int64_t exchange_every,
                                   uint64_t first_round, void* device_chain, uint32_t* accepted_per_step, uint64_t* proposed,
                                   uint64_t* accepted, uint64_t* near_ties, uint64_t* rounds_done);

/* ---- evidence from a ladder: ratios of normalising constants between neighbouring chains ----------------- */

/* A handle has K = num_chains >= 2 rungs (chains with per-chain parameters); Z_k = integral of exp(logp_k) is the normalising
 * constant of rung k's target.  From stored steps of the K chains -- a tempered run's, or any draws of the rungs -- the call
 * estimates log(Z_p / Z_{p+1}) of every pair of neighbours by importance weights, in both directions.  The chain of the
 * ratios is the evidence of rung 0 only when the top rung is a normalised density (its Z is 1, or known).
 *   draws      n used steps per rung (every slice_interval-th of n_steps, from the first on), N = n W draws per rung in the
 *              order i = s W + w.  Pair p is the rungs (a, b) = (p, p + 1), 0 <= p < K - 1.  Direction d = 0, the stepping-stone
 *              direction, takes the draws x_i of rung b (the flatter one): u_i = logp_a(x_i) - logp_b(x_i).  Direction d = 1,
 *              the reverse, takes the draws of rung a: u_i = logp_b(x_i) - logp_a(x_i).  Every output is [2][K - 1], d-major.
 *   logp       the two log-posteriors of a draw are what mcmcpp_hip_calc_logp_device returns for that row with that chain's
 *              parameters, bit for bit, in the handle's dtype, widened to double exactly; u is one double subtraction.
 *   nonfinite  counts the i whose u_i is not finite.  If any u_i is NaN or +inf, then log_ratio, mcse, ess, kish and max_u are
 *              NaN for that (d, p) and for nothing else.  A u_i of -inf (a draw outside the other rung's support) has weight 0.
 *   estimate   m = max u_i (of -0 and +0, +0); e_i = evidence_exp(u_i - m) (mcmcpp_amd/csrc/evidence_exp.hpp: exp with one
 *              value in bits; evidence_exp(0) = 1, evidence_exp(-inf) = 0); S1 = sum_fixed(e), S2 = sum_fixed(e e) over i, with
 *              sum_fixed the shape of mcmcpp_hip_gelman_rubin (slices of rhat_slice_len(N) terms); wbar = S1 / N, a positive
 *              normal number since 1/N <= wbar <= 1; lme = m + normal_score_log(wbar) (normal_score.hpp's logarithm).
 *              log_ratio[0][p] = lme, log_ratio[1][p] = -lme: both estimate log(Z_p / Z_{p+1}).  max_u = m.  If every u_i is
 *              -inf: lme = -inf (log_ratio[1][p] = +inf), and mcse, ess and kish are NaN.
 *   kish       (S1 S1) / S2, Kish's size of the weights.  rel2 = max(S2 / N - wbar wbar, 0) / (wbar wbar).
 *   ess        the `ess` output of mcmcpp_hip_effective_sample_size_device on the weights e seen as a chain of one rung: n
 *              steps, W walkers, one parameter, fp64, split = 1, max_lag = 0 (that call's own body, so its bits): n >= 4.
 *   mcse       0 when rel2 == 0 (constant weights), else sqrt(rel2 / ess): the standard error of lme.
 *   totals     log_ratio_total[d] = the sum of log_ratio[d][.] in ascending p from +0: log(Z_0 / Z_{K-1});
 *              mcse_total[d] = sqrt(the sum of mcse mcse in ascending p from +0).
 * Everything is fp64, every + - * / rounded on its own; no fused operation, no floating-point atomic.  No output depends on
 * the CU count, the chunk size (MCMCPP_HIP_EVIDENCE_CHUNK_MB, read per call, default 1024: host steps are uploaded, and rows
 * evaluated, a chunk at a time) or where a chain lies.
 *   steps         K * n_steps host pointers to steps [W][D] of the handle's dtype, rung k's step s at steps[k * n_steps + s]
 *   device_steps  the chains in memory of the handle's device, laid out as for mcmcpp_hip_gelman_rubin_device: rung k's step s
 *                 at device_steps + (k * chain_stride_steps + s) * W * D elements; chain_stride_steps 0: n_steps.  Read where
 *                 they lie; the rows must satisfy mcmcpp_hip_calc_logp_device's alignment rule.
 *   outputs       log_ratio, mcse, ess, kish, max_u [2][K-1] double; nonfinite [2][K-1] int64; log_ratio_total, mcse_total [2];
 *                 *num_draws = N.  Any may be NULL.  Nothing is written to the outputs of a call that fails.
 * The call reads the calculators only: it needs no set_state, and leaves the walker state, the step streams and every counter
 * as they are.  The weights take 8 N bytes of device memory per (d, p) in flight (two at most), freed when the call returns:
 * MCMCPP_HIP_E_NOMEM with a message where they cannot be had.  Returns MCMCPP_HIP_E_UNSUPPORTED for the differential-evolution
 * mover, batch targets, sharded handles, handles with a communicator and handles with caller-owned positions;
 * MCMCPP_HIP_E_ARG for num_chains < 2, fewer than 4 used steps, slice_interval < 1, 0 < chain_stride_steps < n_steps, NULL steps,
 * a device pointer that is not memory of the handle's device or whose chains end outside its allocation; MCMCPP_HIP_E_STATE
 * while an asynchronous run is in progress. */
int mcmcpp_hip_evidence_ratios(mcmcpp_hip_sampler* h, const void* const* steps, int64_t n_steps, int64_t slice_interval, double* log_ratio,
                               double* mcse, double* ess, double* kish, double* max_u, int64_t* nonfinite, double* log_ratio_total,
                               double* mcse_total, int64_t* num_draws);
int mcmcpp_hip_evidence_ratios_device(mcmcpp_hip_sampler* h, const void* device_steps, int64_t chain_stride_steps, int64_t n_steps,
                                      int64_t slice_interval, double* log_ratio, double* mcse, double* ess, double* kish, double* max_u,
                                      int64_t* nonfinite, double* log_ratio_total, double* mcse_total, int64_t* num_draws);

/* The bridge estimate of the same ratios (Bennett's acceptance ratio; Meng & Wong 1996; Fruehwirth-Schnatter 2004): one estimate
 * of log(Z_p / Z_{p+1}) per pair from the draws of BOTH rungs, where mcmcpp_hip_evidence_ratios gives one per direction.
 *   draws      as for mcmcpp_hip_evidence_ratios: pair p = rungs (a, b) = (p, p + 1), N = n W draws per rung in the order
 *              i = s W + w.  u0_j = logp_a(x_j) - logp_b(x_j) on the draws x_j of b, u1_i = logp_b(y_i) - logp_a(y_i) on the draws
 *              y_i of a: that call's u of d = 0 and d = 1, the same calc_logp_device bits widened to double, one subtraction.
 *   sigma      sigma(x) = 1 / (1 + evidence_exp(-x)) for x >= 0 (-0 included); sigma(x) = e / (1 + e) with e = evidence_exp(x)
 *              for x < 0: evidence_exp is called with arguments <= 0 only, and has one value in bits on host and device.
 *              sigma(-inf) = 0, sigma(+inf) = 1.
 *   sums       h0_j(c) = sigma(u0_j - c), h1_i(c) = sigma(u1_i + c); S_d(c) = sum_tree(h_d), Q_d(c) = sum_tree(h_d (1 - h_d));
 *              g(c) = S_0(c) - S_1(c).  g does not increase with c; the estimate is its root c*.
 *   sum_tree   sum_tree(v, N): tiles of 1024 consecutive terms; the missing terms of the last tile are +0.  In a tile, lane t of
 *              256 forms ((v[2t] + v[2t+1]) + v[2t+512]) + v[2t+513]; then for s = 128, 64, ..., 1: p_t = p_t + p_{t+s} for t < s;
 *              the tile's sum is p_0.  Tile sums are added in ascending order from +0 within a slice of 64 tiles (the last slice
 *              may be short); slice sums are added in ascending order from +0.  The shape is a function of N alone; its longest
 *              chain of dependent additions is 11 in a tile, 64 in a slice and ceil(N / 65536) over the slices.
 *   solver     A pass evaluates S_0, S_1, Q_0, Q_1 at one c; `passes` counts the passes.
 *              1. c = +0; a pass.  If g == 0: stop.
 *              2. up = g > 0 (the root lies above); step = 1.  Repeat: prev = c; c = prev + step if up, else prev - step, and
 *                 +-DBL_MAX where that is infinite; step = step + step; a pass.  If g == 0: stop.  If (g > 0) != up: lo = the
 *                 smaller and hi = the larger of prev and c, go to 3.  If 1100 passes are done: stop with converged = 0.
 *              3. Repeat, 200 times at the most: mid = 0.5 lo + 0.5 hi.  If S_0 > 0 and S_1 > 0 at c:
 *                 f = normal_score_log(S_0) - normal_score_log(S_1) (normal_score.hpp's logarithm), f' = -(Q_0 / S_0 + Q_1 / S_1),
 *                 and next = c - f / f' unless f' == 0: a Newton step on ln S_0 - ln S_1, which has the root of g and is linear in
 *                 c where the rungs barely overlap.  In every other case, and if not lo < next < hi: next = mid.  If next == lo or
 *                 next == hi: stop.  If |next - c| <= 2^-40 max(1, |next|): c = next, stop.  Otherwise c = next; a pass; if
 *                 g == 0: stop; if g > 0: lo = c, else hi = c.  Behind the 200th such pass: stop with converged = 0.
 *              4. Every stop but the two named has converged = 1.  The final pass is at the c of the stop, c*: it gives the S_d of
 *                 the outputs, forms H_d = sum_tree(h_d h_d) and keeps h_d(c*).  It is counted: passes <= 1301.
 *              The result is a function of the two u arrays alone.
 *   outputs    log_ratio [K-1] = c*.  overlap [K-1] = (S_0 + S_1) / N at c*: 1 for identical rungs, towards 0 for disjoint ones.
 *              passes, converged [K-1] int64.  ess [2][K-1], d-major: the `ess` output of
 *              mcmcpp_hip_effective_sample_size_device on h_d(c*) seen as a chain of one rung: n steps, W walkers, one parameter,
 *              fp64, split = 1, max_lag = 0, as mcmcpp_hip_evidence_ratios calls it on its weights.  mean_d = S_d / N;
 *              rel2_d = max(H_d / N - mean_d mean_d, 0) / (mean_d mean_d); t_d = 0 when rel2_d == 0, else rel2_d / ess_d;
 *              mcse [K-1] = sqrt(t_0 + t_1): the delta-method error of Fruehwirth-Schnatter 2004 with the autocorrelation in the
 *              ESS.  nonfinite [2][K-1] int64 as for mcmcpp_hip_evidence_ratios.  *log_ratio_total = the sum of log_ratio in
 *              ascending p from +0; *mcse_total = sqrt(the sum of mcse mcse in ascending p from +0).  *num_draws = N.
 *   edges      A NaN or +inf among the u of either direction: log_ratio, overlap, mcse and both ess of that pair are NaN, passes
 *              and converged 0, and nothing else changes.  A u of -inf has h = 0.  S_0 == 0 or S_1 == 0 at c* (no mass is
 *              shared at double precision): log_ratio, mcse and ess are NaN and overlap is 0.
 * Everything is fp64, every + - * / rounded on its own; no fused operation, no floating-point atomic.  No output depends on the
 * CU count, the chunk size (MCMCPP_HIP_EVIDENCE_CHUNK_MB, as above) or where a chain lies.  steps, device_steps,
 * chain_stride_steps, n_steps and slice_interval are those of mcmcpp_hip_evidence_ratios, and so are the refusals and argument
 * checks with their codes.  Any output may be NULL; nothing is written to the outputs of a call that fails.  The raw u take
 * 8 N bytes of device memory per pair and direction in flight, three at most and two for K = 2, freed when the call returns:
 * MCMCPP_HIP_E_NOMEM with the byte count where they cannot be had.  The walker state is neither needed nor touched. */
int mcmcpp_hip_evidence_bridge(mcmcpp_hip_sampler* h, const void* const* steps, int64_t n_steps, int64_t slice_interval, double* log_ratio,
                               double* mcse, double* overlap, double* ess, int64_t* passes, int64_t* converged, int64_t* nonfinite,
                               double* log_ratio_total, double* mcse_total, int64_t* num_draws);
int mcmcpp_hip_evidence_bridge_device(mcmcpp_hip_sampler* h, const void* device_steps, int64_t chain_stride_steps, int64_t n_steps,
                                      int64_t slice_interval, double* log_ratio, double* mcse, double* overlap, double* ess, int64_t* passes,
                                      int64_t* converged, int64_t* nonfinite, double* log_ratio_total, double* mcse_total, int64_t* num_draws);

/* All K log-normalising constants of the ladder at once (the multistate Bennett acceptance ratio, MBAR: Shirts & Chodera 2008;
 * Tan 2004's extended bridge; Geyer's reverse logistic regression): one joint solve from every draw of every rung, each
 * evaluated under every rung's parameters, with the K x K covariance of the estimates -- where mcmcpp_hip_evidence_bridge gives
 * one estimate per pair of neighbours and an error that takes the pairs for independent.
 *   draws      as for mcmcpp_hip_evidence_ratios: n used steps per rung, N = n W draws per rung in the order i = s W + w, K
 *              rungs.  Draw i of rung r has the index j = r N + i among all K N draws.
 *   l          l[k][j] is the log-posterior of draw j under chain k's parameters: what mcmcpp_hip_calc_logp_device returns for
 *              that row with that chain's parameters, bit for bit, in the handle's dtype, widened to double exactly.  K K N
 *              evaluations, kept as K arrays of K N doubles.  nonfinite [K][K] int64: [r][k] counts the draws of rung r whose
 *              l[k] is not finite.
 *   weights    zeta is a K-vector with zeta_{K-1} = +0 held fixed.  For draw j: a_k = l[k][j] - zeta_k; m = a_0, then for
 *              k = 1 .. K - 1: m = a_k if a_k > m; e_k = evidence_exp(a_k - m) (mcmcpp_amd/csrc/evidence_exp.hpp; arguments
 *              <= 0 only); Dn = ((+0 + e_0) + e_1) + ... in ascending k; w_k(j) = e_k / Dn.  A draw whose K entries are all -inf
 *              (m = -inf) has every w_k = +0.
 *   sums       S_k = sum_tree(w_k, K N) and P_kl = sum_tree(w_k w_l, K N) for k <= l (P_lk = P_kl): mcmcpp_hip_evidence_bridge's
 *              sum_tree over the K N terms in the order of j; every product and every sum rounded on its own.
 *   equations  G_k(zeta) = S_k - N = 0 for k < K - 1.  A_kk = S_k - P_kk and A_kl = -P_kl (k != l), on the reduced indices
 *              0 .. K - 2: symmetric and positive semi-definite; -A is the Jacobian of G.
 *   solve      solve(A, b), the reduced system A x = b of order M = K - 1, in this order.  Factor, for i = 0 .. M - 1: for
 *              j = 0 .. i - 1: t = A_ij, then t = t - L_ik L_jk for k = 0 .. j - 1 ascending, L_ij = t / L_jj; then d = A_ii, then
 *              d = d - L_ik L_ik for k = 0 .. i - 1 ascending; unless d > 0 the factor fails (below); L_ii = sqrt(d).  Forward,
 *              for i = 0 .. M - 1: t = b_i, t = t - L_ik y_k for k = 0 .. i - 1 ascending, y_i = t / L_ii.  Backward, for
 *              i = M - 1 .. 0: t = y_i, t = t - L_ki x_k for k = i + 1 .. M - 1 ascending, x_i = t / L_ii.
 *   solver     A pass evaluates every S_k and P_kl at one zeta; `passes` counts the passes.  zeta = +0.  Repeat, 200 times at
 *              the most: a pass; delta = solve(A, G); mx = max_k |delta_k|; if mx > 4: delta_k = delta_k (4 / mx) (one
 *              division, then one product each) and mx = max_k |delta_k| anew; zeta_k = zeta_k + delta_k for k < K - 1; if
 *              mx <= 2^-40 max(1, max_k |zeta_k|): stop with converged = 1.  Behind the 200th such pass: converged = 0.  The
 *              final pass is at the zeta of the stop; it is counted: passes <= 201.  The result is a function of l alone.
 *   errors     The final pass gives S and P at the stopped zeta, hence A and its factor, and forms per rung r, over that rung's N
 *              terms alone (a tree of its own that begins at j = r N): M_rk = sum_tree(w_k, N), P^r_kl = sum_tree(w_k w_l, N)
 *              (k <= l), C^r_kl = P^r_kl / N - (M_rk / N) (M_rl / N) (not clamped; C^r_lk = C^r_kl).  ess [K]: ess[r] is the
 *              `ess` output of mcmcpp_hip_effective_sample_size_device on the series w_r(r N + i), i = 0 .. N - 1, seen as a chain
 *              of one rung: n steps, W walkers, one parameter, fp64, split = 1, max_lag = 0, as the other two evidence calls use
 *              it.  f_r = (N N) / ess[r].  V_kl = the sum in ascending r from +0 of f_r C^r_kl, where a C^r_kl that is zero
 *              contributes +0 whatever f_r is (the series of identical rungs is constant and has no ESS).  With Y = the matrix
 *              whose column c is solve(A, column c of V): row c of cov is solve(A, row c of Y), on the reduced indices: the
 *              sandwich A^-1 V A^-T of the estimating equations with each rung's autocorrelation in its ESS.  Row and column
 *              K - 1 of cov are +0.  It is not the delta-method mcse of mcmcpp_hip_evidence_bridge, also not for K = 2.
 *   outputs    log_z [K] = zeta: log(Z_k / Z_{K-1}).  cov [K][K].  log_ratio [K-1]: zeta_p - zeta_{p+1}, the estimate of
 *              log(Z_p / Z_{p+1}).  mcse [K-1]: v = (cov_pp + cov_qq) - 2 cov_pq with q = p + 1; sqrt(v), and 0 where v < 0.
 *              ess [K].  nonfinite [K][K] int64.  *log_ratio_total = zeta_0; *mcse_total = sqrt(cov_00), and 0 where
 *              cov_00 < 0.  *passes, *converged int64.  *num_draws = N.
 *   edges      A NaN or +inf anywhere in l: every floating output is NaN, passes = converged = 0 (the solve is joint: nothing can
 *              be spared); nonfinite stands.  An l of -inf has weight 0 and is counted.  A factor that fails in the solver or
 *              behind the final pass (a pivot that is not positive: no mass is shared at double precision): every floating
 *              output is NaN and converged = 1; passes counts the passes made.  Identical rungs: zeta = +0, mcse = 0, passes = 2.
 * Everything is fp64, every + - * / rounded on its own; no fused operation, no floating-point atomic.  No output depends on the
 * CU count, the chunk size (MCMCPP_HIP_EVIDENCE_CHUNK_MB, as above: host steps are uploaded, and rows evaluated, a chunk at a
 * time) or where a chain lies.  steps, device_steps, chain_stride_steps, n_steps and slice_interval are those of
 * mcmcpp_hip_evidence_ratios, and so are the refusals and argument checks with their codes.  Any output may be NULL; nothing is
 * written to the outputs of a call that fails.  l takes 8 K K N bytes of device memory, freed when the call returns:
 * MCMCPP_HIP_E_NOMEM with the byte count where they cannot be had.  The walker state is neither needed nor touched. */
int mcmcpp_hip_evidence_mbar(mcmcpp_hip_sampler* h, const void* const* steps, int64_t n_steps, int64_t slice_interval, double* log_z, double* cov,
                             double* log_ratio, double* mcse, double* ess, int64_t* nonfinite, double* log_ratio_total, double* mcse_total,
                             int64_t* passes, int64_t* converged, int64_t* num_draws);
int mcmcpp_hip_evidence_mbar_device(mcmcpp_hip_sampler* h, const void* device_steps, int64_t chain_stride_steps, int64_t n_steps,
                                    int64_t slice_interval, double* log_z, double* cov, double* log_ratio, double* mcse, double* ess,
                                    int64_t* nonfinite, double* log_ratio_total, double* mcse_total, int64_t* passes, int64_t* converged,
                                    int64_t* num_draws);

/* The evidence of ONE chain's target from an ordinary run: the bridge between the target and a Gaussian q = N(mean, L L^T)
 * fitted to its draws (Overstall & Forster 2010; Gronau et al. 2017).  q is normalised, so the bridge's log-ratio is
 * log Z = log of the integral of exp(logp) itself.  No ladder is needed: num_chains may be 0 or 1.
 *   draws      every slice_interval-th of the n_steps steps [W][D] of one chain, from the first on: n used steps, N = n W draws y_i
 *              in the order i = s W + w.  `chain` selects the parameters, 0 <= chain < max(num_chains, 1).  Which part of a run
 *              the steps are is the caller's choice: a Gaussian fitted to one part is bridged with the draws of another.
 *   Gaussian   mean [D] and chol [D * D], row-major, the lower triangle L of which alone is read; double whatever the handle's
 *              dtype.  MCMCPP_HIP_E_ARG for an entry that is read and is not finite, and for a diagonal entry that is not a
 *              positive normal number.  MCMCPP_HIP_E_UNSUPPORTED for D > 64.
 *   proposals  as many as draws.  Proposal j = 0 .. N - 1, coordinate d, takes the raw output r at position j D + d of the pcg64
 *              engine seeded (seed, stream) as the samplers seed theirs: the caller's seed and stream, not the handle's -- no
 *              stream of the handle is touched.  p = ((r >> 12) + 0.5) 2^-52, both operations exact; z_d = normal_score(p)
 *              (mcmcpp_amd/csrc/normal_score.hpp).  x_i = mean_i + acc_i, where acc_i starts at +0 and takes + L[i][d] z[d] for
 *              d = 0 .. i in ascending order, every product and every sum rounded on its own; x_i is then rounded once to the
 *              handle's dtype.  The proposals are seen as n steps of W walkers in the same order j = s W + w.
 *   log q      for a row x of the handle's dtype, widened exactly to double: z_i = ((x_i - mean_i) - t_i) / L[i][i] for
 *              i = 0 .. D - 1, where t_i starts at +0 and takes + L[i][d] z[d] for d < i in ascending order; s starts at +0 and
 *              takes + z_i z_i in ascending i; log q(x) = (-0.5 s) + k with k = -(the sum from +0, in ascending i, of
 *              normal_score_log(L[i][i])) - D 0.91893853320467274178.  The rounded proposals and the draws go through the same
 *              evaluation.
 *   u          u0_j = logp(x_j) - log q(x_j) on the proposals, u1_i = log q(y_i) - logp(y_i) on the draws; logp is what
 *              mcmcpp_hip_calc_logp_device returns for that row with that chain's parameters, widened to double exactly; one
 *              subtraction each.  In the bridge's words the pair is (a, b) = (target, q).
 *   estimate   From here on the definition is mcmcpp_hip_evidence_bridge's, word for word, on these two arrays: sigma, sum_tree, the
 *              solver, the edges (a NaN or +inf u; no shared mass; a u of -inf has h = 0), mcse from both ESS calls, overlap,
 *              passes, converged, nonfinite [2].  *log_evidence = c*.
 *   outputs    *log_evidence, *mcse, *overlap double; ess [2] double; *passes, *converged int64; nonfinite [2] int64 (index 0:
 *              the proposals, 1: the draws); *num_draws = N; proposals [N][D] of the handle's dtype: the rows as the calculator
 *              saw them; log_q [2][N] double: row 0 of the proposals, row 1 of the draws.  Any may be NULL.  Nothing is written
 *              to the outputs of a call that fails.
 * Everything is fp64, every + - * / rounded on its own; no fused operation, no floating-point atomic.  No output depends on the
 * CU count, the chunk size (MCMCPP_HIP_EVIDENCE_CHUNK_MB, as above: steps are uploaded, and proposals made and evaluated, a chunk
 * at a time) or where the chain lies.  The call is a function of its arguments: it needs no set_state and leaves the walker
 * state, the step streams and every counter as they are.  It holds 8 N bytes of device memory per u (two), and the proposals
 * of a chunk, freed when it returns: MCMCPP_HIP_E_NOMEM with the byte count where they cannot be had.
 *   steps         n_steps host pointers to steps [W][D] of the handle's dtype
 *   device_steps  the chain in memory of the handle's device, step s at device_steps + s * W * D elements; read where it lies;
 *                 the rows must satisfy mcmcpp_hip_calc_logp_device's alignment rule
 * Every handle mcmcpp_hip_calc_logp_device serves is served: stretch-move handles of one or more chains,
 * differential-evolution handles (chain 0) and batch targets (chain 0; the callback is called on the proposals where they were
 * made, in a buffer that is 16-byte aligned).  Refusals: those of mcmcpp_hip_calc_logp_device with their codes, and
 * MCMCPP_HIP_E_UNSUPPORTED for sharded handles, handles with a communicator and handles with caller-owned positions;
 * MCMCPP_HIP_E_ARG for fewer than 4 used steps, slice_interval < 1, NULL steps, mean or chol, a chain out of range, a device
 * pointer that is not memory of the handle's device or whose steps end outside its allocation; MCMCPP_HIP_E_STATE while an
 * asynchronous run is in progress. */
int mcmcpp_hip_evidence_gaussian(mcmcpp_hip_sampler* h, int32_t chain, const void* const* steps, int64_t n_steps, int64_t slice_interval,
                                 const double* mean, const double* chol, uint64_t seed, uint64_t stream, double* log_evidence, double* mcse,
                                 double* overlap, double* ess, int64_t* passes, int64_t* converged, int64_t* nonfinite, int64_t* num_draws,
                                 void* proposals, double* log_q);
int mcmcpp_hip_evidence_gaussian_device(mcmcpp_hip_sampler* h, int32_t chain, const void* device_steps, int64_t n_steps,
                                        int64_t slice_interval, const double* mean, const double* chol, uint64_t seed, uint64_t stream,
                                        double* log_evidence, double* mcse, double* overlap, double* ess, int64_t* passes, int64_t* converged,
                                        int64_t* nonfinite, int64_t* num_draws, void* proposals, double* log_q);
/* GPU time of the calling thread's last successful mcmcpp_hip_evidence_gaussian / _device call in its two own kernels, between HIP
 * events recorded around every launch on the call's stream and summed over the chunks: the kernel that makes the proposals
 * and the kernel that evaluates log q (on the proposals and on the draws).  Either pointer may be NULL. */
void mcmcpp_hip_evidence_gaussian_last_timing(double* rows_ms, double* log_q_ms);

/* ---- measurement ---------------------------------------------------------------------------------- */

/* GPU time of the last mcmcpp_hip_run between HIP events recorded on the launch stream around the
 * step launches (excludes uploads / downloads), and the number of step-kernel launches it covers: one per
 * ensemble step for ensembles small enough to be stepped by the full-step kernel, two (red, black) otherwise, four
 * (propose and accept of each colour) for a batch target, whose time includes the callback's device work. */
int mcmcpp_hip_last_run_timing(mcmcpp_hip_sampler* h, double* gpu_ms, int64_t* step_launches);

/* Host-side cost of the last mcmcpp_hip_run: the time the calling thread spent enqueueing the step launches (and, for a
 * split ensemble, the exchanges), the wall time of the whole call, and -- split ensembles only -- the GPU time of one
 * ensemble step's exchange, averaged over a sample of steps bracketed by HIP events (0 when none was sampled).
 * Any pointer may be NULL. */
int mcmcpp_hip_last_run_host_timing(mcmcpp_hip_sampler* h, double* enqueue_ms, double* wall_ms, double* exchange_us_per_step);

/* Split ensembles: what the exchanges of the last mcmcpp_hip_run moved.  Ranks of a communicator of more than one rank
 * exchange only the rows that moved (index, log-posterior, row, packed into blocks of `block_slots` walkers per rank and
 * all-gathered once per ensemble step -- once per half-step for slices too large for the one-launch-per-step kernels);
 * the bound is learned from the run, and a chunk of steps in which some rank moved more walkers than a block holds is
 * REPEATED from a snapshot with blocks that hold a whole slice, so the chain never depends on the bound.
 *   bytes_per_step   bytes this rank received per ensemble step (all-gathering whole slices: (G-1)/G of the ensemble)
 *   repeated_chunks  chunks of steps that were rolled back and repeated
 *   block_slots      walkers per block at the end of the run (0: whole slices were all-gathered)
 * Any pointer may be NULL. */
int mcmcpp_hip_last_run_exchange(mcmcpp_hip_sampler* h, double* bytes_per_step, int64_t* repeated_chunks, int64_t* block_slots);

/* ---- multi-GPU single ensemble (one handle per GPU) -------------------------------- */

/* (A handle with a communicator needs none of these: mcmcpp_hip_run drives the split ensemble itself.  They remain for
 * callers that bring their own exchange.)
 * Enqueue ONE half-step (color 0 = red, 1 = black) for this handle's shard on its stream and return
 * without waiting.  The caller then exchanges the updated rows (device_positions + offset, see
 * mcmcpp_hip_shard_span) with the other handles -- e.g. an in-place RCCL all-gather on the same
 * stream -- before enqueueing the next half-step.  save_slot >= 0 also writes the shard's rows of
 * that stored step into the device chain buffer given to mcmcpp_hip_bind_device_chain. */
int mcmcpp_hip_half_step_async(mcmcpp_hip_sampler* h, int32_t color, int64_t save_slot);
int mcmcpp_hip_bind_device_chain(mcmcpp_hip_sampler* h, void* device_chain, int64_t slots);
/* device pointer of the ensemble positions (W*D elements) and the element span [offset, offset+count)
 * this handle rewrites during a half-step of `color` */
void* mcmcpp_hip_device_positions(mcmcpp_hip_sampler* h);
int mcmcpp_hip_shard_span(mcmcpp_hip_sampler* h, int32_t color, int64_t* offset_elems, int64_t* count_elems);
int mcmcpp_hip_synchronize(mcmcpp_hip_sampler* h);

/* ---- chain analysis on the device -------------------------------------------- */

/* Analysis::CovarianceMatrix (reference MCMCpp/Analysis/CovarianceMatrix.h:154-257): mean, covariance and
 * correlation matrix of stored chain steps.  The sums  s_i = sum x_i,  S_ij = sum x_i x_j  over all samples are a
 * rank-N update X^T X and run on the matrix cores (fp64 accumulation for both element types); the slicing the
 * reference's calculateCovar(start, end, sliceInterval) does while iterating is expressed by step_stride.
 *   create      dtype MCMCPP_HIP_F64 / _F32 = the chain's ParamType; device -1 = current; 1 <= num_params <= 1024.
 *               MCMCPP_HIP_MOMENTS_CHUNK_MB (read here, default 64) sizes the chunks add_steps uploads host steps in
 *               (a chunk holds at least one step)
 *   add_steps   n_steps stored steps of num_walkers*num_params elements each (host memory), consecutive ones
 *               step_stride steps apart; may be called repeatedly (chain blocks, several chains)
 *   finish      CovarianceMatrix::finalizeMatrix: mean[D], cov[D*D], corr[D*D] in the chain's element type (any may
 *               be NULL); *num_points = samples used.  The accumulator keeps its sums: more steps may follow.
 * The reference's sequential Kahan sums cannot be kept by a parallel sum: results agree with it to rounding
 * (tests/test_moments.py states the tolerance), not bit for bit. */
typedef struct mcmcpp_hip_moments mcmcpp_hip_moments;
int mcmcpp_hip_moments_create(int32_t dtype, int32_t device, int32_t num_walkers, int32_t num_params, mcmcpp_hip_moments** out);
void mcmcpp_hip_moments_destroy(mcmcpp_hip_moments* m);
int mcmcpp_hip_moments_reset(mcmcpp_hip_moments* m);
int mcmcpp_hip_moments_add_steps(mcmcpp_hip_moments* m, const void* steps, int64_t n_steps, int64_t step_stride);
/* the same for n_steps contiguous stored steps that already live in device memory (e.g. a chain written by
 * mcmcpp_hip_run_device, or a device chain bound with mcmcpp_hip_bind_device_chain): no upload; returns when the sums are
 * updated */
int mcmcpp_hip_moments_add_device_steps(mcmcpp_hip_moments* m, const void* device_steps, int64_t n_steps);
/* ... and with the slicing of add_steps: n_steps stored steps, consecutive ones step_stride steps apart in device memory
 * (stride 1 is add_device_steps).  The steps used are gathered on the device into the accumulator's chunk buffer, in the
 * chunks add_steps uploads: the sums are grouped as add_steps groups them. */
int mcmcpp_hip_moments_add_device_steps_strided(mcmcpp_hip_moments* m, const void* device_steps, int64_t n_steps, int64_t step_stride);
int mcmcpp_hip_moments_finish(mcmcpp_hip_moments* m, int64_t* num_points, void* mean, void* cov, void* corr);
const char* mcmcpp_hip_moments_last_error(const mcmcpp_hip_moments* m);

/* Analysis::AutoCorrCalc::calcAutoCorrTimes (reference MCMCpp/Analysis/AutoCorrCalc.h:151-207, with
 * Analysis/Detail/AutoCov.h:146-322): the integrated autocorrelation time of every parameter.  Per (walker, parameter)
 * series: Kahan average, circular autocovariance by two radix-2 FFTs over the next power of two >= n_steps, divided by
 * lag 0; per parameter: the walkers' functions Kahan-summed and divided by their number, then the windowed sum
 * (window_scaling = the reference's setAutoCorrScaleFactor value, default 4).  One workgroup per series, transforms in LDS.
 *   steps          n_steps pointers to stored steps of num_walkers*num_params elements (host memory), oldest first
 *   walkers_to_use 0 = all; otherwise that many walkers, evenly spaced over the ensemble (the reference draws a
 *                  subset seeded from std::random_device, i.e. irreproducibly)
 *   times          [num_params]: the time, or minus the final sum where the window never closed (as the reference)
 *   functions      NULL, or [num_params][n_steps]: the averaged autocovariance functions
 * Every operation is the reference's own expression in the reference's order (twiddle factors from the host's libm):
 * results are bit-identical to the oracle's restatement, which is pinned bit for bit to the reference's AutoCov.  Not
 * reproduced: the reference's transferWalker ADDS each series onto what its scratch array holds (the previous
 * walker's function; uninitialised memory for the first), see INTEGRATION.md 4b. */
int mcmcpp_hip_autocorr_times(int32_t dtype, int32_t device, const void* const* steps, int64_t n_steps, int32_t num_walkers, int32_t num_params,
                              int32_t walkers_to_use, int32_t window_scaling, void* times, void* functions);
/* the same for a chain that already lives in device memory: n_steps contiguous stored steps ([n_steps][W][D], e.g. a chain
 * written by mcmcpp_hip_run_device, or a device chain bound with mcmcpp_hip_bind_device_chain); no upload */
int mcmcpp_hip_autocorr_times_device(int32_t dtype, int32_t device, const void* device_steps, int64_t n_steps, int32_t num_walkers,
                                     int32_t num_params, int32_t walkers_to_use, int32_t window_scaling, void* times, void* functions);
const char* mcmcpp_hip_autocorr_last_error(void);

/* Analysis::CornerHistograms and Analysis::PercentileAndMaximumFinder (reference MCMCpp/Analysis/CornerHistograms.h,
 * PercentileAndMaximumFinder.h): the 1-D histogram of every parameter and, with with_pairs, the 2-D histogram of every
 * parameter pair, over the selected stored steps.  Binning is the reference's, in the chain's element type: per parameter
 * the minimum and maximum of the samples used (start values numeric_limits<T>::max() / ::min(), strict comparisons), the
 * reference's tweak of the two bounds, width = (hi - lo) / bins, bin = int((x - lo) / width).  Every sample the reference
 * bins in range lands in the reference's bin.  A bin outside [0, bins) (the reference writes outside its arrays there) is
 * clamped into bin 0 or bins - 1 and counted in `clamped`.  Counts are 64-bit integer sums: bit-reproducible.
 *   create          dtype MCMCPP_HIP_F64 / _F32 = the chain's ParamType; device -1 = current; bins >= 2;
 *                   1 <= num_params <= 65535.  MCMCPP_HIP_E_NOMEM (with a message) when the 64-bit result arrays cannot be
 *                   allocated.  MCMCPP_HIP_HIST_CHUNK_MB (read here, default 1024) sizes the chunks host chains are
 *                   uploaded in.
 *   compute         n_steps pointers to the steps to use (host memory, the caller has applied sliceInterval); steps that
 *                   are contiguous in memory are uploaded in one copy.  Replaces the previous result.  A NaN sample fails
 *                   the call with MCMCPP_HIP_E_ARG; the handle stays usable.
 *   compute_device  n_steps contiguous steps [n][W][P] in device memory (e.g. a chain written by mcmcpp_hip_run_device, or a
 *                   device chain bound with mcmcpp_hip_bind_device_chain); every slice_interval-th from the first is used;
 *                   no upload.
 *   result          bounds [P][2] = (low edge, bin width) in T, as the reference's paramBounds after findBinning;
 *                   single [P][bins]; pairs [P(P-1)/2][bins][bins] (pair i > j at i(i-1)/2 + j, element [bin_i][bin_j]) or
 *                   NULL; clamped [P]; *num_points = samples used.  Any pointer may be NULL. */
typedef struct mcmcpp_hip_histograms mcmcpp_hip_histograms;
int mcmcpp_hip_histograms_create(int32_t dtype, int32_t device, int32_t num_walkers, int32_t num_params, int32_t bins,
                                 int32_t with_pairs, mcmcpp_hip_histograms** out);
void mcmcpp_hip_histograms_destroy(mcmcpp_hip_histograms* h);
int mcmcpp_hip_histograms_compute(mcmcpp_hip_histograms* h, const void* const* steps, int64_t n_steps);
int mcmcpp_hip_histograms_compute_device(mcmcpp_hip_histograms* h, const void* device_steps, int64_t n_steps,
                                         int64_t slice_interval);
int mcmcpp_hip_histograms_result(const mcmcpp_hip_histograms* h, int64_t* num_points, void* bounds, int64_t* single,
                                 int64_t* pairs, int64_t* clamped);
const char* mcmcpp_hip_histograms_last_error(const mcmcpp_hip_histograms* h);

/* Exact order statistics and exact ranks of the parameters over stored steps (an extension: the reference has only the
 * binned PercentileAndMaximumFinder above).  N = (steps used) x num_walkers samples per parameter.
 *   order_statistics  values[p][k] (T, [num_params][n_ranks]) = the sample of parameter p that n_ranks[k] samples of p
 *                     precede in the total order -inf < ... < -0 < +0 < ... < +inf: its bits are those of a sample in
 *                     the data.  ranks[n_ranks]: 0 <= rank < N, the same for every parameter, in any order, repeats
 *                     allowed; 1 <= n_ranks <= 64; 1 <= num_params <= 1024.  Found by most-significant-digit radix
 *                     selection on order-preserving integer keys: integer counts only, so the result does not depend on
 *                     scheduling, slicing or chunking.
 *   rank_counts       below[p][q] / not_above[p][q] (int64, [num_params][n_query]; either may be NULL) = the number of
 *                     samples x of parameter p with x < query[p][q] / x <= query[p][q], compared as numbers (-0 == +0).
 *                     query is [num_params][n_query] in T; n_query >= 1.
 *   steps             n_steps pointers to the steps to use (host memory, the caller has applied its slicing), uploaded in
 *                     chunks of MCMCPP_HIP_QUANTILE_CHUNK_MB (read per call, default 1024): once when they fit one chunk,
 *                     once per pass otherwise.
 *   device_steps      n_steps contiguous steps [n_steps][W][P] in memory of the device, read where they lie; every
 *                     slice_interval-th from the first is used.
 * Free functions with a thread-local last error.  MCMCPP_HIP_E_ARG (with a message), before the device is opened, for a bad
 * dtype, num_params, num_walkers, n_ranks or n_query, a NULL array, slice_interval < 1, N == 0, a rank outside [0, N) and a
 * NaN query; and for a NaN sample, a device_steps that is not memory of that device, or steps that do not end inside its
 * allocation.  Nothing is written to the outputs of a call that fails. */
int mcmcpp_hip_order_statistics(int32_t dtype, int32_t device, const void* const* steps, int64_t n_steps, int32_t num_walkers,
                                int32_t num_params, const int64_t* ranks, int32_t n_ranks, void* values);
int mcmcpp_hip_order_statistics_device(int32_t dtype, int32_t device, const void* device_steps, int64_t n_steps,
                                       int64_t slice_interval, int32_t num_walkers, int32_t num_params, const int64_t* ranks,
                                       int32_t n_ranks, void* values);
int mcmcpp_hip_rank_counts(int32_t dtype, int32_t device, const void* const* steps, int64_t n_steps, int32_t num_walkers,
                           int32_t num_params, const void* query, int32_t n_query, int64_t* below, int64_t* not_above);
int mcmcpp_hip_rank_counts_device(int32_t dtype, int32_t device, const void* device_steps, int64_t n_steps, int64_t slice_interval,
                                  int32_t num_walkers, int32_t num_params, const void* query, int32_t n_query, int64_t* below,
                                  int64_t* not_above);
const char* mcmcpp_hip_order_statistics_last_error(void);

/* The Gelman-Rubin potential scale reduction (split R-hat, BDA3 form) of every parameter, with the walkers of num_chains
 * independent chains as sequences (an extension: the reference has no such class).  Chains of one handle (num_chains, chain k
 * seeded seed + k) or of several handles: have they converged to the same distribution?
 *   input           K = num_chains chains of n used steps of W walkers x P parameters in T; all arithmetic and all outputs
 *                   are double (a float sample converts exactly), every + - x / rounded on its own.
 *   sequences       with split != 0 every walker gives two sequences of L = floor(n / 2) steps: used steps [0, L) and
 *                   [n - L, n) (for odd n the middle step is dropped); without, one of L = n.  H = 2 or 1; M = K H W
 *                   sequences, sequence m = (k H + h) W + w.  L >= 2 and M >= 2.
 *   sum_fixed       the one shape of every sum below, so that a result is a function of the data alone (not of scheduling,
 *                   CU count, chunk size, or where the chain lies): v[0..N) is cut into consecutive slices of
 *                   slice_len(N) = max(1024, ceil(N / 64) rounded up to a multiple of 64) terms (the last may be short; at
 *                   most 64 slices); a slice is summed in ascending order from +0; the slice sums are added in ascending
 *                   order.  No floating-point atomics.
 *   per sequence    c = its first sample, d_s = x_s - c; S1 = sum_fixed(d), S2 = sum_fixed(d d) over its L steps;
 *                   q = S1 / L; sequence_mean[m][p] = c + q; sequence_m2[m][p] = max(S2 - S1 q, 0).
 *   per parameter   v_m = sequence_m2 / (L - 1); within = sum_fixed(v_m) / M; mean = sum_fixed(sequence_mean) / M;
 *                   e_m = sequence_mean - mean; between = sum_fixed(e_m e_m) / (M - 1) (B / L in BDA3's notation);
 *                   varplus = (within (L - 1)) / L + between; rhat = sqrt(varplus / within).
 *   per chain       chain_mean[k][p] = sum_fixed of sequence_mean over the chain's H W sequences in m order, over H W;
 *                   chain_within[k][p] the same of v_m: they tell which ensemble disagrees.
 *   non-finite      samples propagate by IEEE rules; a constant parameter has within = 0 and rhat = NaN.
 *   steps           num_chains x n_steps host pointers, chain k's step s at steps[k n_steps + s] (the caller has applied
 *                   its slicing), uploaded chain by chain in chunks of MCMCPP_HIP_RHAT_CHUNK_MB (read per call, default
 *                   1024); the chunks do not change a bit of the result.
 *   device_steps    chain k starts k x chain_stride_steps steps behind the pointer (0: n_steps; else >= n_steps, e.g. to
 *                   skip a burn-in by offsetting the pointer into the [K][n_saved][W][P] array run_device wrote); of each
 *                   chain's n_steps steps every slice_interval-th from the first is used; read where they lie.
 *   outputs         rhat, mean, within, between [P]; chain_mean, chain_within [K][P]; sequence_mean, sequence_m2 [M][P];
 *                   *sequence_length = L, *num_sequences = M.  Any of them may be NULL.
 * Free functions with a thread-local last error.  MCMCPP_HIP_E_ARG (with a message), before the device is opened, for a bad
 * dtype, num_chains or num_params outside 1..1024, num_walkers < 1, W P >= 2^31, slice_interval < 1, a chain_stride_steps
 * below n_steps, a NULL array or step pointer, L < 2 and M < 2; and for a device_steps that is not memory of that device, or
 * chains that do not all end inside its allocation.  Nothing is written to the outputs of a call that fails. */
int mcmcpp_hip_gelman_rubin(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps,
                            int32_t num_walkers, int32_t num_params, int32_t split, double* rhat, double* mean, double* within,
                            double* between, double* chain_mean, double* chain_within, double* sequence_mean,
                            double* sequence_m2, int64_t* sequence_length, int64_t* num_sequences);
int mcmcpp_hip_gelman_rubin_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains,
                                   int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval, int32_t num_walkers,
                                   int32_t num_params, int32_t split, double* rhat, double* mean, double* within, double* between,
                                   double* chain_mean, double* chain_within, double* sequence_mean, double* sequence_m2,
                                   int64_t* sequence_length, int64_t* num_sequences);
const char* mcmcpp_hip_gelman_rubin_last_error(void);

/* The effective sample size and the integrated autocorrelation time of every parameter over the same sequences: the
 * multi-sequence estimator of BDA3 / Stan that goes with the split R-hat above (an extension: autocorr_times above is the
 * reference's class, one pooled chain, and knows nothing of the between-chain variance).  Everything in fp64, each + - x /
 * rounded on its own, no fma.
 *   phase 1         sequences, split, H, L, M, the order m = (k H + h) W + w, sum_fixed, sequence_mean, within, between,
 *                   varplus, rhat and mean are exactly those of the Gelman-Rubin call above: these outputs equal that call's
 *                   on the same input bit for bit.
 *   per sequence m, parameter p, lag t
 *                   e_s = x_s - sequence_mean[m][p];  A_m[t] = e_0 e_t + e_1 e_(t+1) + ... + e_(L-1-t) e_(L-1), added in
 *                   ascending s from +0: a plain ascending sum (the slices of sum_fixed are not used along s).
 *   per parameter and lag
 *                   S[t] = sum_fixed over m of A_m[t];  gamma[t] = (S[t] / M) / L;  rho[0] = 1;  for t >= 1
 *                   rho[t] = 1 - (within - gamma[t]) / varplus.
 *   window          cap = L - 1 when max_lag = 0, otherwise min(max_lag, L - 1);  kmax = floor((cap - 1) / 2);
 *                   P_k = rho[2k] + rho[2k+1].  Walk k = 0, 1, ..., kmax; stop, with closed = 1, at the first k >= 1 for which
 *                   `P_k >= 0` is false (a NaN stops the walk).  Otherwise Q_0 = P_0, Q_k = P_k if P_k < Q_(k-1), else
 *                   Q_(k-1), and total = Q_0 + Q_1 + ... in ascending k.  lags_used = 2 x (pairs summed); closed = 0 when
 *                   kmax was summed without a stop.
 *   result          tau = -1 + 2 total; if tau < 1 / log10(N), tau = 1 / log10(N), with N = M L as a double and the host
 *                   libm's log10 (a NaN tau stays);  ess = N / tau.  A constant parameter has varplus = 0: its rho, tau and
 *                   ess are NaN by IEEE rules.  Non-finite samples propagate.
 *   functions       n_functions >= 0: rho and autocov (= gamma), both [P][n_functions].  Every lag
 *                   t < min(n_functions, cap + 1) is evaluated and returned whether or not the window closed before it;
 *                   entries past that are NaN.
 *   rounds          lags are evaluated in rounds of whole blocks of 32: the first covers MCMCPP_HIP_ESS_FIRST_LAGS lags
 *                   (default 64; at least min(n_functions, cap + 1)); while a parameter's window is neither closed nor at
 *                   its cap, the next round is twice as long.  A round holds no more lags than fit MCMCPP_HIP_ESS_WORK_MB
 *                   (default 1024) of lagged products, 8 M P bytes a lag, and one block at the least.  Both are read per
 *                   call, and neither they nor the CU count nor where the chain lies change a bit of any output.
 *   steps           as for the Gelman-Rubin call (phase 1 uploads them in its chunks).  For the lagged products one
 *                   (chain, half) of L steps is the unit of upload; the units stay in device memory across the rounds where
 *                   they all fit and are uploaded again every round where they do not.  MCMCPP_HIP_E_NOMEM (with a message)
 *                   when one unit and one block of lagged products cannot be allocated.
 *   device_steps    as for the Gelman-Rubin call: chain_stride_steps, slice_interval, read where they lie.
 *   outputs         ess, tau [P] double; lags_used, closed [P] int64; rho, autocov [P][n_functions]; rhat, mean, within,
 *                   between [P]; *sequence_length = L, *num_sequences = M.  Any of them may be NULL.
 * Free functions with a thread-local last error.  MCMCPP_HIP_E_ARG (with a message), before the device is opened, for every
 * argument the Gelman-Rubin call refuses, and for max_lag < 0 and n_functions < 0; and for a device_steps that is not memory
 * of that device, or chains that do not all end inside its allocation.  Nothing is written to the outputs of a call that
 * fails. */
int mcmcpp_hip_effective_sample_size(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps,
                                     int32_t num_walkers, int32_t num_params, int32_t split, int64_t max_lag, int64_t n_functions,
                                     double* ess, double* tau, int64_t* lags_used, int64_t* closed, double* rho, double* autocov,
                                     double* rhat, double* mean, double* within, double* between, int64_t* sequence_length,
                                     int64_t* num_sequences);
int mcmcpp_hip_effective_sample_size_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains,
                                            int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval, int32_t num_walkers,
                                            int32_t num_params, int32_t split, int64_t max_lag, int64_t n_functions, double* ess,
                                            double* tau, int64_t* lags_used, int64_t* closed, double* rho, double* autocov,
                                            double* rhat, double* mean, double* within, double* between, int64_t* sequence_length,
                                            int64_t* num_sequences);
const char* mcmcpp_hip_effective_sample_size_last_error(void);

/* The normal scores of the draws of every parameter: the rank-normalisation of Vehtari, Gelman, Simpson, Carpenter and
 * Buerkner (2021), on which the rank-normalised R-hat and the bulk-ESS below rest (an extension).  Ranks are integers, found
 * exactly by a stable radix sort on the device; everything after them is fp64, each + - x / rounded on its own, no fma.
 *   draws           the sequences, split, H, L and M are exactly those of the Gelman-Rubin call above.  With split and an odd
 *                   number n of used steps the middle used step belongs to no sequence and is not ranked.  A parameter has
 *                   S = M L draws, 2 <= S <= 2^31 - 1.  Step j of chain k of the output is the j-th used step of that chain
 *                   that belongs to a sequence: scores is a chain [K][H L][W][P] whose own split halves are the sequences.
 *   order           x_(i), i = 0 .. S - 1: the i-th smallest draw of the parameter in the total order of
 *                   mcmcpp_hip_order_statistics (-inf < ... < -0 < +0 < ... < +inf).  A float draw converts to double exactly.
 *   quantile q      h = q (S - 1) in double, lo = floor(h), hi = ceil(h); x_(lo) where x_(lo) == x_(hi), else
 *                   x_(lo) + (x_(hi) - x_(lo)) (h - floor(h)).  median = quantile 0.5, q05 = quantile 0.05, q95 = quantile 0.95.
 *   value ranked    fold == 0: v = x.  fold != 0: v = |x - median| in double.
 *   rank            values compare as numbers (-0 == +0).  below = #{v' < v}, equal = #{v' == v} over the S draws;
 *                   r = below + (equal + 1) / 2: the average rank, exact in double.
 *   score           p = (r - 0.375) / (S + 0.25);  z = mcmcpp::normal_score(p) of mcmcpp_amd/csrc/normal_score.hpp: Wichura's
 *                   AS 241 (PPND16) in the evaluation order that header's comment states, with a logarithm of its own.  The
 *                   device and the host produce the same bits.  All S draws equal: every z is +0.
 *   knobs           parameters are ranked a tile at a time, as many as fit MCMCPP_HIP_RANK_WORK_MB (read per call, default
 *                   1024; one parameter at the least: 2 S (key bytes + 4) bytes and the digit tables).  Host chains are
 *                   uploaded once, as the sequences' steps, in copy groups of MCMCPP_HIP_RHAT_CHUNK_MB.  Neither changes a bit.
 *   memory          held in device memory together: the fp64 chain of scores, 8 K H L W P bytes (the caller's for the device
 *                   form of the normal scores, the library's otherwise); for host chains their upload as well, (element size)
 *                   x K H L W P bytes -- MCMCPP_HIP_RHAT_CHUNK_MB groups the copies and bounds no memory, unlike in the R-hat
 *                   and ESS calls, which stream host chains through; and the sort workspace.  MCMCPP_HIP_E_NOMEM, with the
 *                   byte count, when one of them cannot be had.
 *   median          a quantile interpolated between -inf and a larger order statistic, or up to +inf from a smaller one, is
 *                   NaN or infinite by IEEE rules (-inf + inf), and is returned so for fold == 0.  A fold about a median
 *                   that is not finite would make every |x - median| NaN or infinite: it fails the call.
 *   steps, device_steps
 *                   as for the Gelman-Rubin call.
 *   outputs         scores [K][H L][W][P] double, required: host memory for mcmcpp_hip_normal_scores, caller-owned memory
 *                   of that device for mcmcpp_hip_normal_scores_device (checked to be such, and large enough); median, q05,
 *                   q95 [P] double; *sequence_length = L, *num_sequences = M; these may be NULL.
 * MCMCPP_HIP_E_ARG (with a message) for every argument the Gelman-Rubin call refuses, for S > 2^31 - 1, for S x num_params > 256 x (2^31 - 1) (a launch grid), a NULL scores, a
 * scores of the device form that is not memory of that device or too small, a NaN draw (it has no place in the order), and,
 * folded, a median that is not finite (the folded values would be NaN).  MCMCPP_HIP_E_NOMEM, with the byte count, when the
 * workspace of one parameter cannot be allocated.  Nothing is written to any output of a call that fails.  The thread-local
 * last error is mcmcpp_hip_rank_diagnostics_last_error's. */
int mcmcpp_hip_normal_scores(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps,
                             int32_t num_walkers, int32_t num_params, int32_t split, int32_t fold, double* scores, double* median,
                             double* q05, double* q95, int64_t* sequence_length, int64_t* num_sequences);
int mcmcpp_hip_normal_scores_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains,
                                    int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval, int32_t num_walkers,
                                    int32_t num_params, int32_t split, int32_t fold, double* scores, double* median, double* q05,
                                    double* q95, int64_t* sequence_length, int64_t* num_sequences);

/* Rank-normalised split R-hat, bulk-ESS and tail-ESS of every parameter (Vehtari et al. 2021; what Stan, ArviZ and `posterior`
 * report), defined by composition of the calls above:
 *   rhat_rank, ess_bulk, closed_bulk
 *                   the rhat, ess and closed that mcmcpp_hip_effective_sample_size_device(MCMCPP_HIP_F64, ...) returns on the
 *                   scores of fold = 0, read as K chains of H L steps with the same split and max_lag.
 *   rhat_folded     the rhat of mcmcpp_hip_gelman_rubin_device on the scores of fold = 1.
 *   ess_tail_lower, ess_tail_upper
 *                   that ESS call's ess on the fp64 chain [K][H L][W][P] of the indicators 1.0 / 0.0 of x <= q05 and of
 *                   x <= q95, compared in double (not rank-normalised, as in `posterior`).  A constant indicator gives NaN by
 *                   the ESS call's rule.  closed_tail = 1 where both windows closed.
 *   ess_tail        NaN if either is NaN, else the smaller.   rhat: NaN if rhat_rank or rhat_folded is NaN, else the larger.
 * The results are bit for bit those of the existing entry points on those chains, so they depend on the data alone.
 *   outputs         rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper, median, q05, q95 [P]
 *                   double; closed_bulk, closed_tail [P] int64; *sequence_length, *num_sequences.  Any of them may be NULL.
 * Failures as for the normal scores (there is no scores argument), and max_lag < 0.  Nothing is written to the outputs of a
 * call that fails. */
int mcmcpp_hip_rank_diagnostics(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps,
                                int32_t num_walkers, int32_t num_params, int32_t split, int64_t max_lag, double* rhat,
                                double* rhat_rank, double* rhat_folded, double* ess_bulk, double* ess_tail, double* ess_tail_lower,
                                double* ess_tail_upper, double* median, double* q05, double* q95, int64_t* closed_bulk,
                                int64_t* closed_tail, int64_t* sequence_length, int64_t* num_sequences);
int mcmcpp_hip_rank_diagnostics_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains,
                                       int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval, int32_t num_walkers,
                                       int32_t num_params, int32_t split, int64_t max_lag, double* rhat, double* rhat_rank,
                                       double* rhat_folded, double* ess_bulk, double* ess_tail, double* ess_tail_lower,
                                       double* ess_tail_upper, double* median, double* q05, double* q95, int64_t* closed_bulk,
                                       int64_t* closed_tail, int64_t* sequence_length, int64_t* num_sequences);
const char* mcmcpp_hip_rank_diagnostics_last_error(void);

/* The posterior summary of every parameter: mean, sd, quantiles and a highest-density interval, each with its Monte Carlo
 * standard error and effective sample size (Vehtari et al. 2021, section 4: mcse_mean, mcse_sd, mcse_quantile, ess_quantile; the
 * row Stan, `posterior` and ArviZ print), an extension.  The sequences, H, L, M, S = M L, the draw order and the total order
 * x_(0) <= ... <= x_(S-1) are those of mcmcpp_hip_normal_scores.  All arithmetic is fp64, each + - x / sqrt rounded on its own, no
 * fma, no floating-point atomics.  "The ESS call" below is mcmcpp_hip_effective_sample_size_device(MCMCPP_HIP_F64, ...) with the
 * same split and max_lag on an fp64 chain [K][H L][W][P] in device memory whose draw j, parameter p holds the value named: the
 * figures are that entry point's bits.
 *   mean, ess_mean  the ESS call's mean and ess on the draws as they are (a float draw converts to double exactly).
 *   sd              with that call's within and between: var = (((L-1) M) within + (L (M-1)) between) / (S-1), the integer
 *                   products exact; sd = sqrt(var): the pooled sample variance with one degree of freedom removed.
 *   mcse_mean       sd / sqrt(ess_mean).
 *   ess_sd, mcse_sd c = (x - mean) (x - mean) in double.  ess_sd = the ESS call's ess on c, Evar its mean, and with its within_c,
 *                   between_c: m4c = (((L-1) M) within_c + (L (M-1)) between_c) / S;  mcse_sd = sqrt(((m4c / ess_sd) / Evar) / 4)
 *                   (`posterior`'s rule).
 *   quantile        [P][n_probs]: the "quantile q" rule of mcmcpp_hip_normal_scores for q = probs[i].
 *   ess_quantile    [P][n_probs]: the ESS call's ess on the indicators 1.0 / 0.0 of x <= quantile[p][i], compared in double.
 *   mcse_quantile, rank_lower, rank_upper
 *                   [P][n_probs]: a = ess_quantile prob + 1, b = ess_quantile (1 - prob) + 1;
 *                   u_lo = beta_quantile(0.15865525393145707, a, b), u_hi = beta_quantile(0.8413447460685429, a, b);
 *                   rank_lower = max(floor(u_lo S), 1) - 1, rank_upper = min(ceil(u_hi S), S) - 1, the products in double;
 *                   mcse_quantile = (x_(rank_upper) - x_(rank_lower)) / 2.  A NaN ess_quantile gives NaN and ranks -1.
 *   beta_quantile   mcmcpp_hip_beta_quantile below: specified to a relative accuracy of 1e-10, not to bits (it rests on the host
 *                   libm), so the two ranks are exact wherever u S lies further than S x 1e-10 from an integer.  Everything
 *                   else in this call is defined to the bit.
 *   hdi_lower, hdi_upper
 *                   [P], where hdi_prob != 0: m = floor(hdi_prob S) in double; w_i = x_(i+m) - x_(i) for 0 <= i < S - m; the
 *                   smallest w_i that is not NaN, among equal widths the lowest i; the bounds are x_(i) and x_(i+m) (ArviZ's
 *                   rule for one mode).  Every width NaN (inf - inf): both bounds NaN.  hdi_prob = 0: no interval, the two
 *                   outputs are not written.
 *   knobs, memory   as for mcmcpp_hip_rank_diagnostics: MCMCPP_HIP_RANK_WORK_MB, MCMCPP_HIP_RHAT_CHUNK_MB and where the chain
 *                   lies change no bit.  The parameters are sorted once, a tile at a time; where they do not fit one tile,
 *                   their sorted keys are kept for the ranks of mcse_quantile ((element size) x S P bytes more), and where
 *                   that exceeds MCMCPP_HIP_SUMMARY_KEEP_MB (read per call; default: no bound) or the device's memory, every
 *                   tile is sorted a second time instead.  No bit depends on which.
 *   outputs         mean, sd, mcse_mean, ess_mean, ess_sd, mcse_sd, hdi_lower, hdi_upper [P] double; quantile, ess_quantile,
 *                   mcse_quantile [P][n_probs] double; rank_lower, rank_upper [P][n_probs] int64; *sequence_length = L,
 *                   *num_sequences = M.  Any of them may be NULL.
 * MCMCPP_HIP_E_ARG (with a message), before the device is opened, for everything mcmcpp_hip_rank_diagnostics refuses, and for
 * n_probs outside 0..16, a NULL probs with n_probs > 0, a prob that is not inside (0, 1), and an hdi_prob that is neither 0
 * nor inside (0, 1) with 1 <= floor(hdi_prob S) <= S - 1; then for a NaN draw.  Nothing is written to any output of a call
 * that fails. */
int mcmcpp_hip_posterior_summary(int32_t dtype, int32_t device, const void* const* steps, int32_t num_chains, int64_t n_steps,
                                 int32_t num_walkers, int32_t num_params, int32_t split, int64_t max_lag, const double* probs,
                                 int32_t n_probs, double hdi_prob, double* mean, double* sd, double* mcse_mean, double* ess_mean,
                                 double* ess_sd, double* mcse_sd, double* quantile, double* ess_quantile, double* mcse_quantile,
                                 int64_t* rank_lower, int64_t* rank_upper, double* hdi_lower, double* hdi_upper,
                                 int64_t* sequence_length, int64_t* num_sequences);
int mcmcpp_hip_posterior_summary_device(int32_t dtype, int32_t device, const void* device_steps, int32_t num_chains,
                                        int64_t chain_stride_steps, int64_t n_steps, int64_t slice_interval, int32_t num_walkers,
                                        int32_t num_params, int32_t split, int64_t max_lag, const double* probs, int32_t n_probs,
                                        double hdi_prob, double* mean, double* sd, double* mcse_mean, double* ess_mean, double* ess_sd,
                                        double* mcse_sd, double* quantile, double* ess_quantile, double* mcse_quantile,
                                        int64_t* rank_lower, int64_t* rank_upper, double* hdi_lower, double* hdi_upper,
                                        int64_t* sequence_length, int64_t* num_sequences);
const char* mcmcpp_hip_posterior_summary_last_error(void);

/* The x in (0, 1) with I_x(a, b) = p: the quantile function of the Beta distribution (mcmcpp_amd/csrc/beta_quantile.hpp: a
 * continued fraction inside a bracketed Newton iteration; its comment has the algorithm and the iteration caps).  Valid for
 * a, b in [1, 2^31 + 2] and 0 < p < 1, with a relative error below 1e-10.  Deterministic, but specified to that accuracy and
 * not to bits: it uses the host libm's lgamma, log and exp.  Opens no device. */
double mcmcpp_hip_beta_quantile(double p, double a, double b);

int mcmcpp_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MCMCPP_HIP_H */
