"""ctypes binding of include/mcmcpp_hip.h.  There is no CPU fallback: if libmcmcpp_hip.so cannot be
loaded, or a call fails, an exception carrying the library's own error message is raised."""
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

F64, F32 = 0, 1
CALC_ISO_GAUSSIAN, CALC_DENSE_GAUSSIAN, CALC_ROSENBROCK, CALC_SKEWED_GAUSSIAN_2D = 0, 1, 2, 3
CALC_BATCH = 4  # a host callback evaluates each half-step's proposals in one batch (HipSampler(log_prob=...))
MOVER_STRETCH, MOVER_DIFFERENTIAL_EVOLUTION = 0, 1
OK = 0
E_CALLBACK = 8

# mcmcpp_hip_batch_logp_fn: (user, proposals, logp_out, count, num_params, hip_stream) -> int
BATCH_LOGP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)

# every symbol include/mcmcpp_hip.h declares
EXPORTS = [
    "mcmcpp_hip_abi_version", "mcmcpp_hip_register_calculator", "mcmcpp_hip_create", "mcmcpp_hip_destroy", "mcmcpp_hip_last_error",
    "mcmcpp_hip_set_batch_calculator", "mcmcpp_hip_set_state", "mcmcpp_hip_seek", "mcmcpp_hip_run", "mcmcpp_hip_get_state", "mcmcpp_hip_reset_counters",
    "mcmcpp_hip_get_counters", "mcmcpp_hip_calc_logp", "mcmcpp_hip_set_chain_params", "mcmcpp_hip_calc_logp_chain", "mcmcpp_hip_last_run_timing", "mcmcpp_hip_last_run_host_timing",
    "mcmcpp_hip_comm_unique_id", "mcmcpp_hip_last_run_exchange", "mcmcpp_hip_run_async", "mcmcpp_hip_wait_stored", "mcmcpp_hip_run_wait",
    "mcmcpp_hip_host_alloc", "mcmcpp_hip_host_free",
    "mcmcpp_hip_device_alloc", "mcmcpp_hip_device_free", "mcmcpp_hip_device_copy", "mcmcpp_hip_device_chain_last_error",
    "mcmcpp_hip_device_chain_compact",
    "mcmcpp_hip_run_device", "mcmcpp_hip_run_device_async", "mcmcpp_hip_calc_logp_device", "mcmcpp_hip_moments_add_device_steps_strided",
    "mcmcpp_hip_half_step_async", "mcmcpp_hip_bind_device_chain", "mcmcpp_hip_device_positions",
    "mcmcpp_hip_shard_span", "mcmcpp_hip_synchronize", "mcmcpp_hip_exchange_chains",
    "mcmcpp_hip_run_tempered", "mcmcpp_hip_run_tempered_device", "mcmcpp_hip_evidence_ratios", "mcmcpp_hip_evidence_ratios_device",
    "mcmcpp_hip_evidence_bridge", "mcmcpp_hip_evidence_bridge_device", "mcmcpp_hip_evidence_mbar", "mcmcpp_hip_evidence_mbar_device",
    "mcmcpp_hip_evidence_gaussian", "mcmcpp_hip_evidence_gaussian_device",
    "mcmcpp_hip_evidence_gaussian_last_timing",
    "mcmcpp_hip_moments_create", "mcmcpp_hip_moments_destroy", "mcmcpp_hip_moments_reset", "mcmcpp_hip_moments_add_steps",
    "mcmcpp_hip_moments_add_device_steps", "mcmcpp_hip_moments_finish", "mcmcpp_hip_moments_last_error",
    "mcmcpp_hip_autocorr_times", "mcmcpp_hip_autocorr_times_device", "mcmcpp_hip_autocorr_last_error",
    "mcmcpp_hip_histograms_create", "mcmcpp_hip_histograms_destroy", "mcmcpp_hip_histograms_compute",
    "mcmcpp_hip_histograms_compute_device", "mcmcpp_hip_histograms_result", "mcmcpp_hip_histograms_last_error",
    "mcmcpp_hip_order_statistics", "mcmcpp_hip_order_statistics_device", "mcmcpp_hip_rank_counts", "mcmcpp_hip_rank_counts_device",
    "mcmcpp_hip_order_statistics_last_error",
    "mcmcpp_hip_gelman_rubin", "mcmcpp_hip_gelman_rubin_device", "mcmcpp_hip_gelman_rubin_last_error",
    "mcmcpp_hip_effective_sample_size", "mcmcpp_hip_effective_sample_size_device", "mcmcpp_hip_effective_sample_size_last_error",
    "mcmcpp_hip_normal_scores", "mcmcpp_hip_normal_scores_device", "mcmcpp_hip_rank_diagnostics", "mcmcpp_hip_rank_diagnostics_device",
    "mcmcpp_hip_rank_diagnostics_last_error",
    "mcmcpp_hip_posterior_summary", "mcmcpp_hip_posterior_summary_device", "mcmcpp_hip_posterior_summary_last_error", "mcmcpp_hip_beta_quantile",
]


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("dtype", C.c_int32), ("num_walkers", C.c_int32),
                ("num_params", C.c_int32), ("calc_id", C.c_int32), ("calc_params_len", C.c_int32),
                ("calc_params", C.c_void_p), ("seed", C.c_uint64), ("stream", C.c_uint64), ("device", C.c_int32),
                ("shard_begin", C.c_int32), ("shard_count", C.c_int32), ("graph_steps", C.c_int32),
                ("gw_alpha_num", C.c_int32), ("gw_alpha_den", C.c_int32),
                ("device_positions", C.c_void_p), ("hip_stream", C.c_void_p), ("flags", C.c_uint32),
                ("mover", C.c_uint32), ("comm_world", C.c_int32), ("comm_rank", C.c_int32), ("comm_id", C.c_void_p),
                ("comm", C.c_void_p), ("num_chains", C.c_int32), ("reserved0", C.c_int32)]

FLAG_CALLER_STREAM = 1
COMM_ID_BYTES = 128


def library_path():
    # MCMCPP_HIP_LIB: load another build of the library instead (e.g. to compare two builds in one job)
    return os.environ.get("MCMCPP_HIP_LIB") or os.path.join(_HERE, "libmcmcpp_hip.so")


def build_library(force=False):
    """Compile every HIP source for gfx950 into mcmcpp_amd/libmcmcpp_hip.so (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        subprocess.check_call(args + ["clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return library_path()


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % path)
        L = C.CDLL(path)
        vp, i32, i64, u64p = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_uint64)
        L.mcmcpp_hip_abi_version.restype = C.c_int
        L.mcmcpp_hip_register_calculator.argtypes = [i32, vp, vp, i32]
        L.mcmcpp_hip_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.mcmcpp_hip_destroy.argtypes = [vp]
        L.mcmcpp_hip_destroy.restype = None
        L.mcmcpp_hip_last_error.argtypes = [vp]
        L.mcmcpp_hip_last_error.restype = C.c_char_p
        L.mcmcpp_hip_set_state.argtypes = [vp, vp, vp]
        if hasattr(L, "mcmcpp_hip_set_batch_calculator"):
            L.mcmcpp_hip_set_batch_calculator.argtypes = [vp, vp, vp, vp, vp]
        L.mcmcpp_hip_seek.argtypes = [vp, C.c_uint64]
        L.mcmcpp_hip_run.argtypes = [vp, i64, i32, vp, vp]
        L.mcmcpp_hip_get_state.argtypes = [vp, vp, vp, vp]
        L.mcmcpp_hip_reset_counters.argtypes = [vp]
        L.mcmcpp_hip_get_counters.argtypes = [vp, u64p, u64p, u64p, u64p]
        L.mcmcpp_hip_calc_logp.argtypes = [vp, vp, i64, vp]
        if hasattr(L, "mcmcpp_hip_set_chain_params"):
            L.mcmcpp_hip_set_chain_params.argtypes = [vp, i32, vp, i32]
            L.mcmcpp_hip_calc_logp_chain.argtypes = [vp, i32, vp, i64, vp]
        L.mcmcpp_hip_last_run_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64)]
        dp = C.POINTER(C.c_double)
        L.mcmcpp_hip_last_run_host_timing.argtypes = [vp, dp, dp, dp]
        L.mcmcpp_hip_comm_unique_id.argtypes = [vp]
        L.mcmcpp_hip_last_run_exchange.argtypes = [vp, dp, C.POINTER(i64), C.POINTER(i64)]
        L.mcmcpp_hip_run_async.argtypes = [vp, i64, i32, vp, vp]
        if hasattr(L, "mcmcpp_hip_run_device"):  # (absent from earlier builds selected with MCMCPP_HIP_LIB)
            L.mcmcpp_hip_run_device.argtypes = [vp, i64, i32, vp, vp]
            L.mcmcpp_hip_run_device_async.argtypes = [vp, i64, i32, vp, vp]
            L.mcmcpp_hip_calc_logp_device.argtypes = [vp, i32, vp, i64, vp]
        L.mcmcpp_hip_wait_stored.argtypes = [vp, i64]
        L.mcmcpp_hip_run_wait.argtypes = [vp]
        L.mcmcpp_hip_host_alloc.argtypes = [C.c_uint64]
        L.mcmcpp_hip_host_alloc.restype = vp
        L.mcmcpp_hip_host_free.argtypes = [vp]
        L.mcmcpp_hip_host_free.restype = None
        if hasattr(L, "mcmcpp_hip_device_alloc"):  # (absent from earlier builds selected with MCMCPP_HIP_LIB)
            L.mcmcpp_hip_device_alloc.argtypes = [i32, C.c_uint64]
            L.mcmcpp_hip_device_alloc.restype = vp
            L.mcmcpp_hip_device_free.argtypes = [vp]
            L.mcmcpp_hip_device_free.restype = None
            L.mcmcpp_hip_device_copy.argtypes = [vp, vp, C.c_uint64]
            L.mcmcpp_hip_device_chain_last_error.argtypes = []
            L.mcmcpp_hip_device_chain_last_error.restype = C.c_char_p
            L.mcmcpp_hip_device_chain_compact.argtypes = [i32, i32, vp, i64, i64, i64, i64, C.POINTER(i64)]
        L.mcmcpp_hip_half_step_async.argtypes = [vp, i32, i64]
        L.mcmcpp_hip_bind_device_chain.argtypes = [vp, vp, i64]
        L.mcmcpp_hip_device_positions.argtypes = [vp]
        L.mcmcpp_hip_device_positions.restype = vp
        L.mcmcpp_hip_shard_span.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64)]
        L.mcmcpp_hip_synchronize.argtypes = [vp]
        if hasattr(L, "mcmcpp_hip_exchange_chains"):  # (absent from earlier builds selected with MCMCPP_HIP_LIB)
            L.mcmcpp_hip_exchange_chains.argtypes = [vp, C.c_uint64, vp, vp, vp]
        if hasattr(L, "mcmcpp_hip_run_tempered"):  # (likewise)
            L.mcmcpp_hip_run_tempered.argtypes = [vp, i64, i32, i64, C.c_uint64, vp, vp, vp, vp, vp, u64p]
            L.mcmcpp_hip_run_tempered_device.argtypes = [vp, i64, i32, i64, C.c_uint64, vp, vp, vp, vp, vp, u64p]
        if hasattr(L, "mcmcpp_hip_evidence_ratios"):  # (likewise)
            outputs = [vp] * 9  # log_ratio, mcse, ess, kish, max_u, nonfinite, log_ratio_total, mcse_total, *num_draws
            L.mcmcpp_hip_evidence_ratios.argtypes = [vp, C.POINTER(vp), i64, i64] + outputs
            L.mcmcpp_hip_evidence_ratios_device.argtypes = [vp, vp, i64, i64, i64] + outputs
        if hasattr(L, "mcmcpp_hip_evidence_bridge"):  # (likewise)
            outputs = [vp] * 10  # log_ratio, mcse, overlap, ess, passes, converged, nonfinite, log_ratio_total, mcse_total, *num_draws
            L.mcmcpp_hip_evidence_bridge.argtypes = [vp, C.POINTER(vp), i64, i64] + outputs
            L.mcmcpp_hip_evidence_bridge_device.argtypes = [vp, vp, i64, i64, i64] + outputs
        if hasattr(L, "mcmcpp_hip_evidence_mbar"):  # (likewise)
            outputs = [vp] * 11  # log_z, cov, log_ratio, mcse, ess, nonfinite, log_ratio_total, mcse_total, *passes, *converged, *num_draws
            L.mcmcpp_hip_evidence_mbar.argtypes = [vp, C.POINTER(vp), i64, i64] + outputs
            L.mcmcpp_hip_evidence_mbar_device.argtypes = [vp, vp, i64, i64, i64] + outputs
        if hasattr(L, "mcmcpp_hip_evidence_gaussian"):  # (likewise)
            # mean, chol, seed, stream; log_evidence, mcse, overlap, ess, passes, converged, nonfinite, *num_draws, proposals, log_q
            tail = [vp, vp, C.c_uint64, C.c_uint64] + [vp] * 10
            L.mcmcpp_hip_evidence_gaussian.argtypes = [vp, i32, C.POINTER(vp), i64, i64] + tail
            L.mcmcpp_hip_evidence_gaussian_device.argtypes = [vp, i32, vp, i64, i64] + tail
            L.mcmcpp_hip_evidence_gaussian_last_timing.argtypes = [dp, dp]
            L.mcmcpp_hip_evidence_gaussian_last_timing.restype = None
        if hasattr(L, "mcmcpp_hip_moments_create"):  # (absent only from older experiment builds selected with MCMCPP_HIP_LIB)
            L.mcmcpp_hip_moments_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
            L.mcmcpp_hip_moments_destroy.argtypes = [vp]
            L.mcmcpp_hip_moments_destroy.restype = None
            L.mcmcpp_hip_moments_reset.argtypes = [vp]
            L.mcmcpp_hip_moments_add_steps.argtypes = [vp, vp, i64, i64]
            L.mcmcpp_hip_moments_add_device_steps.argtypes = [vp, vp, i64]
            if hasattr(L, "mcmcpp_hip_moments_add_device_steps_strided"):
                L.mcmcpp_hip_moments_add_device_steps_strided.argtypes = [vp, vp, i64, i64]
            L.mcmcpp_hip_moments_finish.argtypes = [vp, C.POINTER(i64), vp, vp, vp]
            L.mcmcpp_hip_moments_last_error.argtypes = [vp]
            L.mcmcpp_hip_moments_last_error.restype = C.c_char_p
        if hasattr(L, "mcmcpp_hip_autocorr_times"):
            L.mcmcpp_hip_autocorr_times.argtypes = [i32, i32, C.POINTER(vp), i64, i32, i32, i32, i32, vp, vp]
            L.mcmcpp_hip_autocorr_times_device.argtypes = [i32, i32, vp, i64, i32, i32, i32, i32, vp, vp]
            L.mcmcpp_hip_autocorr_last_error.argtypes = []
            L.mcmcpp_hip_autocorr_last_error.restype = C.c_char_p
        if hasattr(L, "mcmcpp_hip_histograms_create"):
            L.mcmcpp_hip_histograms_create.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
            L.mcmcpp_hip_histograms_destroy.argtypes = [vp]
            L.mcmcpp_hip_histograms_destroy.restype = None
            L.mcmcpp_hip_histograms_compute.argtypes = [vp, C.POINTER(vp), i64]
            L.mcmcpp_hip_histograms_compute_device.argtypes = [vp, vp, i64, i64]
            L.mcmcpp_hip_histograms_result.argtypes = [vp, C.POINTER(i64), vp, vp, vp, vp]
            L.mcmcpp_hip_histograms_last_error.argtypes = [vp]
            L.mcmcpp_hip_histograms_last_error.restype = C.c_char_p
        if hasattr(L, "mcmcpp_hip_order_statistics"):
            L.mcmcpp_hip_order_statistics.argtypes = [i32, i32, C.POINTER(vp), i64, i32, i32, vp, i32, vp]
            L.mcmcpp_hip_order_statistics_device.argtypes = [i32, i32, vp, i64, i64, i32, i32, vp, i32, vp]
            L.mcmcpp_hip_rank_counts.argtypes = [i32, i32, C.POINTER(vp), i64, i32, i32, vp, i32, vp, vp]
            L.mcmcpp_hip_rank_counts_device.argtypes = [i32, i32, vp, i64, i64, i32, i32, vp, i32, vp, vp]
            L.mcmcpp_hip_order_statistics_last_error.argtypes = []
            L.mcmcpp_hip_order_statistics_last_error.restype = C.c_char_p
        if hasattr(L, "mcmcpp_hip_gelman_rubin"):
            outputs = [vp] * 10  # eight double arrays, *sequence_length, *num_sequences
            L.mcmcpp_hip_gelman_rubin.argtypes = [i32, i32, C.POINTER(vp), i32, i64, i32, i32, i32] + outputs
            L.mcmcpp_hip_gelman_rubin_device.argtypes = [i32, i32, vp, i32, i64, i64, i64, i32, i32, i32] + outputs
            L.mcmcpp_hip_gelman_rubin_last_error.argtypes = []
            L.mcmcpp_hip_gelman_rubin_last_error.restype = C.c_char_p
        if hasattr(L, "mcmcpp_hip_effective_sample_size"):
            outputs = [vp] * 12  # ess, tau, lags_used, closed, rho, autocov, rhat, mean, within, between, *sequence_length, *num_sequences
            L.mcmcpp_hip_effective_sample_size.argtypes = [i32, i32, C.POINTER(vp), i32, i64, i32, i32, i32, i64, i64] + outputs
            L.mcmcpp_hip_effective_sample_size_device.argtypes = [i32, i32, vp, i32, i64, i64, i64, i32, i32, i32, i64, i64] + outputs
            L.mcmcpp_hip_effective_sample_size_last_error.argtypes = []
            L.mcmcpp_hip_effective_sample_size_last_error.restype = C.c_char_p
        if hasattr(L, "mcmcpp_hip_normal_scores"):
            outputs = [vp] * 6  # scores, median, q05, q95, *sequence_length, *num_sequences
            L.mcmcpp_hip_normal_scores.argtypes = [i32, i32, C.POINTER(vp), i32, i64, i32, i32, i32, i32] + outputs
            L.mcmcpp_hip_normal_scores_device.argtypes = [i32, i32, vp, i32, i64, i64, i64, i32, i32, i32, i32] + outputs
            outputs = [vp] * 14  # ten double arrays, closed_bulk, closed_tail, *sequence_length, *num_sequences
            L.mcmcpp_hip_rank_diagnostics.argtypes = [i32, i32, C.POINTER(vp), i32, i64, i32, i32, i32, i64] + outputs
            L.mcmcpp_hip_rank_diagnostics_device.argtypes = [i32, i32, vp, i32, i64, i64, i64, i32, i32, i32, i64] + outputs
            L.mcmcpp_hip_rank_diagnostics_last_error.argtypes = []
            L.mcmcpp_hip_rank_diagnostics_last_error.restype = C.c_char_p
        if hasattr(L, "mcmcpp_hip_posterior_summary"):  # (absent from earlier builds selected with MCMCPP_HIP_LIB)
            tail = [i32, i64, vp, i32, C.c_double] + [vp] * 15  # split, max_lag, probs, n_probs, hdi_prob; thirteen arrays, *sequence_length, *num_sequences
            L.mcmcpp_hip_posterior_summary.argtypes = [i32, i32, C.POINTER(vp), i32, i64, i32, i32] + tail
            L.mcmcpp_hip_posterior_summary_device.argtypes = [i32, i32, vp, i32, i64, i64, i64, i32, i32] + tail
            L.mcmcpp_hip_posterior_summary_last_error.argtypes = []
            L.mcmcpp_hip_posterior_summary_last_error.restype = C.c_char_p
            L.mcmcpp_hip_beta_quantile.argtypes = [C.c_double, C.c_double, C.c_double]
            L.mcmcpp_hip_beta_quantile.restype = C.c_double
        _lib = L
    return _lib


def comm_unique_id():
    """The rendezvous token of a new RCCL communicator (make it on one rank, hand it to all)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().mcmcpp_hip_comm_unique_id(buf)
    if rc != OK:
        raise HipError(rc, lib().mcmcpp_hip_last_error(None).decode())
    return buf.raw


def pinned_empty(shape, dtype=np.float64):
    """A numpy array in pinned host memory (mcmcpp_hip_host_alloc), e.g. a chain block the launches can write into."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    p = lib().mcmcpp_hip_host_alloc(n * dt.itemsize)
    if not p:
        raise MemoryError("mcmcpp_hip_host_alloc(%d) failed" % (n * dt.itemsize))
    buf = (C.c_char * (n * dt.itemsize)).from_address(p)
    # the memory goes back when nothing refers to the buffer any more (numpy keeps it alive through arr.base)
    weakref.finalize(buf, lib().mcmcpp_hip_host_free, p)
    return np.frombuffer(buf, dtype=dt).reshape(shape)


def device_chain_compact(steps, burn_in, interval, n_steps=None, step_elems=None, dtype=None, device=-1):
    """Chain::resetChainForSubSampling on stored steps in device memory, in place (mcmcpp_hip_device_chain_compact): a contiguous
    float64 / float32 device tensor (n, W, D), or an integer address with n_steps, step_elems and dtype given.  Returns the number
    of steps kept; they are the first ones of the array afterwards."""
    if _is_tensor(steps):
        import torch
        if steps.dim() != 3 or steps.dtype not in (torch.float64, torch.float32) or not steps.is_cuda or not steps.is_contiguous():
            raise ValueError("device steps must be a contiguous float64 or float32 device tensor (n, W, D)")
        dtype = F64 if steps.dtype == torch.float64 else F32
        n_steps, step_elems = steps.shape[0], steps.shape[1] * steps.shape[2]
        device = steps.device.index if device < 0 else device
        _after_torch(steps)
        ptr = steps.data_ptr()
    else:
        if n_steps is None or step_elems is None or dtype is None:
            raise ValueError("an integer device address needs n_steps, step_elems and dtype")
        ptr = int(steps)
    kept = C.c_int64(0)
    rc = lib().mcmcpp_hip_device_chain_compact(dtype, device, C.c_void_p(ptr), n_steps, step_elems, burn_in, interval, C.byref(kept))
    if rc != OK:
        raise HipError(rc, (lib().mcmcpp_hip_device_chain_last_error() or b"").decode())
    return kept.value


def np_dtype(dtype):
    return np.float64 if dtype == F64 else np.float32


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _is_tensor(x):
    """A torch tensor?  (Without importing torch: whoever holds a tensor has imported it.)"""
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _torch_dtype(dtype):
    import torch
    return torch.float64 if dtype == F64 else torch.float32


def _after_torch(t):
    """The library launches on streams of its own, which wait for nothing torch has enqueued.  Before a tensor's memory is
    handed to it, the current torch stream of the tensor's device is therefore drained: the work that produces the tensor, a
    copy that made it contiguous, and whatever last used the block the caching allocator gave a fresh tensor.  (Work the
    caller has put on another torch stream is the caller's to order, as it is between two torch streams.)  The library's
    calls return when their results are there, so nothing is needed behind them."""
    import torch
    torch.cuda.current_stream(t.device).synchronize()


def _device_steps(steps, n_steps, W, D, dtype, device=None):
    """(address, n_steps) of stored steps in device memory: a contiguous device tensor (n, W, D) of the handle's dtype (and
    device, where known), or an integer address with n_steps given."""
    if not _is_tensor(steps):
        if n_steps is None:
            raise ValueError("an integer device address needs n_steps")
        return int(steps), int(n_steps)
    if steps.dim() != 3 or tuple(steps.shape[1:]) != (W, D):
        raise ValueError("device steps must have shape (n, %d, %d), not %s" % (W, D, tuple(steps.shape)))
    if steps.dtype != _torch_dtype(dtype):
        raise ValueError("device steps must be %s, not %s" % (_torch_dtype(dtype), steps.dtype))
    if not steps.is_cuda or not steps.is_contiguous():
        raise ValueError("device steps must be a contiguous tensor in device memory")
    if device is not None and device >= 0 and steps.device.index != device:
        raise ValueError("device steps are on device %d, the handle on device %d" % (steps.device.index, device))
    if n_steps is not None and n_steps != steps.shape[0]:
        raise ValueError("n_steps = %d, but the tensor holds %d steps" % (n_steps, steps.shape[0]))
    _after_torch(steps)
    return steps.data_ptr(), int(steps.shape[0])


class HipError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "mcmcpp_hip error %d: %s" % (code, msg))
        self.code = code


class HipSampler:
    """Thin owner of one mcmcpp_hip_sampler handle (one GPU)."""

    def __init__(self, W, D, calc_id, params=None, seed=0, stream=0, dtype=F64, device=-1, shard_begin=0,
                 shard_count=0, graph_steps=0, device_positions=None, hip_stream=None, alpha=(2, 1), mover=0,
                 comm_world=0, comm_rank=0, comm_id=None, comm=None, num_chains=0, log_prob=None, batch_callback=None):
        """params: the calculator's parameters, shared by all chains; or, with num_chains = K > 1, one row per chain
        ((K, len) or (K, D, D)): row 0 goes to create, rows 1.. to set_chain_params.

        comm_world >= 1: this handle is rank comm_rank of a split ensemble (comm_id: the 128 bytes of comm_unique_id(),
        the same on all ranks; or comm: an existing ncclComm_t as an integer); run() then steps the split ensemble.

        calc_id=CALC_BATCH takes the target from the caller, as exactly one of
          log_prob        fn(x) -> logp: x a torch tensor (W/2, D) on the handle's device, logp (W/2,) of the same dtype
                          (the handle then launches on a torch.cuda.Stream of its own, which fn's work is enqueued on)
          batch_callback  (fn, user): a C function pointer of type mcmcpp_hip_batch_logp_fn (an integer address or a
                          BATCH_LOGP_FN object) and its user pointer; the library's own device buffers are used."""
        if (calc_id == CALC_BATCH) != (log_prob is not None or batch_callback is not None):
            raise ValueError("log_prob / batch_callback go with calc_id=CALC_BATCH, and CALC_BATCH needs one of them")
        if log_prob is not None and batch_callback is not None:
            raise ValueError("give log_prob or batch_callback, not both")
        self._torch_stream = None
        if log_prob is not None:
            import torch
            dev = torch.device("cuda", device if device >= 0 else torch.cuda.current_device())
            self._torch_stream = torch.cuda.Stream(device=dev)
            hip_stream = self._torch_stream.cuda_stream
        self.W, self.D, self.dtype = W, D, dtype
        self.K = num_chains if num_chains > 1 else 1  # independent ensembles stepped together (leading array dimension)
        self.np_t = np_dtype(dtype)
        chain_params = None
        if params is not None:
            params = np.ascontiguousarray(params, dtype=self.np_t)
            # (a (D, D) precision matrix is one shared block even when K == D)
            if self.K > 1 and params.ndim >= 2 and params.shape[0] == self.K and not (calc_id == CALC_DENSE_GAUSSIAN and params.shape == (D, D)):
                chain_params = params.reshape(self.K, -1)
                params = chain_params[0]
        self.params = None if params is None else params.ravel()
        self._comm_id = None if comm_id is None else C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self.cfg = Config(C.sizeof(Config), dtype, W, D, calc_id, 0 if self.params is None else self.params.size,
                          _ptr(self.params), seed & (2**64 - 1), stream & (2**64 - 1), device, shard_begin,
                          shard_count, graph_steps, alpha[0], alpha[1], device_positions,
                          0 if hip_stream is None else hip_stream, 0 if hip_stream is None else FLAG_CALLER_STREAM, mover,
                          comm_world, comm_rank, None if self._comm_id is None else C.cast(self._comm_id, C.c_void_p), comm,
                          num_chains, 0)
        self.h = C.c_void_p()
        rc = lib().mcmcpp_hip_create(C.byref(self.cfg), C.byref(self.h))
        if rc != OK:
            raise HipError(rc, lib().mcmcpp_hip_last_error(None).decode())
        self._cb_error = None
        if log_prob is not None:
            self._set_torch_target(log_prob, dev)
        elif batch_callback is not None:
            fn, user = batch_callback
            self._cb = fn  # (kept alive as long as the handle)
            fp = C.cast(fn, C.c_void_p) if isinstance(fn, C._CFuncPtr) else C.c_void_p(fn)
            self._check(lib().mcmcpp_hip_set_batch_calculator(self.h, fp, user, None, None))
        if chain_params is not None:
            for k in range(1, self.K):
                self.set_chain_params(k, chain_params[k])

    def _set_torch_target(self, log_prob, dev):
        import torch
        tt = torch.float64 if self.dtype == F64 else torch.float32
        n = self.W // 2
        # the proposals are formed in, and the log-posteriors read from, these tensors' storage
        self._foreign = None  # calc_logp_device: (rows, out), the caller's tensors the callback is given pieces of
        self._prop = torch.empty((n, self.D), dtype=tt, device=dev)
        self._lp = torch.empty((n,), dtype=tt, device=dev)
        prop_ptr = self._prop.data_ptr()
        ts = self._torch_stream

        def trampoline(user, proposals, logp_out, count, num_params, hip_stream):
            try:
                assert num_params == self.D and 0 < count <= n
                if proposals == prop_ptr:
                    x, lp = self._prop[:count], self._lp[:count]
                else:
                    # mcmcpp_hip_calc_logp_device: rows of the caller's own.  Torch cannot wrap a bare address, so the rows
                    # must be a piece of the tensors HipSampler.calc_logp_device has announced
                    if self._foreign is None:
                        raise ValueError("a torch log_prob handle evaluates foreign rows through HipSampler.calc_logp_device only")
                    rows, out = self._foreign
                    first, rest = divmod(proposals - rows.data_ptr(), rows.element_size() * self.D)
                    assert rest == 0 and 0 <= first and first + count <= rows.shape[0]
                    assert logp_out == out.data_ptr() + first * out.element_size()
                    x, lp = rows[first:first + count], out[first:first + count]
                # (the current stream is thread-local: run_async calls from the handle's worker thread)
                with torch.cuda.device(dev), torch.cuda.stream(ts):
                    y = log_prob(x)
                    if not isinstance(y, torch.Tensor) or tuple(y.shape) != (count,) or y.dtype != tt or y.device != dev:
                        raise TypeError("log_prob must return a tensor of shape (%d,), dtype %s on %s; got %s" % (
                            count, tt, dev, (tuple(y.shape), y.dtype, y.device) if isinstance(y, torch.Tensor) else type(y)))
                    lp.copy_(y)
                return 0
            except BaseException as e:  # (nothing may propagate through the C frames)
                self._cb_error = e
                return 1

        self._cb = BATCH_LOGP_FN(trampoline)  # (kept alive as long as the handle)
        self._check(lib().mcmcpp_hip_set_batch_calculator(self.h, C.cast(self._cb, C.c_void_p), None, C.c_void_p(prop_ptr),
                                                          C.c_void_p(self._lp.data_ptr())))

    def close(self):
        if getattr(self, "h", None):
            lib().mcmcpp_hip_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc):
        if rc != OK:
            err = HipError(rc, lib().mcmcpp_hip_last_error(self.h).decode())
            cause, self._cb_error = getattr(self, "_cb_error", None), None
            if rc == E_CALLBACK and cause is not None:
                raise err from cause
            raise err

    def set_state(self, pos, logp):
        pos = np.ascontiguousarray(pos, dtype=self.np_t)
        logp = np.ascontiguousarray(logp, dtype=self.np_t)
        assert pos.size == self.K * self.W * self.D and logp.size == self.K * self.W
        self._check(lib().mcmcpp_hip_set_state(self.h, _ptr(pos), _ptr(logp)))

    def seek(self, ensemble_steps_done):
        self._check(lib().mcmcpp_hip_seek(self.h, ensemble_steps_done))

    def run(self, n_saved, interval=1, save_chain=True, want_accepted=True, out=None):
        """out: optional preallocated (n_saved, W, D) array receiving the stored steps (like a Chain block that
        already exists); by default a fresh array is allocated."""
        lead = (self.K,) if self.K > 1 else ()  # several chains: chain[K][n_saved][W][D], acc[K][steps]
        if out is not None:
            assert save_chain and out.shape == lead + (n_saved, self.W, self.D) and out.dtype == self.np_t and out.flags.c_contiguous
        chain = out if out is not None else (np.empty(lead + (n_saved, self.W, self.D), dtype=self.np_t) if save_chain else None)
        acc = np.zeros(lead + (n_saved * interval,), dtype=np.uint32) if want_accepted else None
        self._check(lib().mcmcpp_hip_run(self.h, n_saved, interval, _ptr(chain), _ptr(acc)))
        return chain, acc

    def run_async(self, n_saved, interval=1, out=None, want_accepted=False):
        """Start the run on the handle's worker thread; returns (chain, acc) arrays that fill up as it proceeds
        (several chains: chain[K][n_saved][W][D], acc[K][steps], as run returns them)."""
        lead = (self.K,) if self.K > 1 else ()
        if out is not None:
            assert out.shape == lead + (n_saved, self.W, self.D) and out.dtype == self.np_t and out.flags.c_contiguous
        chain = out if out is not None else np.empty(lead + (n_saved, self.W, self.D), dtype=self.np_t)
        acc = np.zeros(lead + (n_saved * interval,), dtype=np.uint32) if want_accepted else None
        self._async_keep = (chain, acc)
        self._check(lib().mcmcpp_hip_run_async(self.h, n_saved, interval, _ptr(chain), _ptr(acc)))
        return chain, acc

    def _device_out(self, n_saved, out):
        """(address, what run_device returns) of a device destination: a fresh tensor, the caller's tensor, or (address, nbytes)"""
        shape = ((self.K,) if self.K > 1 else ()) + (n_saved, self.W, self.D)
        if out is None:
            import torch
            dev = torch.device("cuda", self.cfg.device if self.cfg.device >= 0 else torch.cuda.current_device())
            out = torch.empty(shape, dtype=_torch_dtype(self.dtype), device=dev)
        if _is_tensor(out):
            if tuple(out.shape) != shape or out.dtype != _torch_dtype(self.dtype) or not out.is_cuda or not out.is_contiguous():
                raise ValueError("out must be a contiguous device tensor of shape %s and dtype %s" % (shape, _torch_dtype(self.dtype)))
            if self.cfg.device >= 0 and out.device.index != self.cfg.device:
                raise ValueError("out is on device %d, the handle on device %d" % (out.device.index, self.cfg.device))
            _after_torch(out)
            return out.data_ptr(), out
        ptr, nbytes = out
        need = int(np.prod(shape)) * np.dtype(self.np_t).itemsize
        if nbytes < need:
            raise ValueError("out holds %d bytes, the run stores %d" % (nbytes, need))
        return int(ptr), out

    def run_device(self, n_saved, interval=1, out=None, want_accepted=True):
        """run() with the stored steps left in device memory (mcmcpp_hip_run_device).  Returns (chain, acc): chain a torch
        tensor (n_saved, W, D) -- (K, n_saved, W, D) with several chains -- on the handle's device, acc the per-step accepted
        counts as numpy (None unless want_accepted).  out: a contiguous device tensor of that shape and dtype to store into,
        or, for callers without torch, an (integer device address, nbytes) pair, which is then returned as it is."""
        ptr, chain = self._device_out(n_saved, out)
        lead = (self.K,) if self.K > 1 else ()
        acc = np.zeros(lead + (n_saved * interval,), dtype=np.uint32) if want_accepted else None
        self._check(lib().mcmcpp_hip_run_device(self.h, n_saved, interval, C.c_void_p(ptr), _ptr(acc)))
        return chain, acc

    def run_device_async(self, n_saved, interval=1, out=None, want_accepted=False):
        """Start run_device on the handle's worker thread; wait_stored(c) returns when the first c stored steps of every chain
        are complete in the returned device tensor, run_wait when the run is over."""
        ptr, chain = self._device_out(n_saved, out)
        lead = (self.K,) if self.K > 1 else ()
        acc = np.zeros(lead + (n_saved * interval,), dtype=np.uint32) if want_accepted else None
        self._async_keep = (chain, acc)
        self._check(lib().mcmcpp_hip_run_device_async(self.h, n_saved, interval, C.c_void_p(ptr), _ptr(acc)))
        return chain, acc

    def calc_logp_device(self, x, chain=0):
        """Log-posteriors of the rows of the device tensor x (..., D), e.g. of a chain run_device wrote, as a device tensor
        (...,): no host copies (mcmcpp_hip_calc_logp_device; an x that is not contiguous is made so on the device first).
        chain=k: with chain k's parameters.  A batch target -- C callback or torch log_prob -- is called on the rows
        themselves, in chunks of at most W/2."""
        import torch
        if not _is_tensor(x) or x.dim() < 1 or x.shape[-1] != self.D or x.dtype != _torch_dtype(self.dtype) or not x.is_cuda:
            raise ValueError("x must be a device tensor (..., %d) of dtype %s" % (self.D, _torch_dtype(self.dtype)))
        rows = x.contiguous().view(-1, self.D)
        out = torch.empty((rows.shape[0],), dtype=rows.dtype, device=rows.device)
        _after_torch(rows)  # (x's producer, the copy behind contiguous(), the last user of out's block)
        if self._torch_stream is not None:
            self._foreign = (rows, out)
        try:
            self._check(lib().mcmcpp_hip_calc_logp_device(self.h, chain, C.c_void_p(rows.data_ptr()), rows.shape[0], C.c_void_p(out.data_ptr())))
        finally:
            if self._torch_stream is not None:
                self._foreign = None
        return out.view(x.shape[:-1])

    def wait_stored(self, count):
        self._check(lib().mcmcpp_hip_wait_stored(self.h, count))

    def run_wait(self):
        self._check(lib().mcmcpp_hip_run_wait(self.h))

    def get_state(self):
        lead = (self.K,) if self.K > 1 else ()
        pos = np.empty(lead + (self.W, self.D), dtype=self.np_t)
        logp = np.empty(lead + (self.W,), dtype=self.np_t)
        nacc = np.empty(lead + (self.W,), dtype=np.uint32)
        self._check(lib().mcmcpp_hip_get_state(self.h, _ptr(pos), _ptr(logp), _ptr(nacc)))
        return pos, logp, nacc

    def reset_counters(self):
        self._check(lib().mcmcpp_hip_reset_counters(self.h))

    def counters(self):
        v = [C.c_uint64(0) for _ in range(4)]
        self._check(lib().mcmcpp_hip_get_counters(self.h, *[C.byref(x) for x in v]))
        return dict(accepted=v[0].value, ensemble_steps=v[1].value, near_ties=v[2].value, redraws=v[3].value)

    def set_chain_params(self, chain, params):
        """Chain `chain`'s own calculator parameters from the next run / calc_logp on (stored log-posteriors are not
        recomputed: calc_logp(pos, chain) and set_state do that)."""
        p = np.ascontiguousarray(params, dtype=self.np_t).ravel()
        self._check(lib().mcmcpp_hip_set_chain_params(self.h, chain, _ptr(p), p.size))

    def calc_logp(self, pos, chain=None):
        """Log-posteriors of the rows of pos; chain=k: with chain k's parameters (None: the handle's own, i.e. chain 0's)."""
        pos = np.ascontiguousarray(pos, dtype=self.np_t).reshape(-1, self.D)
        out = np.empty(pos.shape[0], dtype=self.np_t)
        if chain is None:
            self._check(lib().mcmcpp_hip_calc_logp(self.h, _ptr(pos), pos.shape[0], _ptr(out)))
        else:
            self._check(lib().mcmcpp_hip_calc_logp_chain(self.h, chain, _ptr(pos), pos.shape[0], _ptr(out)))
        return out

    def exchange_chains(self, round):
        """One replica-exchange round among the K chains (mcmcpp_hip_exchange_chains): round r proposes to swap walker w of
        chain k with walker w of chain k + 1 for every k = r (mod 2).  Returns dict(proposed, accepted, near_ties), numpy
        [K-1]: the counters of pair (k, k + 1), 0 for the pairs that are not in this round."""
        v = [np.zeros(max(self.K - 1, 1), dtype=np.uint64) for _ in range(3)]
        self._check(lib().mcmcpp_hip_exchange_chains(self.h, round, *[_ptr(x) for x in v]))
        return dict(proposed=v[0][:self.K - 1], accepted=v[1][:self.K - 1], near_ties=v[2][:self.K - 1])

    def run_exchanging(self, n_saved, interval=1, exchange_every=1, first_round=0, out=None, device=False):
        """Parallel tempering: n_saved stored steps (one every `interval` ensemble steps) with a replica-exchange round after
        every `exchange_every` ensemble steps (a multiple of interval), rounds numbered first_round, first_round + 1, ...
        A loop of run (device=True: run_device) segments, each followed by exchange_chains; a tail shorter than
        exchange_every runs without a trailing exchange.  Returns (chain [K][n_saved][W][D] -- a device tensor with
        device=True --, accepted per step [K][n_saved * interval], the summed swap counters as exchange_chains returns
        them, the next round number).  out: the array (device: tensor) to store into.

        Each segment costs a synchronisation (the exchange works on the state between runs, the segment's stored steps are
        copied to their place): choose exchange_every with that in mind."""
        if self.K < 2:
            raise ValueError("run_exchanging needs num_chains >= 2")
        if interval < 1 or exchange_every < 1 or exchange_every % interval:
            raise ValueError("exchange_every must be a positive multiple of interval")
        K, per = self.K, exchange_every // interval
        shape = (K, n_saved, self.W, self.D)
        if device:
            _, chain = self._device_out(n_saved, out)
            if not _is_tensor(chain):
                raise ValueError("run_exchanging(device=True) stores into a torch tensor")
        else:
            if out is not None:
                assert out.shape == shape and out.dtype == self.np_t and out.flags.c_contiguous
            chain = out if out is not None else np.empty(shape, dtype=self.np_t)
        acc = np.zeros((K, n_saved * interval), dtype=np.uint32)
        swaps = dict(proposed=np.zeros(K - 1, np.uint64), accepted=np.zeros(K - 1, np.uint64), near_ties=np.zeros(K - 1, np.uint64))
        rnd, done = first_round, 0
        while done < n_saved:
            seg = min(per, n_saved - done)
            c, a = (self.run_device if device else self.run)(seg, interval=interval)
            chain[:, done:done + seg] = c
            acc[:, done * interval:(done + seg) * interval] = a
            done += seg
            if seg == per:
                r = self.exchange_chains(rnd)
                for key in swaps:
                    swaps[key] += r[key]
                rnd += 1
        if device:
            import torch
            torch.cuda.current_stream(chain.device).synchronize()  # (the copies into `chain` are the caller's to rely on)
        return chain, acc, swaps, rnd

    def run_tempered(self, n_saved, interval=1, exchange_every=1, first_round=0, out=None, device=False):
        """run_exchanging in one call (mcmcpp_hip_run_tempered; device=True: mcmcpp_hip_run_tempered_device): the rounds lie
        inside the run's launch sequence, two launches each, with no synchronisation and no copy between the segments.
        exchange_every counts ensemble steps and need not be a multiple of interval.  Returns what run_exchanging returns,
        bit for bit.  out: the array -- pageable or pinned_empty -- (device: tensor, or (address, nbytes)) to store into."""
        K = self.K
        acc = np.zeros((K, n_saved * interval), dtype=np.uint32)
        v = [np.zeros(max(K - 1, 1), dtype=np.uint64) for _ in range(3)]
        rounds = C.c_uint64(0)
        if device:
            ptr, chain = self._device_out(n_saved, out)
            fn, dst = lib().mcmcpp_hip_run_tempered_device, C.c_void_p(ptr)
        else:
            shape = (K, n_saved, self.W, self.D)
            if out is not None:
                assert out.shape == shape and out.dtype == self.np_t and out.flags.c_contiguous
            chain = out if out is not None else np.empty(shape, dtype=self.np_t)
            fn, dst = lib().mcmcpp_hip_run_tempered, _ptr(chain)
        self._check(fn(self.h, n_saved, interval, exchange_every, first_round, dst, _ptr(acc), *[_ptr(x) for x in v], C.byref(rounds)))
        swaps = dict(proposed=v[0][:K - 1], accepted=v[1][:K - 1], near_ties=v[2][:K - 1])
        return chain, acc, swaps, first_round + rounds.value

    def _evidence_call(self, host_fn, device_fn, steps, slice_interval, chain_stride_steps, outputs):
        """the steps of evidence_ratios, evidence_bridge and evidence_mbar, checked, through the host-pointer or the device entry point"""
        K = self.K
        if _is_tensor(steps):
            if steps.dim() != 4 or tuple(steps.shape[0:1] + steps.shape[2:]) != (K, self.W, self.D):
                raise ValueError("device steps must have shape (%d, n, %d, %d), not %s" % (K, self.W, self.D, tuple(steps.shape)))
            if steps.dtype != _torch_dtype(self.dtype) or not steps.is_cuda:
                raise ValueError("device steps must be a device tensor of dtype %s" % _torch_dtype(self.dtype))
            E = self.W * self.D
            if not steps[0].is_contiguous() or (K > 1 and steps.stride(0) % E):
                raise ValueError("every chain of the device steps must be contiguous, and the chains a whole number of steps apart")
            stride = steps.stride(0) // E if chain_stride_steps is None else chain_stride_steps
            _after_torch(steps)
            self._check(device_fn(self.h, C.c_void_p(steps.data_ptr()), stride, steps.shape[1], slice_interval, *outputs))
        else:
            x = np.asarray(steps)
            if x.ndim != 4 or x.shape[0] != K or x.shape[2:] != (self.W, self.D) or x.dtype != self.np_t:
                raise ValueError("steps must be a %s array (%d, n, %d, %d)" % (np.dtype(self.np_t).name, K, self.W, self.D))
            n = x.shape[1]
            rows = [np.ascontiguousarray(x[k, s]) for k in range(K) for s in range(n)]  # (a contiguous step is not copied)
            ptrs = (C.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])
            self._check(host_fn(self.h, ptrs, n, slice_interval, *outputs))

    def evidence_ratios(self, steps, slice_interval=1, chain_stride_steps=None):
        """The ratios of normalising constants between neighbouring chains of a ladder, from stored steps of the K chains
        (mcmcpp_hip_evidence_ratios): steps a numpy array [K][n][W][D], or the device tensor run_tempered(device=True) returned
        (a view chain[:, burn:] of it likewise), which is read in place (mcmcpp_hip_evidence_ratios_device; chain_stride_steps:
        the steps between two chains, by default the tensor's own stride).  Every slice_interval-th step is used.  Returns a
        dict of numpy arrays: log_ratio, mcse, ess, kish, max_u [2][K-1] float64 and nonfinite [2][K-1] int64 -- row 0 the
        stepping-stone direction (draws of the flatter rung), row 1 the reverse; both estimate log(Z_p / Z_{p+1}) --,
        log_ratio_total and mcse_total [2], and num_draws.  The chain of ratios is an evidence only when the top rung is a
        normalised density."""
        K, P = self.K, max(self.K - 1, 1)
        out = {key: np.full((2, P), np.nan) for key in ("log_ratio", "mcse", "ess", "kish", "max_u")}
        out["nonfinite"] = np.zeros((2, P), np.int64)
        out["log_ratio_total"], out["mcse_total"] = np.full(2, np.nan), np.full(2, np.nan)
        draws = C.c_int64(0)
        outputs = [_ptr(out[key]) for key in ("log_ratio", "mcse", "ess", "kish", "max_u", "nonfinite", "log_ratio_total", "mcse_total")] + [C.byref(draws)]
        self._evidence_call(lib().mcmcpp_hip_evidence_ratios, lib().mcmcpp_hip_evidence_ratios_device, steps, slice_interval, chain_stride_steps, outputs)
        for key in ("log_ratio", "mcse", "ess", "kish", "max_u", "nonfinite"):
            out[key] = out[key][:, :K - 1]
        out["num_draws"] = draws.value
        return out

    def evidence_bridge(self, steps, slice_interval=1, chain_stride_steps=None):
        """The bridge estimate (Bennett's acceptance ratio) of the same ratios, one per pair from the draws of both rungs
        (mcmcpp_hip_evidence_bridge; steps, slice_interval and chain_stride_steps as for evidence_ratios).  Returns a dict of
        numpy arrays: log_ratio, mcse, overlap [K-1] float64, passes, converged [K-1] int64, ess [2][K-1] float64 and nonfinite
        [2][K-1] int64 (row d: the draws of rung p + 1 for d = 0, of rung p for d = 1), the floats log_ratio_total and mcse_total,
        and num_draws."""
        K, P = self.K, max(self.K - 1, 1)
        out = {key: np.full(P, np.nan) for key in ("log_ratio", "mcse", "overlap")}
        out["ess"] = np.full((2, P), np.nan)
        out["passes"], out["converged"], out["nonfinite"] = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros((2, P), np.int64)
        totals = np.full(2, np.nan)
        draws = C.c_int64(0)
        outputs = [_ptr(out[key]) for key in ("log_ratio", "mcse", "overlap", "ess", "passes", "converged", "nonfinite")]
        outputs += [C.c_void_p(totals.ctypes.data), C.c_void_p(totals.ctypes.data + 8), C.byref(draws)]
        self._evidence_call(lib().mcmcpp_hip_evidence_bridge, lib().mcmcpp_hip_evidence_bridge_device, steps, slice_interval, chain_stride_steps, outputs)
        for key in ("log_ratio", "mcse", "overlap", "passes", "converged"):
            out[key] = out[key][:K - 1]
        for key in ("ess", "nonfinite"):
            out[key] = out[key][:, :K - 1]
        out["log_ratio_total"], out["mcse_total"] = np.float64(totals[0]), np.float64(totals[1])
        out["num_draws"] = draws.value
        return out

    def evidence_mbar(self, steps, slice_interval=1, chain_stride_steps=None):
        """All K log-normalising constants of the ladder in one joint solve from every draw of every rung (the multistate Bennett
        acceptance ratio, mcmcpp_hip_evidence_mbar; steps, slice_interval and chain_stride_steps as for evidence_ratios).  Returns
        a dict of numpy arrays: log_z [K] (log(Z_k / Z_{K-1})), cov [K][K], log_ratio and mcse [K-1] (log(Z_p / Z_{p+1}) and its
        standard error from cov), ess [K], nonfinite [K][K] int64 (row r: the draws of rung r, column k: under chain k), the floats
        log_ratio_total = log_z[0] and mcse_total = sqrt(cov[0][0]), and passes, converged, num_draws."""
        K = self.K
        out = dict(log_z=np.full(K, np.nan), cov=np.full((K, K), np.nan), log_ratio=np.full(max(K - 1, 1), np.nan), mcse=np.full(max(K - 1, 1), np.nan),
                   ess=np.full(K, np.nan), nonfinite=np.zeros((K, K), np.int64))
        totals = np.full(2, np.nan)
        counts = np.zeros(3, np.int64)  # passes, converged, num_draws
        outputs = [_ptr(out[key]) for key in ("log_z", "cov", "log_ratio", "mcse", "ess", "nonfinite")]
        outputs += [C.c_void_p(totals.ctypes.data), C.c_void_p(totals.ctypes.data + 8)] + [C.c_void_p(counts.ctypes.data + 8 * i) for i in range(3)]
        self._evidence_call(lib().mcmcpp_hip_evidence_mbar, lib().mcmcpp_hip_evidence_mbar_device, steps, slice_interval, chain_stride_steps, outputs)
        for key in ("log_ratio", "mcse"):
            out[key] = out[key][:K - 1]
        out["log_ratio_total"], out["mcse_total"] = np.float64(totals[0]), np.float64(totals[1])
        out["passes"], out["converged"], out["num_draws"] = np.int64(counts[0]), np.int64(counts[1]), int(counts[2])
        return out

    def evidence_gaussian(self, steps, chain=0, mean=None, chol=None, fit_fraction=0.5, slice_interval=1, seed=0, stream=0, want_proposals=False):
        """The log-evidence of chain `chain`'s target from stored steps of that chain, by the bridge estimate between the target
        and a Gaussian N(mean, chol chol^T) (mcmcpp_hip_evidence_gaussian): no ladder is needed.  steps: a numpy array [n][W][D],
        or a device tensor of that shape (run_device's, or a view behind a burn-in), read in place
        (mcmcpp_hip_evidence_gaussian_device).  Every slice_interval-th step is used.  With mean and chol given, all used steps are
        bridged against as many proposals from pcg64(seed, stream).  With both omitted, the Gaussian is fitted to the first
        fit_fraction of the used steps (HipMoments' mean and covariance, numpy's Cholesky factor) and the rest are bridged.
        Returns a dict: log_evidence, mcse, overlap (floats), ess [2], nonfinite [2] (index 0: the proposals, 1: the draws), passes,
        converged, num_draws, log_q [2][N], the mean and chol used and, with want_proposals, proposals [N][D]."""
        if (mean is None) != (chol is None):
            raise ValueError("mean and chol go together")
        tensor = _is_tensor(steps)
        if not tensor:
            steps = np.asarray(steps)
            if steps.ndim != 3 or steps.shape[1:] != (self.W, self.D) or steps.dtype != self.np_t:
                raise ValueError("steps must be a %s array (n, %d, %d)" % (np.dtype(self.np_t).name, self.W, self.D))
        if mean is None:
            used = (steps.shape[0] + slice_interval - 1) // slice_interval
            head = int(used * fit_fraction) * slice_interval  # the steps the fit takes; the bridge starts behind them
            if head < 1 or head >= steps.shape[0]:
                raise ValueError("fit_fraction %r leaves no steps to fit on, or none to bridge on" % (fit_fraction,))
            m = HipMoments(self.W, self.D, self.dtype, self.cfg.device)
            try:
                (m.add_device_steps if tensor else m.add_steps)(steps[:head], slice_interval=slice_interval)
                _, mean, cov, _ = m.finish()
            finally:
                m.close()
            chol = np.linalg.cholesky(cov.astype(np.float64))
            steps = steps[head:]
        mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        chol = np.ascontiguousarray(chol, dtype=np.float64)
        if mean.shape != (self.D,) or chol.shape != (self.D, self.D):
            raise ValueError("mean must have shape (%d,) and chol (%d, %d)" % (self.D, self.D, self.D))
        n = int(steps.shape[0])
        N = max((n + slice_interval - 1) // slice_interval, 0) * self.W
        figures = np.full(3, np.nan)
        ess, counts, nonfinite = np.full(2, np.nan), np.zeros(3, np.int64), np.zeros(2, np.int64)
        log_q = np.full((2, N), np.nan)
        proposals = np.zeros((N, self.D), self.np_t) if want_proposals else None
        tail = [_ptr(mean), _ptr(chol), C.c_uint64(seed), C.c_uint64(stream)] + [C.c_void_p(figures.ctypes.data + 8 * j) for j in range(3)] + [_ptr(ess)]
        tail += [C.c_void_p(counts.ctypes.data), C.c_void_p(counts.ctypes.data + 8), _ptr(nonfinite), C.c_void_p(counts.ctypes.data + 16), _ptr(proposals), _ptr(log_q)]
        if tensor:
            ptr, n = _device_steps(steps, None, self.W, self.D, self.dtype, self.cfg.device)
            self._check(lib().mcmcpp_hip_evidence_gaussian_device(self.h, chain, C.c_void_p(ptr), n, slice_interval, *tail))
        else:
            rows = [np.ascontiguousarray(steps[s]) for s in range(n)]  # (a contiguous step is not copied)
            ptrs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in rows])
            self._check(lib().mcmcpp_hip_evidence_gaussian(self.h, chain, ptrs, n, slice_interval, *tail))
        out = dict(log_evidence=np.float64(figures[0]), mcse=np.float64(figures[1]), overlap=np.float64(figures[2]), ess=ess, passes=np.int64(counts[0]),
                   converged=np.int64(counts[1]), nonfinite=nonfinite, num_draws=int(counts[2]), log_q=log_q, mean=mean, chol=chol)
        if want_proposals:
            out["proposals"] = proposals
        return out

    def last_run_timing(self):
        ms, n = C.c_double(0), C.c_int64(0)
        self._check(lib().mcmcpp_hip_last_run_timing(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_run_host_timing(self):
        """(ms the host spent enqueueing, wall ms of the call, GPU us of one step's exchange -- split ensembles only)"""
        v = [C.c_double(0) for _ in range(3)]
        self._check(lib().mcmcpp_hip_last_run_host_timing(self.h, *[C.byref(x) for x in v]))
        return v[0].value, v[1].value, v[2].value

    def last_run_exchange(self):
        """Split ensembles: (bytes this rank received per ensemble step, chunks repeated with larger blocks, slots per block)"""
        b, r, c = C.c_double(0), C.c_int64(0), C.c_int64(0)
        self._check(lib().mcmcpp_hip_last_run_exchange(self.h, C.byref(b), C.byref(r), C.byref(c)))
        return b.value, r.value, c.value

    def half_step_async(self, color, save_slot=-1):
        self._check(lib().mcmcpp_hip_half_step_async(self.h, color, save_slot))

    def bind_device_chain(self, ptr, slots):
        self._check(lib().mcmcpp_hip_bind_device_chain(self.h, ptr, slots))

    def device_positions(self):
        return lib().mcmcpp_hip_device_positions(self.h)

    def shard_span(self, color):
        off, cnt = C.c_int64(0), C.c_int64(0)
        self._check(lib().mcmcpp_hip_shard_span(self.h, color, C.byref(off), C.byref(cnt)))
        return off.value, cnt.value

    def synchronize(self):
        self._check(lib().mcmcpp_hip_synchronize(self.h))


class HipMoments:
    """Device-side Analysis::CovarianceMatrix (include/mcmcpp_hip.h, mcmcpp_hip_moments_*)."""

    def __init__(self, num_walkers, num_params, dtype=F64, device=-1):
        self.W, self.D, self.dtype, self.device = num_walkers, num_params, dtype, device
        self.h = C.c_void_p()
        rc = lib().mcmcpp_hip_moments_create(dtype, device, num_walkers, num_params, C.byref(self.h))
        if rc != OK:
            raise HipError(rc, (lib().mcmcpp_hip_moments_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != OK:
            raise HipError(rc, (lib().mcmcpp_hip_moments_last_error(self.h) or b"").decode())

    def add_steps(self, steps, slice_interval=1):
        """steps[(n, W, D)] (C-contiguous); every slice_interval-th step is used, starting with the first."""
        steps = np.ascontiguousarray(steps, dtype=np_dtype(self.dtype))
        assert steps.ndim == 3 and steps.shape[1:] == (self.W, self.D)
        used = (steps.shape[0] + slice_interval - 1) // slice_interval
        self._check(lib().mcmcpp_hip_moments_add_steps(self.h, _ptr(steps), used, slice_interval))

    def add_device_steps(self, steps, n_steps=None, slice_interval=1):
        """Stored steps in device memory: a contiguous device tensor (n, W, D), or an integer address (e.g.
        torch.Tensor.data_ptr()) of n_steps contiguous steps.  Every slice_interval-th step is used, starting with the first."""
        ptr, n = _device_steps(steps, n_steps, self.W, self.D, self.dtype, self.device)
        if slice_interval == 1:
            self._check(lib().mcmcpp_hip_moments_add_device_steps(self.h, C.c_void_p(ptr), n))
        else:
            used = (n + slice_interval - 1) // slice_interval
            self._check(lib().mcmcpp_hip_moments_add_device_steps_strided(self.h, C.c_void_p(ptr), used, slice_interval))

    def finish(self):
        t = np_dtype(self.dtype)
        mean, cov, corr = np.zeros(self.D, t), np.zeros((self.D, self.D), t), np.zeros((self.D, self.D), t)
        n = C.c_int64(0)
        self._check(lib().mcmcpp_hip_moments_finish(self.h, C.byref(n), _ptr(mean), _ptr(cov), _ptr(corr)))
        return n.value, mean, cov, corr

    def reset(self):
        self._check(lib().mcmcpp_hip_moments_reset(self.h))

    def close(self):
        if self.h:
            lib().mcmcpp_hip_moments_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipHistograms:
    """Device-side Analysis::CornerHistograms / PercentileAndMaximumFinder (include/mcmcpp_hip.h, mcmcpp_hip_histograms_*)."""

    def __init__(self, num_walkers, num_params, bins, with_pairs=True, dtype=F64, device=-1):
        self.W, self.P, self.bins, self.with_pairs, self.dtype, self.device = num_walkers, num_params, bins, bool(with_pairs), dtype, device
        self.h = C.c_void_p()
        rc = lib().mcmcpp_hip_histograms_create(dtype, device, num_walkers, num_params, bins, 1 if with_pairs else 0, C.byref(self.h))
        if rc != OK:
            self.h = C.c_void_p()
            raise HipError(rc, (lib().mcmcpp_hip_histograms_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != OK:
            raise HipError(rc, (lib().mcmcpp_hip_histograms_last_error(self.h) or b"").decode())

    def compute(self, steps, slice_interval=1):
        """steps: array [(n, W, P)] or a sequence of arrays [(W, P)]; every slice_interval-th step is used, starting with the first."""
        if isinstance(steps, np.ndarray):
            steps = np.ascontiguousarray(steps, dtype=np_dtype(self.dtype))
            assert steps.ndim == 3 and steps.shape[1:] == (self.W, self.P)
            blocks = [steps[k] for k in range(0, steps.shape[0], slice_interval)]
        else:
            blocks = [np.ascontiguousarray(b, dtype=np_dtype(self.dtype)) for b in list(steps)[::slice_interval]]
            assert all(b.shape == (self.W, self.P) for b in blocks)
        ptrs = (C.c_void_p * max(1, len(blocks)))(*[b.ctypes.data for b in blocks])
        self._keep = blocks
        self._check(lib().mcmcpp_hip_histograms_compute(self.h, ptrs, len(blocks)))

    def compute_device(self, steps, n_steps=None, slice_interval=1):
        """Stored steps in device memory: a contiguous device tensor (n, W, P), or an integer address (e.g.
        torch.Tensor.data_ptr()) of n_steps contiguous steps."""
        ptr, n = _device_steps(steps, n_steps, self.W, self.P, self.dtype, self.device)
        self._check(lib().mcmcpp_hip_histograms_compute_device(self.h, C.c_void_p(ptr), n, slice_interval))

    def result(self, want_pairs=None):
        """(num_points, bounds[(P, 2)] in the chain's type, single[(P, bins)], pairs[(P(P-1)/2, bins, bins)] or None, clamped[P])"""
        want_pairs = self.with_pairs if want_pairs is None else want_pairs
        n = C.c_int64(0)
        bounds = np.zeros((self.P, 2), np_dtype(self.dtype))
        single = np.zeros((self.P, self.bins), np.int64)
        pairs = np.zeros((self.P * (self.P - 1) // 2, self.bins, self.bins), np.int64) if want_pairs else None
        clamped = np.zeros(self.P, np.int64)
        self._check(lib().mcmcpp_hip_histograms_result(self.h, C.byref(n), _ptr(bounds), _ptr(single), _ptr(pairs), _ptr(clamped)))
        return n.value, bounds, single, pairs, clamped

    def close(self):
        if self.h:
            lib().mcmcpp_hip_histograms_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def autocorr_times(steps, walkers_to_use=0, window_scaling=4, want_functions=False, dtype=None, device=-1):
    """Device-side Analysis::AutoCorrCalc::calcAutoCorrTimes (include/mcmcpp_hip.h, mcmcpp_hip_autocorr_times).

    steps: array [(n, W, D)] or a sequence of n arrays [(W, D)] (stored steps, oldest first).  Returns times[D], or
    (times, functions[(D, n)]) with want_functions."""
    if isinstance(steps, np.ndarray):
        if dtype is None:
            dtype = F32 if steps.dtype == np.float32 else F64
        steps = np.ascontiguousarray(steps, dtype=np_dtype(dtype))
        assert steps.ndim == 3
        blocks = [steps[i] for i in range(steps.shape[0])]
    else:
        if dtype is None:
            dtype = F32 if np.asarray(steps[0]).dtype == np.float32 else F64
        blocks = [np.ascontiguousarray(b, dtype=np_dtype(dtype)) for b in steps]
    n = len(blocks)
    W, D = blocks[0].shape
    assert all(b.shape == (W, D) for b in blocks)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in blocks])
    t = np_dtype(dtype)
    times = np.zeros(D, t)
    functions = np.zeros((D, n), t) if want_functions else None
    rc = lib().mcmcpp_hip_autocorr_times(dtype, device, ptrs, n, W, D, walkers_to_use, window_scaling, _ptr(times), _ptr(functions))
    if rc != OK:
        raise HipError(rc, (lib().mcmcpp_hip_autocorr_last_error() or b"").decode())
    return (times, functions) if want_functions else times


def autocorr_times_device(steps, n_steps=None, W=None, D=None, dtype=None, walkers_to_use=0, window_scaling=4, device=-1):
    """The same for stored steps in device memory: a contiguous device tensor (n, W, D) -- shape, dtype and device are the
    tensor's, and are checked against W, D, dtype and device where those are given -- or an integer address (e.g.
    torch.Tensor.data_ptr()) of n_steps contiguous steps of W x D elements (dtype: F64 unless given)."""
    if _is_tensor(steps):
        import torch
        if steps.dim() != 3 or steps.dtype not in (torch.float64, torch.float32):
            raise ValueError("device steps must be a float64 or float32 tensor (n, W, D)")
        tensor_dtype = F64 if steps.dtype == torch.float64 else F32
        if dtype is not None and dtype != tensor_dtype:
            raise ValueError("device steps are %s, not the dtype asked for" % steps.dtype)
        dtype = tensor_dtype
        W, D = (steps.shape[1] if W is None else W), (steps.shape[2] if D is None else D)
        if device < 0 and steps.is_cuda:
            device = steps.device.index
    elif W is None or D is None:
        raise ValueError("an integer device address needs n_steps, W and D")
    dtype = F64 if dtype is None else dtype
    device_ptr, n_steps = _device_steps(steps, n_steps, W, D, dtype, device)
    times = np.zeros(D, np_dtype(dtype))
    rc = lib().mcmcpp_hip_autocorr_times_device(dtype, device, C.c_void_p(device_ptr), n_steps, W, D, walkers_to_use, window_scaling, _ptr(times), None)
    if rc != OK:
        raise HipError(rc, (lib().mcmcpp_hip_autocorr_last_error() or b"").decode())
    return times


def _quantile_source(steps, slice_interval, dtype, device):
    """What order_statistics and rank_counts hand the library: (dtype, device, W, P, N, call), where call(host_fn, device_fn,
    *rest) runs the entry point that fits `steps` -- a numpy array [(n, W, P)] (host path: the pointers of every
    slice_interval-th step) or a contiguous device tensor (n, W, P) (device path: read where it lies, no copy)."""
    if slice_interval < 1:
        raise ValueError("slice_interval must be at least 1")
    if _is_tensor(steps):
        import torch
        if steps.dim() != 3 or steps.dtype not in (torch.float64, torch.float32):
            raise ValueError("device steps must be a float64 or float32 tensor (n, W, P)")
        tensor_dtype = F64 if steps.dtype == torch.float64 else F32
        if dtype is not None and dtype != tensor_dtype:
            raise ValueError("device steps are %s, not the dtype asked for" % steps.dtype)
        n, W, P = (int(v) for v in steps.shape)
        if device < 0 and steps.is_cuda:
            device = steps.device.index
        ptr, n = _device_steps(steps, None, W, P, tensor_dtype, device)

        def call(host_fn, device_fn, *rest):
            return device_fn(tensor_dtype, device, C.c_void_p(ptr), n, slice_interval, W, P, *rest)
        return tensor_dtype, W, P, ((n + slice_interval - 1) // slice_interval) * W, call
    steps = np.asarray(steps)
    if dtype is None:
        dtype = F32 if steps.dtype == np.float32 else F64
    if steps.ndim != 3:
        raise ValueError("steps must have shape (n, W, P), not %s" % (steps.shape,))
    n, W, P = steps.shape
    # (a step that is not contiguous by itself is copied; the steps need not lie one behind the other)
    blocks = [np.ascontiguousarray(steps[k], dtype=np_dtype(dtype)) for k in range(0, n, slice_interval)]
    ptrs = (C.c_void_p * max(1, len(blocks)))(*[b.ctypes.data for b in blocks])

    def call(host_fn, device_fn, *rest):
        return host_fn(dtype, device, ptrs, len(blocks), W, P, *rest)
    return dtype, W, P, len(blocks) * W, call


def _quantile_check(rc):
    if rc != OK:
        raise HipError(rc, (lib().mcmcpp_hip_order_statistics_last_error() or b"").decode())


def order_statistics(steps, ranks, slice_interval=1, dtype=None, device=-1):
    """Exact order statistics of every parameter over stored steps (include/mcmcpp_hip.h, mcmcpp_hip_order_statistics): values[(P,
    len(ranks))], values[p][k] the sample of parameter p with 0-based rank ranks[k] among the N = (steps used) x W samples of p,
    in the order -inf < ... < -0 < +0 < ... < +inf.  steps: a numpy array [(n, W, P)], or a contiguous torch tensor (n, W, P)
    on the GPU, which is read where it lies.  Every slice_interval-th step is used, starting with the first."""
    dtype, W, P, N, call = _quantile_source(steps, slice_interval, dtype, device)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
    values = np.zeros((P, ranks.size), np_dtype(dtype))
    _quantile_check(call(lib().mcmcpp_hip_order_statistics, lib().mcmcpp_hip_order_statistics_device, _ptr(ranks), ranks.size, _ptr(values)))
    return values


def rank_counts(steps, query, slice_interval=1, dtype=None, device=-1):
    """(below, not_above), both int64 [(P, n_query)]: the samples x of parameter p with x < query[p][q] and with x <= query[p][q],
    compared as numbers (-0 == +0), counted on the device (mcmcpp_hip_rank_counts).  steps as for order_statistics; query
    [(P, n_query)], or [(n_query,)] for every parameter alike."""
    dtype, W, P, N, call = _quantile_source(steps, slice_interval, dtype, device)
    query = np.asarray(query, dtype=np_dtype(dtype))
    if query.ndim == 1:
        query = np.broadcast_to(query, (P, query.size))
    if query.ndim != 2 or query.shape[0] != P:
        raise ValueError("query must have shape (%d, n_query), not %s" % (P, query.shape))
    query = np.ascontiguousarray(query)
    below, not_above = np.zeros(query.shape, np.int64), np.zeros(query.shape, np.int64)
    _quantile_check(call(lib().mcmcpp_hip_rank_counts, lib().mcmcpp_hip_rank_counts_device, _ptr(query), query.shape[1], _ptr(below), _ptr(not_above)))
    return below, not_above


def quantile_ranks(q, N):
    """(h, lo, hi) of the quantiles q in [0, 1] among N samples: h = q (N - 1) in float64, lo = floor(h), hi = ceil(h)"""
    q = np.asarray(q, dtype=np.float64).ravel()
    if N < 1 or not np.all((q >= 0) & (q <= 1)):
        raise ValueError("quantiles need at least one sample and 0 <= q <= 1")
    h = q * np.float64(N - 1)
    return h, np.floor(h).astype(np.int64), np.ceil(h).astype(np.int64)


def quantile_rule(x_lo, x_hi, h, method, np_t):
    """The value of a quantile from the order statistics of ranks floor(h) and ceil(h) ([(P, len(h))] each): "lower", "higher", or
    "linear" = x_lo + (x_hi - x_lo) (h - floor(h)) in float64, rounded once to np_t."""
    if method == "lower":
        return x_lo.astype(np_t)
    if method == "higher":
        return x_hi.astype(np_t)
    if method != "linear":
        raise ValueError('method must be "linear", "lower" or "higher"')
    lo, hi = x_lo.astype(np.float64), x_hi.astype(np.float64)
    with np.errstate(invalid="ignore"):
        mid = lo + (hi - lo) * (h - np.floor(h))
    return np.where(x_lo == x_hi, lo, mid).astype(np_t)  # (equal neighbours, infinite ones included, are the answer)


def quantiles(steps, q, method="linear", slice_interval=1, dtype=None, device=-1):
    """Exact quantiles q (in [0, 1]) of every parameter: [(P, len(q))], from the order statistics of ranks floor(h) and ceil(h),
    h = q (N - 1): see quantile_rule for the three methods."""
    if method not in ("linear", "lower", "higher"):
        raise ValueError('method must be "linear", "lower" or "higher"')
    dtype, W, P, N, _ = _quantile_source(steps, slice_interval, dtype, device)
    h, lo, hi = quantile_ranks(q, N)
    if not h.size:
        return np.zeros((P, 0), np_dtype(dtype))
    ranks, where = np.unique(np.concatenate([lo, hi]), return_inverse=True)  # (each rank is selected once)
    x = order_statistics(steps, ranks, slice_interval, dtype, device)
    return quantile_rule(x[:, where[:h.size]], x[:, where[h.size:]], h, method, np_dtype(dtype))


def _rhat_device_source(steps, chain_stride_steps, dtype, device):
    """(dtype, device, address, K, chain_stride_steps, n, W, P) of a device tensor (K, n, W, P) or (n, W, P): every chain
    contiguous, the chains a whole number of steps apart (a view such as chain[:, burn_in:] of a contiguous tensor is)"""
    import torch
    if steps.dim() not in (3, 4) or steps.dtype not in (torch.float64, torch.float32):
        raise ValueError("device steps must be a float64 or float32 tensor (K, n, W, P) or (n, W, P)")
    tensor_dtype = F64 if steps.dtype == torch.float64 else F32
    if dtype is not None and dtype != tensor_dtype:
        raise ValueError("device steps are %s, not the dtype asked for" % steps.dtype)
    if steps.dim() == 3:
        steps = steps[None]
    K, n, W, P = (int(v) for v in steps.shape)
    if not steps.is_cuda or not steps[0].is_contiguous():
        raise ValueError("device steps must lie in device memory, every chain contiguous")
    stride = int(steps.stride(0)) if K > 1 else n * W * P
    if stride % (W * P) or stride < n * W * P:
        raise ValueError("the chains of the device steps must be a whole number of steps apart, and not overlap")
    if chain_stride_steps is not None and K > 1 and chain_stride_steps != stride // (W * P):
        raise ValueError("chain_stride_steps = %d, but the tensor's chains are %d steps apart" % (chain_stride_steps, stride // (W * P)))
    if device >= 0 and steps.device.index != device:
        raise ValueError("device steps are on device %d, not on device %d" % (steps.device.index, device))
    _after_torch(steps)
    return tensor_dtype, steps.device.index, steps.data_ptr(), K, stride // (W * P), n, W, P


def _rhat_sources(steps, slice_interval, chain_stride_steps, dtype, device):
    """What gelman_rubin and effective_sample_size hand to the library: (on_device, dtype, device, source, K, chain stride, n,
    W, P, keep).  On the device `source` is the address and n counts stored steps; on the host it is the array of step
    pointers, sliced already, n counts used steps, and `keep` holds the arrays they point into."""
    if slice_interval < 1:
        raise ValueError("slice_interval must be at least 1")
    if _is_tensor(steps):
        dtype, device, ptr, K, stride, n, W, P = _rhat_device_source(steps, chain_stride_steps, dtype, device)
        return True, dtype, device, C.c_void_p(ptr), K, stride, n, W, P, steps
    if chain_stride_steps is not None:
        raise ValueError("chain_stride_steps belongs to steps in device memory")
    if isinstance(steps, np.ndarray):
        if steps.ndim not in (3, 4):
            raise ValueError("steps must have shape (K, n, W, P) or (n, W, P), not %s" % (steps.shape,))
        chains = [steps] if steps.ndim == 3 else list(steps)
    else:
        chains = [list(c) for c in steps]
    if not chains or any(len(c) != len(chains[0]) for c in chains):
        raise ValueError("every chain must hold the same number of steps")
    if dtype is None:
        dtype = F32 if len(chains[0]) and np.asarray(chains[0][0]).dtype == np.float32 else F64
    # (a step that is not contiguous by itself is copied; the steps need not lie one behind the other)
    blocks = [np.ascontiguousarray(c[s], dtype=np_dtype(dtype)) for c in chains for s in range(0, len(c), slice_interval)]
    K, n = len(chains), len(blocks) // len(chains)
    if not blocks or blocks[0].ndim != 2 or any(b.shape != blocks[0].shape for b in blocks):
        raise ValueError("every step must have the same shape (W, P)")
    W, P = blocks[0].shape
    ptrs = (C.c_void_p * len(blocks))(*[b.ctypes.data for b in blocks])
    return False, dtype, device, ptrs, K, 0, n, W, P, blocks


def gelman_rubin(steps, split=True, slice_interval=1, chain_stride_steps=None, dtype=None, device=-1, want_sequences=False):
    """The Gelman-Rubin split R-hat of every parameter, with the walkers of K chains as sequences (include/mcmcpp_hip.h,
    mcmcpp_hip_gelman_rubin: an extension).  steps: a numpy array [(K, n, W, P)] or [(n, W, P)] (one chain); a list of K lists of
    step arrays [(W, P)]; or a torch tensor of those shapes on the GPU, read where it lies (every chain contiguous: the view
    chain[:, burn_in:] of what run_device wrote qualifies, its chains chain_stride_steps apart).  Every slice_interval-th step
    of a chain is used, from its first.  Returns a dict: rhat, mean, within, between [(P,)], chain_mean, chain_within [(K, P)],
    sequence_length, num_sequences, and with want_sequences sequence_mean, sequence_m2 [(M, P)]; all float64."""
    on_device, dtype, device, source, K, stride, n, W, P, _keep = _rhat_sources(steps, slice_interval, chain_stride_steps, dtype, device)
    L_ = lib()

    def call(*outputs):
        if on_device:
            return L_.mcmcpp_hip_gelman_rubin_device(dtype, device, source, K, stride, n, slice_interval, W, P, int(bool(split)), *outputs)
        return L_.mcmcpp_hip_gelman_rubin(dtype, device, source, K, n, W, P, int(bool(split)), *outputs)
    used = (n + slice_interval - 1) // slice_interval if on_device else n
    M = K * (2 if split else 1) * W
    out = dict(rhat=np.zeros(P), mean=np.zeros(P), within=np.zeros(P), between=np.zeros(P), chain_mean=np.zeros((K, P)), chain_within=np.zeros((K, P)))
    if want_sequences:
        out.update(sequence_mean=np.zeros((M, P)), sequence_m2=np.zeros((M, P)))
    length, count = C.c_int64(0), C.c_int64(0)
    rc = call(*([_ptr(out[k]) for k in ("rhat", "mean", "within", "between", "chain_mean", "chain_within")] +
                [_ptr(out.get("sequence_mean")), _ptr(out.get("sequence_m2")), C.cast(C.byref(length), C.c_void_p), C.cast(C.byref(count), C.c_void_p)]))
    if rc != OK:
        raise HipError(rc, (L_.mcmcpp_hip_gelman_rubin_last_error() or b"").decode())
    assert count.value == M and length.value == (used // 2 if split else used)
    out.update(sequence_length=length.value, num_sequences=count.value)
    return out


def effective_sample_size(steps, split=True, max_lag=0, n_functions=0, slice_interval=1, chain_stride_steps=None, dtype=None, device=-1):
    """The effective sample size and integrated autocorrelation time of every parameter over the walkers of K chains
    (include/mcmcpp_hip.h, mcmcpp_hip_effective_sample_size: the multi-sequence estimator that goes with the split R-hat; an
    extension).  steps: as for gelman_rubin.  max_lag: 0, or the largest lag the window may reach.  n_functions: how many lags
    of rho and autocov to return.  Returns a dict: ess, tau (float64), lags_used, closed (int64) [(P,)]; rho, autocov
    [(P, n_functions)]; rhat, mean, within, between [(P,)]; sequence_length, num_sequences."""
    if max_lag < 0 or n_functions < 0:
        raise ValueError("max_lag and n_functions must not be negative")
    on_device, dtype, device, source, K, stride, n, W, P, _keep = _rhat_sources(steps, slice_interval, chain_stride_steps, dtype, device)
    L_ = lib()
    out = dict(ess=np.zeros(P), tau=np.zeros(P), lags_used=np.zeros(P, np.int64), closed=np.zeros(P, np.int64), rho=np.zeros((P, n_functions)),
               autocov=np.zeros((P, n_functions)), rhat=np.zeros(P), mean=np.zeros(P), within=np.zeros(P), between=np.zeros(P))
    length, count = C.c_int64(0), C.c_int64(0)
    outputs = [_ptr(a) if a.size else None for a in out.values()] + [C.cast(C.byref(length), C.c_void_p), C.cast(C.byref(count), C.c_void_p)]
    if on_device:
        rc = L_.mcmcpp_hip_effective_sample_size_device(dtype, device, source, K, stride, n, slice_interval, W, P, int(bool(split)), max_lag, n_functions, *outputs)
    else:
        rc = L_.mcmcpp_hip_effective_sample_size(dtype, device, source, K, n, W, P, int(bool(split)), max_lag, n_functions, *outputs)
    if rc != OK:
        raise HipError(rc, (L_.mcmcpp_hip_effective_sample_size_last_error() or b"").decode())
    out.update(sequence_length=length.value, num_sequences=count.value)
    return out


def _rank_check(rc):
    if rc != OK:
        raise HipError(rc, (lib().mcmcpp_hip_rank_diagnostics_last_error() or b"").decode())


def normal_scores(steps, split=True, fold=False, slice_interval=1, chain_stride_steps=None, dtype=None, device=-1):
    """The normal scores of the draws of every parameter (include/mcmcpp_hip.h, mcmcpp_hip_normal_scores: the rank-normalisation
    of Vehtari et al. 2021; an extension).  steps: as for gelman_rubin.  fold: rank |x - median| instead of x.  Returns a dict:
    scores, float64 [(K, H L, W, P)], the chain of the sequences' steps -- a numpy array for host steps, a torch tensor on the
    steps' device for device steps; median, q05, q95 [(P,)] float64; sequence_length, num_sequences."""
    on_device, dtype, device, source, K, stride, n, W, P, _keep = _rhat_sources(steps, slice_interval, chain_stride_steps, dtype, device)
    used = (n + slice_interval - 1) // slice_interval if on_device else n
    HL = used // 2 * 2 if split else used
    out = dict(median=np.zeros(P), q05=np.zeros(P), q95=np.zeros(P))
    length, count = C.c_int64(0), C.c_int64(0)
    tail = [_ptr(out[k]) for k in ("median", "q05", "q95")] + [C.cast(C.byref(length), C.c_void_p), C.cast(C.byref(count), C.c_void_p)]
    L_ = lib()
    if on_device:
        import torch
        scores = torch.empty((K, max(HL, 0), W, P), dtype=torch.float64, device=steps.device)
        _after_torch(scores)
        _rank_check(L_.mcmcpp_hip_normal_scores_device(dtype, device, source, K, stride, n, slice_interval, W, P, int(bool(split)), int(bool(fold)),
                                                       C.c_void_p(scores.data_ptr()), *tail))
    else:
        scores = np.zeros((K, max(HL, 0), W, P))
        _rank_check(L_.mcmcpp_hip_normal_scores(dtype, device, source, K, n, W, P, int(bool(split)), int(bool(fold)), _ptr(scores), *tail))
    out.update(scores=scores, sequence_length=length.value, num_sequences=count.value)
    return out


RANK_DIAGNOSTICS_KEYS = ("rhat", "rhat_rank", "rhat_folded", "ess_bulk", "ess_tail", "ess_tail_lower", "ess_tail_upper", "median", "q05", "q95",
                         "closed_bulk", "closed_tail")


def rank_diagnostics(steps, split=True, max_lag=0, slice_interval=1, chain_stride_steps=None, dtype=None, device=-1):
    """Rank-normalised split R-hat, bulk-ESS and tail-ESS of every parameter (include/mcmcpp_hip.h, mcmcpp_hip_rank_diagnostics;
    an extension).  steps: as for gelman_rubin.  Returns a dict: rhat, rhat_rank, rhat_folded, ess_bulk, ess_tail,
    ess_tail_lower, ess_tail_upper, median, q05, q95 (float64), closed_bulk, closed_tail (int64) [(P,)]; sequence_length,
    num_sequences."""
    if max_lag < 0:
        raise ValueError("max_lag must not be negative")
    on_device, dtype, device, source, K, stride, n, W, P, _keep = _rhat_sources(steps, slice_interval, chain_stride_steps, dtype, device)
    out = {k: np.zeros(P, np.int64 if k.startswith("closed") else np.float64) for k in RANK_DIAGNOSTICS_KEYS}
    length, count = C.c_int64(0), C.c_int64(0)
    outputs = [_ptr(a) for a in out.values()] + [C.cast(C.byref(length), C.c_void_p), C.cast(C.byref(count), C.c_void_p)]
    L_ = lib()
    if on_device:
        _rank_check(L_.mcmcpp_hip_rank_diagnostics_device(dtype, device, source, K, stride, n, slice_interval, W, P, int(bool(split)), max_lag, *outputs))
    else:
        _rank_check(L_.mcmcpp_hip_rank_diagnostics(dtype, device, source, K, n, W, P, int(bool(split)), max_lag, *outputs))
    out.update(sequence_length=length.value, num_sequences=count.value)
    return out


def beta_quantile(p, a, b):
    """The x with I_x(a, b) = p, by the library's host function (include/mcmcpp_hip.h, mcmcpp_hip_beta_quantile: specified to a
    relative accuracy of 1e-10).  Opens no device."""
    if not (0.0 < p < 1.0) or not (a >= 1.0 and b >= 1.0):
        raise ValueError("beta_quantile needs 0 < p < 1 and a, b >= 1")
    return float(lib().mcmcpp_hip_beta_quantile(float(p), float(a), float(b)))


POSTERIOR_SUMMARY_KEYS = ("mean", "sd", "mcse_mean", "ess_mean", "ess_sd", "mcse_sd", "quantile", "ess_quantile", "mcse_quantile", "rank_lower", "rank_upper",
                          "hdi_lower", "hdi_upper")


def posterior_summary(steps, probs=(0.05, 0.5, 0.95), hdi_prob=0.94, split=True, max_lag=0, slice_interval=1, chain_stride_steps=None, dtype=None, device=-1):
    """The summary row of every parameter with its Monte Carlo standard errors (include/mcmcpp_hip.h,
    mcmcpp_hip_posterior_summary; an extension).  steps: as for gelman_rubin.  probs: up to 16 probabilities inside (0, 1).
    hdi_prob: 0 for no highest-density interval (hdi_lower and hdi_upper are then NaN).  Returns a dict: mean, sd, mcse_mean,
    ess_mean, ess_sd, mcse_sd, hdi_lower, hdi_upper [(P,)] float64; quantile, ess_quantile, mcse_quantile [(P, len(probs))]
    float64; rank_lower, rank_upper [(P, len(probs))] int64; probs, hdi_prob, sequence_length, num_sequences."""
    if max_lag < 0:
        raise ValueError("max_lag must not be negative")
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    on_device, dtype, device, source, K, stride, n, W, P, _keep = _rhat_sources(steps, slice_interval, chain_stride_steps, dtype, device)
    Q = probs.size
    out = {k: np.zeros((P, Q) if "quantile" in k or k.startswith("rank_") else P, np.int64 if k.startswith("rank_") else np.float64) for k in POSTERIOR_SUMMARY_KEYS}
    out["hdi_lower"][:] = out["hdi_upper"][:] = np.nan
    length, count = C.c_int64(0), C.c_int64(0)
    outputs = [_ptr(a) if a.size else None for a in out.values()] + [C.cast(C.byref(length), C.c_void_p), C.cast(C.byref(count), C.c_void_p)]
    lead = [int(bool(split)), max_lag, _ptr(probs) if Q else None, Q, float(hdi_prob)]
    L_ = lib()
    if on_device:
        rc = L_.mcmcpp_hip_posterior_summary_device(dtype, device, source, K, stride, n, slice_interval, W, P, *(lead + outputs))
    else:
        rc = L_.mcmcpp_hip_posterior_summary(dtype, device, source, K, n, W, P, *(lead + outputs))
    if rc != OK:
        raise HipError(rc, (L_.mcmcpp_hip_posterior_summary_last_error() or b"").decode())
    out.update(probs=probs, hdi_prob=float(hdi_prob), sequence_length=length.value, num_sequences=count.value)
    return out
