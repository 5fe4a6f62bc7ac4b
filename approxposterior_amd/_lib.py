# -*- coding: utf-8 -*-
"""
ctypes binding of ``libapgp.so`` (include/apgp.h): the hand-written HIP kernels
for gfx950.  There is NO fallback: if the shared library is missing or was
built for another ABI the import fails loudly, and every call that returns a
non-zero status raises ``ApgpError`` with the library's message.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libapgp.so")
ABI_VERSION = 8
MAX_DIM = 32
MAX_FANTASY = 32      # APGP_MAX_FANTASY: points per batch of GP.acquire_batch
MAX_DRAWS = 32        # APGP_MAX_DRAWS: posterior function draws per apgp_path_draws call
MAX_FEATURES = 65536  # APGP_MAX_FEATURES: random Fourier features of a draw
MAX_REFS = 4096       # APGP_MAX_REFS: reference points per apgp_acquire_integrated call
INTEGRATED_MAX_DIM = 16   # APGP_INTEGRATED_MAX_DIM: dimensions apgp_acquire_integrated takes

UTIL_AGP, UTIL_BAPE, UTIL_JONES, UTIL_NONE = 0, 1, 2, 3
UTIL_NEG_MEAN = 4     # -mu (ApproxPosterior.findMAP's objective): apgp_nm_search only
NM_MAX_RESTARTS = 4096
NM_MAX_FEV = 1 << 20
# APGP_NM_STEP_*: the step of one Nelder-Mead iteration in apgp_nm_search's trace
NM_STEPS = {1: "reflect", 2: "expand", 3: "reflect_exp", 4: "contract_out", 5: "contract_in",
            6: "shrink_out", 7: "shrink_in", 8: "maxfev"}
PRUNE_ROWS_SPLIT, PRUNE_ROWS_SIGNED = 0, 1   # APGP_PRUNE_ROWS_*: the kind of a coarse-bound row stream
GMM_EM, GMM_SCORE, GMM_KMEANS = 0, 1, 2
GMM_MAX_COMP = 16
IMP_BLOCK = 256        # APGP_IMP_BLOCK: candidates per workgroup pass of apgp_importance_pass
IMP_MAX_BLOCKS = 2048  # APGP_IMP_MAX_BLOCKS: beyond IMP_BLOCK * IMP_MAX_BLOCKS rows a workgroup takes further tiles


class ApgpError(RuntimeError):
    pass


class KernelStruct(ctypes.Structure):
    """``apgp_kernel_t`` (include/apgp.h)."""
    _fields_ = [("ndim", ctypes.c_int32), ("lin_order", ctypes.c_int32),
                ("amp", ctypes.c_double), ("diag_add", ctypes.c_double),
                ("inv_metric", ctypes.c_double * MAX_DIM), ("lin_coef", ctypes.c_double)]


class BestStruct(ctypes.Structure):
    """``apgp_best_t``."""
    _fields_ = [("u", ctypes.c_double), ("index", ctypes.c_int64)]


class NmOptions(ctypes.Structure):
    """``apgp_nm_options_t``."""
    _fields_ = [("kind", ctypes.c_int32), ("maxiter", ctypes.c_int32), ("maxfev", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("zeta", ctypes.c_double), ("ybest", ctypes.c_double),
                ("xatol", ctypes.c_double), ("fatol", ctypes.c_double), ("rho", ctypes.c_double),
                ("chi", ctypes.c_double), ("psi", ctypes.c_double), ("sigma", ctypes.c_double)]


class EnsMove(ctypes.Structure):
    """``apgp_ens_move_t``: one entry of the ensemble sampler's move table."""
    _fields_ = [("kind", ctypes.c_int32), ("weight", ctypes.c_double), ("p0", ctypes.c_double), ("p1", ctypes.c_double)]


ENS_MOVE_STRETCH, ENS_MOVE_DE, ENS_MOVE_SNOOKER = 0, 1, 2
ENS_MAX_MOVES = 8     # APGP_ENS_MAX_MOVES
PT_MAX_TEMPS = 64     # APGP_PT_MAX_TEMPS: rungs of a tempering ladder
HMC_MAX_LEAP = 1024   # APGP_HMC_MAX_LEAP: leapfrog steps per iteration of apgp_hmc_sample
HMC_G_ROWS = (1, 4)   # wavefronts per chain apgp_hmc_sample offers (g_rows; 0 = the library's rule)
NESTED_MAX_LIVE = 4096   # live points per run of apgp_nested_sample
NESTED_MAX_BATCH = 16    # points replaced per batch: a wavefront per walker


class HmcOptions(ctypes.Structure):
    """``apgp_hmc_options_t``."""
    _fields_ = [("eps", ctypes.c_double), ("jitter", ctypes.c_double), ("nleap", ctypes.c_int32),
                ("g_rows", ctypes.c_int32), ("iteration0", ctypes.c_int64), ("mass", ctypes.c_double * MAX_DIM)]

_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32
_F64 = ctypes.c_double
_KP = ctypes.POINTER(KernelStruct)

# name -> (restype, argtypes); every symbol include/apgp.h declares
SIGNATURES = {
    "apgp_abi_version": (ctypes.c_int, []),
    "apgp_last_error": (ctypes.c_char_p, []),
    "apgp_npad": (_I64, [_I64]),
    "apgp_packed_linv_len": (_I64, [_I64]),
    "apgp_acquire_work_len": (_I64, [_I64, _I64]),
    "apgp_packed_train_len": (_I64, [_I64, _I32]),
    "apgp_trtri_work_len": (_I64, [_I64]),
    "apgp_grad_work_len": (_I64, [_I64]),
    "apgp_gram": (ctypes.c_int, [_P, _I64, _KP, _P, _I64, _P]),
    "apgp_kernel_cross": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _P, _I64, _P]),
    "apgp_potrf": (ctypes.c_int, [_P, _I64, _I64, _P, _F64, _P, _P, _P]),
    "apgp_logdet": (ctypes.c_int, [_P, _I64, _I64, _P, _P]),
    "apgp_fit_summary": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _P, _P]),
    "apgp_nll_eval": (ctypes.c_int, [_P, _I64, _KP, _P, _F64, _P, _P, _P, _P, _P, _P]),
    "apgp_potrf_mode": (ctypes.c_int, [ctypes.c_int]),
    "apgp_potrf_fallbacks": (_I64, []),
    "apgp_potrf_backoff_skips": (_I64, []),
    "apgp_nll_side_batches": (_I64, []),
    "apgp_nll_eval_batch": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "apgp_trsv": (ctypes.c_int, [_P, _I64, _I64, _P, _F64, ctypes.c_int, _P, _P, _P]),
    "apgp_trsv_ex": (ctypes.c_int, [_P, _I64, _I64, _P, _F64, ctypes.c_int, _P, _P, ctypes.c_int, _P]),
    "apgp_trsv_mode": (ctypes.c_int, [ctypes.c_int]),
    "apgp_append_diag": (ctypes.c_int, [_P, _P, _F64, _P, _I64, _P]),
    "apgp_winv_apply_work_len": (_I64, [_I64]),
    "apgp_winv_apply": (ctypes.c_int, [_P, _I64, _I64, _P, _F64, ctypes.c_int, _P, _P, _P, _P]),
    "apgp_trtri_pack": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _P, _P]),
    "apgp_pack_train": (ctypes.c_int, [_P, _P, _I64, _KP, _P, _P]),
    "apgp_acquire": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _I64, _KP, _F64, _I32,
                                    ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P,
                                    _F64, _F64, _P, _P, _P, _P, _P, _P]),
    "apgp_packed_lsolve_len": (_I64, [_I64]),
    "apgp_pack_lsolve": (ctypes.c_int, [_P, _I64, _I64, _P, _P]),
    "apgp_acquire_solve": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _I64, _KP, _F64, _I32,
                                          ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P,
                                          _F64, _F64, _P, _P, _P, _P, _P, _P]),
    "apgp_set_sweep_prune": (ctypes.c_int, [ctypes.c_int]),
    "apgp_get_sweep_prune": (ctypes.c_int, []),
    "apgp_set_seed_rowsplit": (ctypes.c_int, [ctypes.c_int]),
    "apgp_get_seed_rowsplit": (ctypes.c_int, []),
    "apgp_set_seed_park": (ctypes.c_int, [ctypes.c_int]),
    "apgp_get_seed_park": (ctypes.c_int, []),
    "apgp_set_prune_pipe": (ctypes.c_int, [ctypes.c_int]),
    "apgp_get_prune_pipe": (ctypes.c_int, []),
    "apgp_set_seed_prefetch": (ctypes.c_int, [ctypes.c_int]),
    "apgp_get_seed_prefetch": (ctypes.c_int, []),
    "apgp_set_seed_first": (ctypes.c_int, [ctypes.c_int]),
    "apgp_get_seed_first": (ctypes.c_int, []),
    "apgp_set_seed_parts": (ctypes.c_int, [ctypes.c_int]),
    "apgp_get_seed_parts": (ctypes.c_int, []),
    "apgp_sweep_prune_counts_offset": (_I64, [_I64, _I64]),
    "apgp_sweep_prune_select": (ctypes.c_int, [_P, _I64, _P, _P, _F64, _P, _P]),
    "apgp_prune_bounds": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _F64, _I32, ctypes.POINTER(_F64), ctypes.POINTER(_F64),
                                         _P, _F64, _F64, ctypes.c_int, _P, _P]),
    "apgp_sweep_prune_seeds": (ctypes.c_int, [_P, _I64, _P, _P, _P]),
    "apgp_prune_rows_len": (_I64, [_I64, _I32]),
    "apgp_pack_prune_rows": (ctypes.c_int, [_P, _I64, _KP, _P, _P]),
    "apgp_acquire_rows": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _I64, _KP, _F64, _I32,
                                         ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P,
                                         _F64, _F64, _P, _P, _P, _P, _P, _P, _P]),
    "apgp_acquire_solve_rows": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _I64, _KP, _F64, _I32,
                                               ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P,
                                               _F64, _F64, _P, _P, _P, _P, _P, _P, _P]),
    "apgp_prune_bounds_rows": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _F64, _I32, ctypes.POINTER(_F64),
                                              ctypes.POINTER(_F64), _P, _F64, _F64, ctypes.c_int, _P, _P, _P]),
    "apgp_prune_srows_len": (_I64, [_I64, _I32]),
    "apgp_pack_prune_srows": (ctypes.c_int, [_P, _I64, _KP, _P, _P]),
    "apgp_acquire_rows2": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _I64, _KP, _F64, _I32,
                                          ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P,
                                          _F64, _F64, _P, _P, _P, _P, _P, _P, _I32, _P]),
    "apgp_acquire_solve_rows2": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _I64, _KP, _F64, _I32,
                                                ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P,
                                                _F64, _F64, _P, _P, _P, _P, _P, _P, _I32, _P]),
    "apgp_prune_bounds_rows2": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _F64, _I32, ctypes.POINTER(_F64),
                                               ctypes.POINTER(_F64), _P, _F64, _F64, ctypes.c_int, _P, _P, _I32, _P, _P]),
    "apgp_acquire_fantasy_work_len": (_I64, [_I64]),
    "apgp_acquire_fantasy": (ctypes.c_int, [_P, _I64, _I64, _P, _I64, _KP, _P, _I64, _I32, _P, _I64,
                                            _P, _P, _P, _I32, ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P,
                                            _F64, _F64, _P, _P, _P, _P]),
    "apgp_path_draws_work_len": (_I64, [_I64, _I32]),
    "apgp_path_draws_mode": (ctypes.c_int, [ctypes.c_int]),
    "apgp_path_draws": (ctypes.c_int, [_P, _I64, _I64, _P, _I64, _KP, _F64, _P, _P, _P, _P, _P, _I32, _I32,
                                       ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P, _P, _P, _P, _P]),
    "apgp_integrated_work_len": (_I64, [_I64, _I32]),
    "apgp_integrated_mode": (ctypes.c_int, [ctypes.c_int]),
    "apgp_acquire_integrated": (ctypes.c_int, [_P, _I64, _I64, _P, _I64, _KP, _P, _I32, _P, _P, _P,
                                               ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P, _P, _I64, _P, _P, _P, _P]),
    "apgp_predict1_work_len": (_I64, [_I64]),
    "apgp_predict1_host": (ctypes.c_int, [_P, _P, _I64, _KP, _F64, _P, _I64, _P, _I64, _P, _P, _P]),
    "apgp_nm_search_work_len": (_I64, [_I64, _I64]),
    "apgp_nm_search": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _F64, _P, _I64, _P, _I64,
                                      ctypes.POINTER(_F64), ctypes.POINTER(_F64), ctypes.POINTER(NmOptions),
                                      _P, _P, _P, _P, _P, _P, _P]),
    "apgp_predict_grad_work_len": (_I64, [_I64, _I64]),
    "apgp_predict_grad": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _F64, _P, _I64, _P, _I64, _I32,
                                         ctypes.POINTER(_F64), ctypes.POINTER(_F64), _F64, _F64,
                                         _P, _P, _P, _P, _P, _P, _P, _P]),
    "apgp_predict_mean": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _F64, _P, _P]),
    "apgp_predict_mean_host": (ctypes.c_int, [_P, _I64, _P, _I64, _KP, _F64, _P, _P, _P]),
    "apgp_ensemble_sample": (ctypes.c_int, [_P, _I64, _KP, _F64, ctypes.POINTER(_F64), ctypes.POINTER(_F64),
                                            _I32, _I32, _I64, _F64, ctypes.c_uint64, _P, _P, _P, _P, _P, _P]),
    "apgp_ensemble_sample_ex": (ctypes.c_int, [_P, _I64, _KP, _F64, ctypes.POINTER(_F64), ctypes.POINTER(_F64),
                                               _I32, _I32, _I64, _F64, ctypes.c_uint64, _P, _P, _P, _P, _P, ctypes.c_int, _P]),
    "apgp_ensemble_sample_moves": (ctypes.c_int, [_P, _I64, _KP, _F64, ctypes.POINTER(_F64), ctypes.POINTER(_F64),
                                                  _I32, _I32, _I64, _F64, ctypes.c_uint64, _P, _P, _P, _P, _P, ctypes.c_int,
                                                  ctypes.POINTER(EnsMove), _I32, _P]),
    "apgp_ensemble_mode": (ctypes.c_int, [ctypes.c_int]),
    "apgp_tempered_work_len": (_I64, [_I32, _I32, _I32, _I32]),
    "apgp_tempered_sample": (ctypes.c_int, [_P, _I64, _KP, _F64, ctypes.POINTER(_F64), ctypes.POINTER(_F64), _I32, _I32, _I32,
                                            ctypes.POINTER(_F64), _I64, _I64, ctypes.c_uint64, _P, _P, _P, _I32, _P, _P, _P,
                                            _P, _P, ctypes.POINTER(EnsMove), _I32, _P, _P]),
    "apgp_hmc_sample": (ctypes.c_int, [_P, _I64, _KP, _F64, ctypes.POINTER(_F64), ctypes.POINTER(_F64), _I32, _I64,
                                       ctypes.POINTER(HmcOptions), ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "apgp_hmc_rule": (ctypes.c_int, [_I32, _I64, _I32]),
    "apgp_nested_work_len": (_I64, [_I32, _I32, _I32]),
    "apgp_nested_xlds": (ctypes.c_int, [_I64, _I32]),
    "apgp_nested_sample": (ctypes.c_int, [_P, _I64, _KP, _F64, ctypes.POINTER(_F64), ctypes.POINTER(_F64), _I32, _I32, _I32,
                                          _I32, _F64, _F64, _F64, _I32, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "apgp_box_candidates": (ctypes.c_int, [_P, _I64, _I32, ctypes.POINTER(_F64), ctypes.POINTER(_F64), ctypes.c_uint64,
                                           _I64, _P]),
    "apgp_prior_candidates": (ctypes.c_int, [_P, _I64, _I32, _P, _P, _P, ctypes.c_uint64, _I64, _P]),
    "apgp_prior_lnprior": (ctypes.c_int, [_P, _I64, _I32, _P, _P, _P, _P, _P]),
    "apgp_release_scratch": (ctypes.c_int, [_P]),
    "apgp_kinv_solve_work_len": (_I64, [_I64]),
    "apgp_kinv_solve": (ctypes.c_int, [_P, _I64, _I64, _P, _P, _P]),
    "apgp_grad_loglik": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _KP, _P, _P, _P]),
    "apgp_gmm_params_len": (_I64, [_I32, _I32]),
    "apgp_gmm_stats_len": (_I64, [_I32, _I32]),
    "apgp_gmm_pass": (ctypes.c_int, [_P, _I64, _I32, _I32, _P, _I32, _P, _P, _P, _P]),
    "apgp_mix_params_len": (_I64, [_I32, _I32]),
    "apgp_mix_candidates": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, ctypes.c_uint64, _I64, _P]),
    "apgp_sobol_direction": (_I32, [_I32, _I32]),
    "apgp_sobol_box_candidates": (ctypes.c_int, [_P, _I64, _I32, ctypes.POINTER(_F64), ctypes.POINTER(_F64), ctypes.c_uint64,
                                                 _I32, _I32, _I64, _P]),
    "apgp_sobol_prior_candidates": (ctypes.c_int, [_P, _I64, _I32, _P, _P, _P, ctypes.c_uint64, _I32, _I32, _I64, _P]),
    "apgp_sobol_mix_candidates": (ctypes.c_int, [_P, _P, _I64, _I32, _I32, _P, ctypes.c_uint64, _I32, _I32, _I64, _P]),
    "apgp_importance_stats_len": (_I64, [_I32]),
    "apgp_importance_work_len": (_I64, [_I64]),
    "apgp_importance_pass": (ctypes.c_int, [_P, _I64, _P, _P, _I64, _KP, _F64, ctypes.POINTER(_F64), ctypes.POINTER(_F64),
                                            _P, _P, _P, _P, _P]),
    "apgp_path_importance_work_len": (_I64, [_I64, _I32]),
    "apgp_path_importance": (ctypes.c_int, [_P, _I64, _P, _P, _I64, _KP, _F64, _P, _P, _P, _P, _P, _I32, _I32,
                                            ctypes.POINTER(_F64), ctypes.POINTER(_F64), _P, _P, _P, _P, _P]),
    "apgp_autocorr_work_len": (_I64, [_I64, _I64, _I32]),
    "apgp_autocorr_block": (ctypes.c_int, [_P, _I64, _I64, _I32, _I64, _I64, _I64, _I64, _I32, _P, _P, _P]),
}

_lib = None


def load():
    """Load libapgp.so (once).  torch is imported first so that the HIP runtime
    already mapped by PyTorch-ROCm is the one the library binds to (same
    SONAME), which lets it launch on torch's streams and device buffers."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ApgpError(
            "libapgp.so not found at %s -- build it with "
            "`make -C approxposterior_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback." % LIB_PATH)
    import torch  # noqa: F401  (maps libamdhip64 first)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    v = lib.apgp_abi_version()
    if v != ABI_VERSION:
        raise ApgpError("libapgp.so ABI %d != expected %d" % (v, ABI_VERSION))
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().apgp_last_error()
        raise ApgpError("%s failed (%d): %s" % (what, status, msg.decode() if msg else ""))
