"""ctypes binding of libmfhip.so (include/mfhip.h; test hooks: include/mfhip_testing.h).

This is the Python-side equivalent of the JNI shim in INTEGRATION.md: plain pointers and
sizes, status codes mapped to exceptions.  The library has no CPU fallback; loading fails
loudly when the shared object is missing, and context creation fails with MFNoDeviceError
when no GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFHIP_LIB", os.path.join(os.path.dirname(PKG_DIR), "lib", "libmfhip.so"))

MF_OK = 0
MF_ERR_INVALID = -1
MF_ERR_HIP = -2
MF_ERR_NOT_FITTED = -3
MF_ERR_NO_DEVICE = -4
MF_ERR_COMM = -5
MF_ERR_CAPACITY = -6
MF_ERR_STATE = -7

MODE_DETERMINISTIC_F64 = 0
MODE_FAST_F32 = 1
BLOCKING_REFERENCE = 0
BLOCKING_BALANCED = 1
SIDE_USER = 0
SIDE_ITEM = 1
ONLINE_NEXT_FACTORS = 0
ONLINE_DELTA = 1
ONLINE_SPARK_SWEEP = 2
INIT_PSEUDO_RANDOM = 0
INIT_SEEDED = 1
UID_BYTES = 128
RECOMMEND_MAX_TOP = 128
METRIC_DOT = 0     # mf_similar / mf_recommend_vectors: the score mf_recommend reports
METRIC_COSINE = 1  # ... scaled by both rows' inverse norms
ALS_REG_WEIGHTED = 0
ALS_REG_PLAIN = 1
ALS_CG_MAX_STEPS = 256
ALS_MAX_RANK = 256
ALS_SOLVER_CHOLESKY = 0
ALS_SOLVER_CG = 1
ALS_SOLVER_NNLS = 2
RANK_NMETRICS = 6  # precision, recall, ap, ndcg, rr, hit: a per-query row of mf_rank_eval
PAIR_RANK_COLD = -1      # mf_pair_ranks: the model does not hold the query id or the candidate id
PAIR_RANK_EXCLUDED = -2  # ... the pair itself is in the exclusion list
NEG_MAX = 64             # mf_online_update_sampled: negatives per event at most
BPR_SCALE_SUM = 0        # mf_bpr_run: a row's step is the sum of its slots' steps
BPR_SCALE_MEAN = 1       # ... divided by the row's slot count
BPR_MAX_REDRAWS = 62
BPR_MAX_BATCH = 1 << 24


class _Seen:
    """exclude=SEEN: the context's resident seen set (Context.seen_set / seen_add / seen_from_als) stands in
    for the exclusion arrays of recommend, rank_eval, pair_ranks and the prequential calls."""

    def __repr__(self):
        return "mfhip.SEEN"


SEEN = _Seen()


class MFError(RuntimeError):
    """Non-zero status from libmfhip (the JNI shim raises RuntimeException, like the reference)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[mfhip {code}] {msg}")
        self.code = code


class MFNoDeviceError(MFError):
    pass


class mf_params(C.Structure):
    _fields_ = [
        ("num_factors", C.c_int32),
        ("iterations", C.c_int32),
        ("lambda_", C.c_double),
        ("learning_rate", C.c_double),
        ("lr_method", C.c_int32),
        ("lr_arg", C.c_double),
        ("num_blocks", C.c_int32),
        ("seed", C.c_int64),
        ("has_seed", C.c_int32),
        ("mode", C.c_int32),
        ("online_learning_rate", C.c_double),
        ("online_init", C.c_int32),
        ("fast_waves", C.c_int32),
        ("fast_blocking", C.c_int32),
        ("reserved", C.c_int32 * 6),
    ]


class mf_stats(C.Structure):
    _fields_ = [
        ("updates", C.c_int64),
        ("supersteps", C.c_int64),
        ("kernel_launches", C.c_int64),
        ("kernel_ms", C.c_double),
        ("algorithmic_bytes", C.c_double),
        ("levels", C.c_int64),
        ("groups", C.c_int32),
        ("reserved0", C.c_int32),
        ("pads", C.c_int64),
        ("moved_bytes", C.c_double),
    ]


class mf_rank_metrics(C.Structure):
    _fields_ = [
        ("queries", C.c_int64),
        ("unknown_queries", C.c_int64),
        ("gt_pairs", C.c_int64),
        ("hits", C.c_int64),
        ("precision", C.c_double),
        ("recall", C.c_double),
        ("map", C.c_double),
        ("ndcg", C.c_double),
        ("mrr", C.c_double),
        ("hit_rate", C.c_double),
        ("reserved", C.c_double * 6),
    ]


class mf_prequential(C.Structure):
    _fields_ = [
        ("events", C.c_int64),
        ("evaluated", C.c_int64),
        ("cold", C.c_int64),
        ("excluded", C.c_int64),
        ("hits", C.c_int64),
        ("sum_ndcg", C.c_double),
        ("sum_rr", C.c_double),
        ("sum_pr", C.c_double),
        ("ndcg", C.c_double),
        ("mrr", C.c_double),
        ("hit_rate", C.c_double),
        ("mpr", C.c_double),
        ("reserved", C.c_double * 6),
    ]


class mf_als_nonneg_stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("rows", "iterations", "max_iterations", "capped", "reason2", "nan_rows")]


class mf_bpr_params(C.Structure):
    _fields_ = [
        ("lr", C.c_double),
        ("lambda_", C.c_double),
        ("batch", C.c_int32),
        ("scale", C.c_int32),
        ("redraws", C.c_int32),
        ("reserved0", C.c_int32),
        ("seed", C.c_int64),
        ("reserved", C.c_int32 * 4),
    ]


class mf_bpr_stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("slots", "void_slots", "user_rows_written", "item_rows_written")]


class mf_als_solve(C.Structure):
    """One of the eight kinds of half-sweep, for mf_als_run_rows / mf_als_update."""
    _fields_ = [
        ("lambda_", C.c_double),
        ("reg", C.c_int32),
        ("implicit", C.c_int32),
        ("alpha", C.c_double),
        ("solver", C.c_int32),
        ("cg_steps", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class mf_als_loss(C.Structure):
    """mf_als_objective's result: the objective's value and its parts."""
    _fields_ = [
        ("total", C.c_double),
        ("fit", C.c_double),
        ("unobserved", C.c_double),
        ("reg_user", C.c_double),
        ("reg_item", C.c_double),
        ("ratings", C.c_int64),
        ("user_rows", C.c_int64),
        ("item_rows", C.c_int64),
        ("reserved", C.c_double * 4),
    ]


# Every symbol include/mfhip.h declares (tests check the library exports all of them).
EXPORTS = [
    "mf_params_init", "mf_last_error", "mf_version", "mf_device_count", "mf_create",
    "mf_comm_unique_id", "mf_create_rank", "mf_destroy", "mf_dsgd_fit", "mf_dsgd_prepare",
    "mf_dsgd_run", "mf_dsgd_superstep", "mf_dsgd_set_superstep", "mf_sync", "mf_num_factors",
    "mf_get_factors", "mf_set_factors", "mf_predict", "mf_rmse", "mf_empirical_risk",
    "mf_block_update", "mf_online_update", "mf_lookup", "mf_set_profiling", "mf_get_stats",
    "mf_reset_stats", "mf_jvm_shuffle", "mf_jvm_block_of", "mf_jvm_random_factors",
    "mf_learning_rate", "mf_get_params", "mf_read_ratings", "mf_save_model", "mf_load_model",
    "mf_dsgd_restart", "mf_online_update_out", "mf_recommend", "mf_als_fit", "mf_als_prepare",
    "mf_als_run", "mf_als_run_implicit", "mf_als_fit_implicit", "mf_rank_eval", "mf_pair_ranks",
    "mf_online_prequential", "mf_online_update_sampled", "mf_negative_draws", "mf_online_prequential_sampled",
    "mf_als_run_cg", "mf_als_run_implicit_cg", "mf_als_fit_cg", "mf_als_fit_implicit_cg",
    "mf_als_run_nonneg", "mf_als_run_implicit_nonneg", "mf_als_fit_nonneg", "mf_als_fit_implicit_nonneg",
    "mf_als_nonneg_stats", "mf_nnls_solve", "mf_als_append", "mf_als_run_rows", "mf_als_update",
    "mf_seen_set", "mf_seen_add", "mf_seen_from_als", "mf_seen_clear", "mf_seen_count", "mf_recommend_seen",
    "mf_rank_eval_seen", "mf_pair_ranks_seen", "mf_online_prequential_seen", "mf_similar", "mf_recommend_vectors",
    "mf_als_remove", "mf_als_remove_rows", "mf_als_retract", "mf_seen_remove", "mf_als_foldin", "mf_recommend_foldin",
    "mf_recommend_among", "mf_bpr_run", "mf_bpr_step_triples", "mf_bpr_draws", "mf_bpr_fit",
    "mf_als_objective", "mf_als_run_until",
]
# The test hooks include/mfhip_testing.h declares (not product surface; same library).
TESTING_EXPORTS = [
    "mf_debug_levels", "mf_debug_fast_schedule", "mf_debug_fast_split", "mf_debug_ring_schedule",
    "mf_debug_plan_digest", "mf_fast_plan_window", "mf_fast_kernel_name", "mf_debug_build_flags",
    "mf_debug_device_bytes", "mf_debug_als_normal_eq", "mf_debug_als_gram", "mf_debug_als_normal_eq_implicit",
    "mf_debug_det_slot_table", "mf_debug_sys_placement", "mf_debug_rank_csr", "mf_debug_als_cg_matvec",
    "mf_debug_als_cg_capacity", "mf_debug_als_nnls_row", "mf_debug_als_csr", "mf_debug_als_append_placement",
    "mf_debug_seen_csr", "mf_debug_seen_merge_placement", "mf_debug_als_remove_select",
    "mf_debug_bpr_triples",
]

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_ctxp = C.c_void_p

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libmfhip.so not found at {LIB_PATH}; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP path has no fallback)")
    L = C.CDLL(LIB_PATH)
    sig = {
        "mf_params_init": (None, [C.POINTER(mf_params)]),
        "mf_last_error": (C.c_char_p, []),
        "mf_version": (C.c_char_p, []),
        "mf_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "mf_create": (C.c_int, [C.POINTER(mf_params), C.POINTER(C.c_int), C.c_int, C.POINTER(_ctxp)]),
        "mf_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
        "mf_create_rank": (C.c_int, [C.POINTER(mf_params), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8),
                                     C.POINTER(_ctxp)]),
        "mf_destroy": (C.c_int, [_ctxp]),
        "mf_dsgd_fit": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64]),
        "mf_dsgd_prepare": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64]),
        "mf_dsgd_run": (C.c_int, [_ctxp, C.c_int64]),
        "mf_dsgd_superstep": (C.c_int, [_ctxp, _i64p]),
        "mf_dsgd_set_superstep": (C.c_int, [_ctxp, C.c_int64]),
        "mf_sync": (C.c_int, [_ctxp]),
        "mf_num_factors": (C.c_int, [_ctxp, C.c_int, _i64p]),
        "mf_get_factors": (C.c_int, [_ctxp, C.c_int, _i32p, _f64p, C.c_int64, _i64p]),
        "mf_set_factors": (C.c_int, [_ctxp, C.c_int, _i32p, _f64p, C.c_int64]),
        "mf_predict": (C.c_int, [_ctxp, _i32p, _i32p, C.c_int64, _f64p, _u8p]),
        "mf_rmse": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, _f64p, _i64p]),
        "mf_empirical_risk": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_double, _f64p]),
        "mf_block_update": (C.c_int, [_ctxp, _f64p, _i32p, _i32p, C.c_int64, _f64p, _i32p, C.c_int64, _f64p,
                                      _i32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_double,
                                      C.c_int, C.c_double, C.c_double]),
        "mf_online_update": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int, C.c_int, _i64p, _i64p]),
        "mf_lookup": (C.c_int, [_ctxp, C.c_int, _i32p, C.c_int64, _f64p, _u8p]),
        "mf_set_profiling": (C.c_int, [_ctxp, C.c_int]),
        "mf_get_stats": (C.c_int, [_ctxp, C.POINTER(mf_stats)]),
        "mf_reset_stats": (C.c_int, [_ctxp]),
        "mf_jvm_shuffle": (C.c_int, [C.c_int64, C.c_int64, _i32p]),
        "mf_jvm_block_of": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, _i32p]),
        "mf_jvm_random_factors": (C.c_int, [C.c_int64, C.c_int32, _f64p]),
        "mf_learning_rate": (C.c_int, [C.c_int, C.c_double, C.c_int32, C.c_double, C.c_double, _f64p]),
        "mf_debug_levels": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _i32p, C.c_int64, _i32p]),
        "mf_debug_fast_schedule": (C.c_int, [_i32p, _i32p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i64p]),
        "mf_debug_fast_split": (C.c_int, [_i32p, _i32p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i64p, _i32p]),
        "mf_fast_plan_window": (C.c_int, [C.c_int32, _i32p]),
        "mf_fast_kernel_name": (C.c_char_p, [C.c_int32]),
        "mf_get_params": (C.c_int, [C.c_void_p, C.POINTER(mf_params)]),
        "mf_read_ratings": (C.c_int, [C.c_char_p, C.c_char, C.c_int32, _i32p, _i32p, _f64p, C.c_int64, _i64p]),
        "mf_save_model": (C.c_int, [C.c_void_p, C.c_char_p]),
        "mf_load_model": (C.c_int, [C.c_void_p, C.c_char_p, _i64p]),
        "mf_dsgd_restart": (C.c_int, [_ctxp]),
        "mf_online_update_out": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int, C.c_int, _i64p, _i64p,
                                           _f64p, _f64p]),
        "mf_recommend": (C.c_int, [_ctxp, C.c_int, _i32p, C.c_int64, C.c_int32, _i32p, _i32p, C.c_int64, _i32p, _f64p,
                                   _i32p]),
        "mf_similar": (C.c_int, [_ctxp, C.c_int, _i32p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p,
                                 C.c_int64, _i32p, _f64p, _i32p]),
        "mf_recommend_vectors": (C.c_int, [_ctxp, C.c_int, _f64p, C.c_int64, C.c_int32, C.c_int32, _i64p, _i32p,
                                           C.c_int64, _i32p, _f64p, _i32p]),
        "mf_rank_eval": (C.c_int, [_ctxp, C.c_int, _i32p, _i32p, C.c_int64, C.c_int32, _i32p, _i32p, C.c_int64,
                                   C.POINTER(mf_rank_metrics), _i32p, _i32p, _f64p, C.c_int64]),
        "mf_pair_ranks": (C.c_int, [_ctxp, C.c_int, _i32p, _i32p, C.c_int64, _i32p, _i32p, C.c_int64, _i32p, _i32p,
                                    _f64p]),
        "mf_online_prequential": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int, C.c_int, C.c_int32, _i32p,
                                            _i32p, C.c_int64, C.POINTER(mf_prequential), _i32p, _i64p, _i64p]),
        "mf_online_update_sampled": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int, C.c_int32, C.c_double,
                                               C.c_int64, C.c_int64, _i32p, _i64p, _i64p]),
        "mf_negative_draws": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int64, _i32p, _i32p]),
        "mf_online_prequential_sampled": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int, C.c_int32, _i32p,
                                                    _i32p, C.c_int64, C.POINTER(mf_prequential), _i32p, _i64p, _i64p,
                                                    C.c_int32, C.c_double, C.c_int64, C.c_int64, _i32p]),
        "mf_debug_rank_csr": (C.c_int, [_ctxp, C.c_int, C.c_int, _i32p, _i32p, C.c_int64, _i32p, _i64p, _i32p,
                                        C.c_int64, C.c_int64, _i64p, _i64p]),
        "mf_als_fit": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int32, C.c_double, C.c_int32]),
        "mf_als_prepare": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64]),
        "mf_als_run": (C.c_int, [_ctxp, C.c_int64, C.c_double, C.c_int32]),
        "mf_debug_als_normal_eq": (C.c_int, [_ctxp, C.c_int, C.c_int32, C.c_double, C.c_int32, _f64p, _f64p]),
        "mf_als_run_implicit": (C.c_int, [_ctxp, C.c_int64, C.c_double, C.c_int32, C.c_double]),
        "mf_als_fit_implicit": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int32, C.c_double, C.c_int32,
                                          C.c_double]),
        "mf_debug_als_gram": (C.c_int, [_ctxp, C.c_int, _f64p]),
        "mf_debug_als_normal_eq_implicit": (C.c_int, [_ctxp, C.c_int, C.c_int32, C.c_double, C.c_int32, C.c_double,
                                                      _f64p, _f64p]),
        "mf_als_run_cg": (C.c_int, [_ctxp, C.c_int64, C.c_double, C.c_int32, C.c_int32]),
        "mf_als_run_implicit_cg": (C.c_int, [_ctxp, C.c_int64, C.c_double, C.c_int32, C.c_double, C.c_int32]),
        "mf_als_fit_cg": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int32, C.c_double, C.c_int32,
                                    C.c_int32]),
        "mf_als_fit_implicit_cg": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int32, C.c_double, C.c_int32,
                                             C.c_double, C.c_int32]),
        "mf_debug_als_cg_matvec": (C.c_int, [_ctxp, C.c_int, C.c_int32, C.c_double, C.c_int32, C.c_double, _f64p,
                                             _f64p, _f64p]),
        "mf_debug_als_cg_capacity": (C.c_int, [_ctxp, _i32p]),
        "mf_als_run_nonneg": (C.c_int, [_ctxp, C.c_int64, C.c_double, C.c_int32]),
        "mf_als_run_implicit_nonneg": (C.c_int, [_ctxp, C.c_int64, C.c_double, C.c_int32, C.c_double]),
        "mf_als_fit_nonneg": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int32, C.c_double, C.c_int32]),
        "mf_als_fit_implicit_nonneg": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int32, C.c_double,
                                                 C.c_int32, C.c_double]),
        "mf_als_nonneg_stats": (C.c_int, [_ctxp, C.POINTER(mf_als_nonneg_stats)]),
        "mf_nnls_solve": (C.c_int, [C.c_int32, _f64p, _f64p, C.c_int, _f64p, _i32p, _i32p]),
        "mf_debug_als_nnls_row": (C.c_int, [_ctxp, C.c_int, C.c_int32, C.c_double, C.c_int32, C.c_double, _f64p,
                                            _i32p, _i32p]),
        "mf_als_append": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64]),
        "mf_als_run_rows": (C.c_int, [_ctxp, C.c_int, _i32p, C.c_int64, C.POINTER(mf_als_solve), _i64p]),
        "mf_als_objective": (C.c_int, [_ctxp, C.POINTER(mf_als_solve), C.POINTER(mf_als_loss)]),
        "mf_als_run_until": (C.c_int, [_ctxp, C.POINTER(mf_als_solve), C.c_int32, C.c_double, _i32p, _f64p]),
        "mf_als_foldin": (C.c_int, [_ctxp, C.c_int, _i64p, _i32p, _f64p, C.c_int64, C.POINTER(mf_als_solve), _f64p,
                                    _i32p]),
        "mf_recommend_foldin": (C.c_int, [_ctxp, C.c_int, _i64p, _i32p, _f64p, C.c_int64, C.POINTER(mf_als_solve),
                                          C.c_int32, C.c_int32, _i32p, _f64p, _i32p, _f64p, _i32p]),
        "mf_als_update": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.POINTER(mf_als_solve), C.c_int32, _i64p,
                                    _i64p]),
        "mf_debug_als_csr": (C.c_int, [_ctxp, C.c_int, _i64p, _i32p, _f64p, _i32p, C.c_int64, C.c_int64, _i64p,
                                       _i64p]),
        "mf_debug_als_append_placement": (C.c_int, [_i64p, C.c_int64, _i32p, C.c_int64, C.c_int64, _i64p, _i64p]),
        "mf_als_remove": (C.c_int, [_ctxp, _i32p, _i32p, C.c_int64, _u8p, _i64p]),
        "mf_als_remove_rows": (C.c_int, [_ctxp, C.c_int, _i32p, C.c_int64, _i64p]),
        "mf_als_retract": (C.c_int, [_ctxp, _i32p, _i32p, C.c_int64, C.POINTER(mf_als_solve), C.c_int32, _u8p, _i64p,
                                     _i64p, _i64p]),
        "mf_debug_als_remove_select": (C.c_int, [_i64p, C.c_int64, _i32p, _i32p, _i32p, C.c_int64, _i64p]),
        "mf_seen_remove": (C.c_int, [_ctxp, _i32p, _i32p, C.c_int64, _i64p, _i64p]),
        "mf_seen_set": (C.c_int, [_ctxp, _i32p, _i32p, C.c_int64, _i64p]),
        "mf_seen_add": (C.c_int, [_ctxp, _i32p, _i32p, C.c_int64, _i64p]),
        "mf_seen_from_als": (C.c_int, [_ctxp]),
        "mf_seen_clear": (C.c_int, [_ctxp]),
        "mf_seen_count": (C.c_int, [_ctxp, _i64p]),
        "mf_recommend_seen": (C.c_int, [_ctxp, C.c_int, _i32p, C.c_int64, C.c_int32, _i32p, _f64p, _i32p]),
        "mf_recommend_among": (C.c_int, [_ctxp, C.c_int, _i32p, C.c_int64, C.c_int32, _i64p, _i32p, C.c_int64, C.c_int32,
                                         _i32p, _i32p, C.c_int64, _i32p, _f64p, _i32p]),
        "mf_rank_eval_seen": (C.c_int, [_ctxp, C.c_int, _i32p, _i32p, C.c_int64, C.c_int32, C.POINTER(mf_rank_metrics),
                                        _i32p, _i32p, _f64p, C.c_int64]),
        "mf_pair_ranks_seen": (C.c_int, [_ctxp, C.c_int, _i32p, _i32p, C.c_int64, _i32p, _i32p, _f64p]),
        "mf_online_prequential_seen": (C.c_int, [_ctxp, _i32p, _i32p, _f64p, C.c_int64, C.c_int, C.c_int32,
                                                 C.POINTER(mf_prequential), _i32p, _i64p, _i64p, C.c_int32, C.c_double,
                                                 C.c_int64, C.c_int64, _i32p, C.c_int]),
        "mf_debug_seen_csr": (C.c_int, [_ctxp, C.c_int, _i32p, _i64p, _i32p, _i32p, C.c_int64, C.c_int64, _i64p,
                                        _i64p]),
        "mf_debug_seen_merge_placement": (C.c_int, [C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_uint64), C.c_int64,
                                                    _i64p, _i64p, _i64p]),
        "mf_bpr_run": (C.c_int, [_ctxp, C.POINTER(mf_bpr_params), C.c_int64, C.c_int64, C.POINTER(mf_bpr_stats)]),
        "mf_bpr_step_triples": (C.c_int, [_ctxp, C.POINTER(mf_bpr_params), _i32p, _i32p, _i32p, C.c_int64,
                                          C.POINTER(mf_bpr_stats)]),
        "mf_bpr_draws": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                   C.POINTER(C.c_uint64)]),
        "mf_bpr_fit": (C.c_int, [_ctxp, _i32p, _i32p, C.c_int64, C.c_double, C.POINTER(mf_bpr_params), C.c_int64,
                                 C.POINTER(mf_bpr_stats)]),
        "mf_debug_bpr_triples": (C.c_int, [_ctxp, _i32p, _i32p, _i32p, C.c_int64, _i64p]),
        "mf_debug_ring_schedule": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, _i32p, _i32p, _i32p, _i32p]),
        "mf_debug_det_slot_table": (C.c_int, [_i64p, _i32p, _i32p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, _i64p,
                                              _i32p, _i32p, _i64p]),
        "mf_debug_sys_placement": (C.c_int, [_f64p, C.c_int64, C.c_int64, C.c_int32, _i32p, _i32p]),
        "mf_debug_plan_digest": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
        "mf_debug_build_flags": (C.c_int32, []),
        "mf_debug_device_bytes": (C.c_int, [_i64p]),
    }
    for name, (res, args) in sig.items():
        if (name in TESTING_EXPORTS or "MFHIP_LIB" in os.environ) and not hasattr(L, name):
            continue  # an older build (A/B runs, named through MFHIP_LIB): it may predate this binding
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status: int) -> None:
    if status != MF_OK:
        msg = lib().mf_last_error().decode(errors="replace")
        if status == MF_ERR_NO_DEVICE:
            raise MFNoDeviceError(status, msg)
        raise MFError(status, msg)


def ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def as_i32(a) -> np.ndarray:
    """Ids as the reference's Int: values outside int32 are rejected, not wrapped."""
    arr = np.asarray(a)
    if arr.dtype != np.int32 and arr.size:
        if arr.dtype.kind not in "iub":
            raise ValueError(f"ids must be integers, got {arr.dtype}")
        lo, hi = int(arr.min()), int(arr.max())
        if lo < -2**31 or hi >= 2**31:
            raise ValueError(f"id out of the Int range: [{lo}, {hi}]")
    return np.ascontiguousarray(arr, dtype=np.int32)


def same_length(*arrays) -> int:
    """Rating columns must be parallel arrays: the C side reads len(first) elements of each."""
    n = len(arrays[0])
    for a in arrays[1:]:
        if len(a) != n:
            raise ValueError(f"columns differ in length: {[len(x) for x in arrays]}")
    return n


def as_f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def default_params() -> mf_params:
    p = mf_params()
    lib().mf_params_init(C.byref(p))
    return p


def device_count() -> int:
    n = C.c_int(0)
    check(lib().mf_device_count(C.byref(n)))
    return n.value


def version() -> str:
    return lib().mf_version().decode()
