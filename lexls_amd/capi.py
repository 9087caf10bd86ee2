"""ctypes loader for liblexls_hip.so (the C ABI declared in include/lexls_hip.h).

The library is built in-tree by ``lexls_amd.build.build_native()`` (hipcc, gfx950).  There is no
Python or CPU fallback for the compute path: if the shared object is missing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LEXLS_HIP_LIB", os.path.join(_HERE, "csrc", "liblexls_hip.so"))  # env override: kernel-tuning A/B builds

# every symbol include/lexls_hip.h declares (tests/test_capi_symbols.py checks the export table against the header)
SYMBOLS = [
    "lexls_last_error", "lexls_version", "lexls_device_count",
    "lexls_lse_create", "lexls_lse_destroy", "lexls_lse_set_stream", "lexls_lse_synchronize",
    "lexls_lse_set_tolerance", "lexls_lse_set_obj_dim", "lexls_lse_set_fixed", "lexls_lse_set_ctr_type",
    "lexls_lse_set_problem_host", "lexls_lse_set_problem_device", "lexls_lse_set_skip",
    "lexls_lse_set_constraint_data", "lexls_lse_gather_problem", "lexls_lse_solve_least_norm_2", "lexls_lse_set_fixed_type", "lexls_lse_get_fixed_type", "lexls_lse_set_deferred_sync", "lexls_lse_set_regularization", "lexls_lse_set_cg_iterations", "lexls_lsi_solve_ex", "lexls_lsi_solve_debug", "lexls_lsi_batch_solve_ex", "lexls_lse_solve_least_norm_3",
    "lexls_lsi_batch_create", "lexls_lsi_batch_run", "lexls_lsi_batch_destroy", "lexls_lsi_batch_stats",
    "lexls_lse_round_layout", "lexls_lse_upload_round", "lexls_lse_download_round", "lexls_lse_sensitivity_resident", "lexls_lse_set_sensitivity_scan",
    "lexls_lse_factorize", "lexls_lse_solve", "lexls_lse_factorize_solve", "lexls_lse_solve_least_norm",
    "lexls_lse_residual", "lexls_lse_sensitivity",
    "lexls_lse_get_x", "lexls_lse_get_factor", "lexls_lse_get_hh_scalars", "lexls_lse_get_permutation", "lexls_lse_get_ranks",
    "lexls_lse_get_v", "lexls_lse_get_mu", "lexls_lse_get_lambda", "lexls_lse_get_sensitivity", "lexls_lse_get_ctr_type",
    "lexls_lse_device_ptr", "lexls_lse_last_kernel", "lexls_lse_last_consumer_kernel", "lexls_lse_last_large_levels", "lexls_lse_last_reg_placement", "lexls_lse_set_kernel_policy",
    "lexls_lse_set_accuracy_guard", "lexls_lse_get_accuracy",
    "lexls_lse_set_prefix_reuse", "lexls_lse_prefix_reuse_ready", "lexls_lse_set_resume_levels",
    "lexls_lsi_solve", "lexls_lsi_solve_dat", "lexls_lsi_batch_solve",
    "lexls_lse_multipliers", "lexls_lse_get_multipliers", "lexls_lse_solve_adjoint", "lexls_lse_set_adjoint_regularized", "lexls_lse_get_adjoint", "lexls_lse_solve_adjoint_device",
    "lexls_lse_solve_adjoint_multi", "lexls_lse_get_adjoint_multi", "lexls_lse_solve_adjoint_multi_device", "lexls_lse_set_adjoint_regularized_multi",
    "lexls_lse_solve_adjoint_matrix", "lexls_lse_get_adjoint_matrix", "lexls_lse_solve_adjoint_matrix_device",
    "lexls_lse_solve_tangent", "lexls_lse_get_tangent", "lexls_lse_solve_tangent_device",
    "lexls_lse_solve_rhs", "lexls_lse_get_solve_rhs", "lexls_lse_solve_rhs_device",
    "lexls_lse_residual_rhs", "lexls_lse_get_residual_rhs", "lexls_lse_residual_rhs_device",
    "lexls_lsi_batch_get_lambda", "lexls_lsi_batch_solve_ex2",
    "lexls_lse_sensitivity_collect", "lexls_lse_sensitivity_collect_resident", "lexls_lse_get_wrong_sign",
    "lexls_lsi_batch_get_cycling_counters", "lexls_lsi_batch_run_device", "lexls_lsi_batch_run_device_ex",
    "lexls_lsi_batch_set_instance_regularization",
    "lexls_lsi_batch_set_working_set_log", "lexls_lsi_batch_get_working_set_log", "lexls_lsi_batch_working_set_log_device",
    "lexls_lsi_batch_enqueue_device", "lexls_lsi_batch_finish",
    "lexls_lsi_batch_set_instance_mask", "lexls_lsi_batch_set_instance_max_factorizations", "lexls_lsi_batch_set_instance_obj_dims",
    "lexls_lsi_batch_solve_adjoint", "lexls_lsi_batch_solve_adjoint_device", "lexls_lsi_batch_set_adjoint_regularized",
    "lexls_lsi_batch_solve_adjoint_multi", "lexls_lsi_batch_solve_adjoint_multi_device", "lexls_lsi_batch_set_adjoint_regularized_multi",
    "lexls_lsi_batch_solve_adjoint_matrix", "lexls_lsi_batch_solve_adjoint_matrix_device", "lexls_lsi_batch_final_factorizations",
    "lexls_lsi_batch_solve_tangent", "lexls_lsi_batch_solve_tangent_device",
    "lexls_lsi_batch_solve_bounds", "lexls_lsi_batch_solve_bounds_device", "lexls_lsi_batch_last_consumer_kernel",
    "lexls_lsi_batch_solve_bounds_cost", "lexls_lsi_batch_solve_bounds_cost_device",
    "lexls_lsi_batch_last_kernel",
]

# one entry of a working-set log (lexls_lsi_debug::log, lexls_lsi_batch_get_working_set_log): the int32 fields of a row, in the order of the
# header's LEXLS_LSI_LOG_* indices; alpha_or_lambda travels in a double array of its own
WORKING_SET_LOG_FIELDS = ("obj_index", "ctr_index", "ctr_type", "cycling_detected", "rank")

ARRAY = dict(x=0, factor=1, hh=2, perm=3, rank=4, first_col=5, total_rank=6, v=7, lam=8, input=9, guard_estimate=10, guard_status=11,
             multipliers=12, wrong_sign=13)

_lib = None


class LexlsError(RuntimeError):
    pass


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LexlsError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        _lib.lexls_last_error.restype = C.c_char_p
        _lib.lexls_lse_last_kernel.restype = C.c_char_p
        _lib.lexls_lse_last_kernel.argtypes = [C.c_void_p]
        _lib.lexls_lse_last_consumer_kernel.restype = C.c_int
        _lib.lexls_lse_last_consumer_kernel.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        _lib.lexls_lse_last_large_levels.restype = C.c_int
        _lib.lexls_lse_last_large_levels.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.lexls_lse_last_reg_placement.restype = C.c_int
        _lib.lexls_lse_last_reg_placement.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.lexls_lsi_batch_last_kernel.restype = C.c_char_p
        _lib.lexls_lsi_batch_last_kernel.argtypes = [C.c_void_p]
        _lib.lexls_lse_set_accuracy_guard.restype = C.c_int
        _lib.lexls_lse_set_accuracy_guard.argtypes = [C.c_void_p, C.c_int, C.c_double]
        _lib.lexls_lse_get_accuracy.restype = C.c_int
        _lib.lexls_lse_get_accuracy.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
        _lib.lexls_lse_sensitivity_collect.restype = C.c_int
        _lib.lexls_lse_sensitivity_collect.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_double, C.c_double]
        _lib.lexls_lse_sensitivity_collect_resident.restype = C.c_int
        _lib.lexls_lse_sensitivity_collect_resident.argtypes = [C.c_void_p, C.c_double, C.c_double]
        _lib.lexls_lse_get_wrong_sign.restype = C.c_int
        _lib.lexls_lse_get_wrong_sign.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
        _lib.lexls_lsi_batch_get_cycling_counters.restype = C.c_int
        _lib.lexls_lsi_batch_get_cycling_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        _lib.lexls_lsi_batch_run_device.restype = C.c_int
        _lib.lexls_lsi_batch_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                    C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # the d_* arrays: device addresses
        _lib.lexls_lsi_batch_run_device_ex.restype = C.c_int
        _lib.lexls_lsi_batch_run_device_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # + d_v0; d_lambda, d_cycling_counts
        _lib.lexls_lsi_batch_enqueue_device.restype = C.c_int
        _lib.lexls_lsi_batch_enqueue_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                                        C.POINTER(C.c_double), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p]  # handle, stream, then run_device_ex's arguments, d_status
        _lib.lexls_lsi_batch_finish.restype = C.c_int
        _lib.lexls_lsi_batch_finish.argtypes = [C.c_void_p, C.c_void_p]  # handle, stream
        _lib.lexls_lsi_batch_set_instance_regularization.restype = C.c_int
        _lib.lexls_lsi_batch_set_instance_regularization.argtypes = [C.c_void_p, C.c_void_p, C.c_int]  # factors: host or device address
        _lib.lexls_lsi_batch_set_instance_mask.restype = C.c_int
        _lib.lexls_lsi_batch_set_instance_mask.argtypes = [C.c_void_p, C.c_void_p]  # d_mask: a device address
        _lib.lexls_lsi_batch_set_instance_max_factorizations.restype = C.c_int
        _lib.lexls_lsi_batch_set_instance_max_factorizations.argtypes = [C.c_void_p, C.c_void_p]  # d_limits: a device address
        _lib.lexls_lsi_batch_set_instance_obj_dims.restype = C.c_int
        _lib.lexls_lsi_batch_set_instance_obj_dims.argtypes = [C.c_void_p, C.c_void_p]  # d_dims: a device address
        _lib.lexls_lsi_batch_set_working_set_log.restype = C.c_int
        _lib.lexls_lsi_batch_set_working_set_log.argtypes = [C.c_void_p, C.c_uint32]
        _lib.lexls_lsi_batch_get_working_set_log.restype = C.c_int
        _lib.lexls_lsi_batch_get_working_set_log.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        _lib.lexls_lsi_batch_working_set_log_device.restype = C.c_int
        _lib.lexls_lsi_batch_working_set_log_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        _lib.lexls_lsi_batch_set_adjoint_regularized.restype = C.c_int
        _lib.lexls_lsi_batch_set_adjoint_regularized.argtypes = [C.c_void_p, C.c_int]
        _lib.lexls_lse_set_adjoint_regularized.restype = C.c_int
        _lib.lexls_lse_set_adjoint_regularized.argtypes = [C.c_void_p, C.c_int]
        _lib.lexls_lsi_batch_set_adjoint_regularized_multi.restype = C.c_int
        _lib.lexls_lsi_batch_set_adjoint_regularized_multi.argtypes = [C.c_void_p, C.c_int]
        _lib.lexls_lse_set_adjoint_regularized_multi.restype = C.c_int
        _lib.lexls_lse_set_adjoint_regularized_multi.argtypes = [C.c_void_p, C.c_int]
        _lib.lexls_lse_solve_adjoint.restype = C.c_int
        _lib.lexls_lse_solve_adjoint.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        _lib.lexls_lse_get_adjoint.restype = C.c_int
        _lib.lexls_lse_get_adjoint.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib.lexls_lse_solve_adjoint_device.restype = C.c_int
        _lib.lexls_lse_solve_adjoint_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # d_g, d_grad_rhs, d_grad_fixed: device addresses
        _lib.lexls_lsi_batch_solve_adjoint.restype = C.c_int
        _lib.lexls_lsi_batch_solve_adjoint.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib.lexls_lsi_batch_solve_adjoint_device.restype = C.c_int
        _lib.lexls_lsi_batch_solve_adjoint_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # d_g, d_grad_lb, d_grad_ub: device addresses
        _lib.lexls_lse_solve_adjoint_multi.restype = C.c_int
        _lib.lexls_lse_solve_adjoint_multi.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32]
        _lib.lexls_lse_get_adjoint_multi.restype = C.c_int
        _lib.lexls_lse_get_adjoint_multi.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib.lexls_lse_solve_adjoint_multi_device.restype = C.c_int
        _lib.lexls_lse_solve_adjoint_multi_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]  # d_G, ncot, d_grad_rhs, d_grad_fixed
        _lib.lexls_lse_solve_adjoint_matrix.restype = C.c_int
        _lib.lexls_lse_solve_adjoint_matrix.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        _lib.lexls_lse_get_adjoint_matrix.restype = C.c_int
        _lib.lexls_lse_get_adjoint_matrix.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        _lib.lexls_lse_solve_adjoint_matrix_device.restype = C.c_int
        _lib.lexls_lse_solve_adjoint_matrix_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # d_g, d_grad_lod, d_differentiable
        _lib.lexls_lse_solve_tangent.restype = C.c_int
        _lib.lexls_lse_solve_tangent.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32]  # h_dlod, h_dfixed, ntan
        _lib.lexls_lse_get_tangent.restype = C.c_int
        _lib.lexls_lse_get_tangent.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        _lib.lexls_lse_solve_tangent_device.restype = C.c_int
        _lib.lexls_lse_solve_tangent_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]  # d_dlod, d_dfixed, ntan, d_dx, d_differentiable
        _lib.lexls_lse_solve_rhs.restype = C.c_int
        _lib.lexls_lse_solve_rhs.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32]  # h_rhs, h_fixed, nrhs
        _lib.lexls_lse_get_solve_rhs.restype = C.c_int
        _lib.lexls_lse_get_solve_rhs.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        _lib.lexls_lse_solve_rhs_device.restype = C.c_int
        _lib.lexls_lse_solve_rhs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]  # d_rhs, d_fixed, nrhs, d_x
        _lib.lexls_lse_residual_rhs.restype = C.c_int
        _lib.lexls_lse_residual_rhs.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32]  # h_rhs, h_fixed, nrhs
        _lib.lexls_lse_get_residual_rhs.restype = C.c_int
        _lib.lexls_lse_get_residual_rhs.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]  # h_v, h_cost
        _lib.lexls_lse_residual_rhs_device.restype = C.c_int
        _lib.lexls_lse_residual_rhs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]  # d_rhs, d_fixed, nrhs, d_x, d_v, d_cost
        _lib.lexls_internal_apply_solve_map.restype = C.c_int
        _lib.lexls_internal_apply_solve_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]  # d_rhs, d_out: device addresses
        _lib.lexls_lsi_batch_solve_adjoint_multi.restype = C.c_int
        _lib.lexls_lsi_batch_solve_adjoint_multi.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib.lexls_lsi_batch_solve_adjoint_multi_device.restype = C.c_int
        _lib.lexls_lsi_batch_solve_adjoint_multi_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]  # d_G, ncot, d_grad_lb, d_grad_ub
        _lib.lexls_lsi_batch_solve_adjoint_matrix.restype = C.c_int
        _lib.lexls_lsi_batch_solve_adjoint_matrix.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        _lib.lexls_lsi_batch_solve_tangent.restype = C.c_int
        _lib.lexls_lsi_batch_solve_tangent.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        _lib.lexls_lsi_batch_solve_tangent_device.restype = C.c_int
        _lib.lexls_lsi_batch_solve_tangent_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]  # d_ddata, ntan, d_dx, d_differentiable
        _lib.lexls_lsi_batch_solve_bounds.restype = C.c_int
        _lib.lexls_lsi_batch_solve_bounds.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                      C.POINTER(C.c_uint8)]  # h_lb, h_ub, nrhs, h_x, h_violation, h_valid
        _lib.lexls_lsi_batch_solve_bounds_device.restype = C.c_int
        _lib.lexls_lsi_batch_solve_bounds_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]  # d_lb, d_ub, nrhs, d_x, d_violation, d_valid
        _lib.lexls_lsi_batch_solve_bounds_cost.restype = C.c_int
        _lib.lexls_lsi_batch_solve_bounds_cost.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                           C.POINTER(C.c_double), C.POINTER(C.c_uint8)]  # h_lb, h_ub, nrhs, h_x, h_violation, h_cost, h_valid
        _lib.lexls_lsi_batch_solve_bounds_cost_device.restype = C.c_int
        _lib.lexls_lsi_batch_solve_bounds_cost_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                  C.c_void_p]  # d_lb, d_ub, nrhs, d_x, d_violation, d_cost, d_valid
        _lib.lexls_lsi_batch_last_consumer_kernel.restype = C.c_char_p
        _lib.lexls_lsi_batch_last_consumer_kernel.argtypes = [C.c_void_p]
        _lib.lexls_lsi_batch_final_factorizations.restype = C.c_int
        _lib.lexls_lsi_batch_final_factorizations.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        _lib.lexls_lsi_batch_solve_adjoint_matrix_device.restype = C.c_int
        _lib.lexls_lsi_batch_solve_adjoint_matrix_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # d_g, d_grad_data, d_differentiable
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise LexlsError(f"liblexls_hip error {rc}: {lib().lexls_last_error().decode()}")
