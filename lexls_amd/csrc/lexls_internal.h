// Functions that cross the translation units of liblexls_hip without being part of its ABI: defined in lexls_capi.hip, called by the lock-step LexLSI
// driver.  Declared HERE ONLY — they are extern "C", so a declaration written by hand elsewhere would link against a changed parameter list without a diagnostic.
#pragma once
#include "../../include/lexls_hip.h"

extern "C"
{
    /// lets the other translation units of the library report through lexls_last_error()
    void lexls_internal_set_error(const char *msg);
    /// lexls_lse_upload_round without the per-element argument checks: the driver fills the block from its own working sets
    int lexls_internal_upload_round_trusted(lexls_lse_t h, const void *h_in, int gather);
    /// the resident constraint data (lexls_lse_set_constraint_data), read by the driver's step kernels
    const double *lexls_internal_cdata(lexls_lse_t h);
    /// lexls_lse_set_constraint_data from memory of the handle's device: a device-to-device copy, only ENQUEUED in the handle's stream
    int lexls_internal_set_constraint_data_device(lexls_lse_t h, const double *d_data, uint64_t per_problem);
    /// the buffer gathered rows go to exists (a handle that never uploaded a round has none; lexls_internal_round_resident needs it)
    int lexls_internal_ensure_gather_buffer(lexls_lse_t h);
    /// the same for the resident iterations of a run with cycling handling, which relax bounds in it (every run uploads the data anew)
    double *lexls_internal_cdata_writable(lexls_lse_t h);
    /// the device copy of the in slab (lexls_lse_round_layout): the resident iterations write the next equality problem there themselves
    char *lexls_internal_round_in(lexls_lse_t h);
    /// the in slab was written ON THE DEVICE (same stream): gather the rows it names; kernel choice follows the capacities given at creation
    int lexls_internal_round_resident(lexls_lse_t h, int has_fixed);
    /// the device array the resident iterations write the changed levels into (NULL: prefix reuse off, or a regularized handle)
    int32_t *lexls_internal_resume_levels(lexls_lse_t h);
    /// the promise that lexls_internal_resume_levels holds the levels for the next factorization
    void lexls_internal_arm_resume(lexls_lse_t h);
    /// the regularization of ONE run (type 1 .. 9, one factor per LexLSE level for every problem), only ENQUEUED in the handle's stream
    int lexls_internal_set_regularization_block(lexls_lse_t h, int type, const double *h_level_factors, double variable_factor, uint32_t cg_iterations);
    /// the same with factors of its own for every problem (h_factors: batch x nObj, problem-major)
    int lexls_internal_set_regularization_block_per_problem(lexls_lse_t h, int type, const double *h_factors, double variable_factor, uint32_t cg_iterations);
    /// the same without factors: the caller writes them into *d_factors (batch x nObj, the array the kernels read) in the handle's stream
    int lexls_internal_set_regularization_block_device(lexls_lse_t h, int type, double variable_factor, uint32_t cg_iterations, double **d_factors);
    /// 1 when the resident iterations of this handle's batch can run under regularization `type` (nothing is launched, nothing changes)
    int lexls_internal_resident_reg_serves(lexls_lse_t h, int type);
    /// ALL remaining resident iterations in one persistent launch (resident_args: a ResidentArgs); 1 = the shape has none, nothing changed
    int lexls_internal_resident_fused(lexls_lse_t h, int has_fixed, int count, double tolW, double tolC, const void *resident_args, size_t resident_args_bytes);
    /// 1 when lexls_internal_resident_fused would take the launch for a run of regularization `type` (0: none); resident_lds: the driver's LDS per
    /// instance (resident_lds_per_wave).  A pure predicate: nothing is launched, nothing changes
    int lexls_internal_resident_fused_serves(lexls_lse_t h, int has_fixed, int type, size_t resident_lds);
    /// the device buffer lexls_lse_multipliers filled last (NULL: none valid), and whether the sweep served it
    const double *lexls_internal_multipliers(lexls_lse_t h, int *swept);
    /// the handle's kernel policy (lexls_lse_set_kernel_policy), to put it back after a change
    int lexls_internal_kernel_policy(lexls_lse_t h);
    /// d_out (batch x nVar, the order of x) = M d_rhs (batch x cap, LOD row order) for x = M b + N x_fixed of the kept, unregularized factor, fixed
    /// values zero (apply_solve_map_kernel, the piece of lexls_lse_solve_adjoint_matrix that has no public entry); both in device memory, enqueued only
    int lexls_internal_apply_solve_map(lexls_lse_t h, const double *d_rhs, double *d_out);
    /// lexls_lse_solve_adjoint_matrix_device with N^T g as a further output (d_grad_fixed: batch x nVar, fixVariable order, zero from nfixed on; may
    /// be NULL) from the chain's own solve_adjoint launch: what lexls_lsi_batch_solve_adjoint_matrix routes to the active simple bounds
    int lexls_internal_solve_adjoint_matrix(lexls_lse_t h, const double *d_g, double *d_grad_lod, double *d_grad_fixed, uint8_t *d_differentiable);
}
