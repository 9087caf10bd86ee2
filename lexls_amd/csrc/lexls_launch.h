// Host-side launchers of the liblexls_hip kernels (one per translation unit that defines kernels).
#pragma once
#include "lexls_kernels.h"
#include "lexls_dispatch.h" // (which kernel: plan_lqr; the LDS formulas: lexls_lds.h)

namespace lexls
{
    template <typename K>
    inline hipError_t set_lds(K kernel, size_t bytes) // a launcher's request for dynamic LDS: above the 64 KiB every kernel may have, the kernel is told so
    {
        return bytes <= 64 * 1024 ? hipSuccess : hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    }
    // lqr_generic.hip — any shape, one workgroup per problem (id: one of the generic_* forms, dispatch::generic_choice)
    hipError_t launch_lqr_generic(LseArgs a, uint32_t max_rows, KernelId id, bool write_factor, bool do_solve, hipStream_t s);
    // lse_postfactor.hip — solve() and the residuals on a kept factor
    // (variant, where given: the name of the kernel variant launched — lexls_lse_last_consumer_kernel; host bookkeeping only)
    hipError_t launch_solve_generic(const LseArgs &a, hipStream_t s, bool reciprocal_diagonal = false, const char **variant = nullptr);
    hipError_t launch_residual(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    // lse_adjoint.hip — the adjoint family of the kept factor (the view and the trust rule its kernels share: lse_kept_factor.h)
    /// the work buffer launch_solve_adjoint needs for a regularized factor whose matrices do not fit in LDS (0 where none is needed)
    size_t adjoint_reg_work_bytes(const LseArgs &a);
    /// lexls_lse_solve_adjoint: d_grad_rhs (batch x cap) = M^T g, d_grad_fixed (batch x nVar, may be NULL) = N^T g for x = M b + N x_fixed of the
    /// kept factor; d_g is batch x nVar in the order of x.  One wavefront per problem, enqueued only.  a.reg_type == 0: solve_adjoint_kernel.  A
    /// regularized factor of type 1, 3, 4, 5, 8 or 9 with a.reg_variable == 0 (anything else: hipErrorInvalidValue): solve_adjoint_reg_kernel, M and
    /// N those of the damped solve with a.reg_factor (read at the time of this call) held fixed; its matrices sit in LDS when adjoint_reg_in_lds
    /// (lexls_lds.h) says so, else in d_work (adjoint_reg_work_bytes)
    hipError_t launch_solve_adjoint(const LseArgs &a, const double *d_g, double *d_grad_rhs, double *d_grad_fixed, hipStream_t s, const char **variant = nullptr,
                                    double *d_work = nullptr);
    /// lexls_lse_solve_adjoint_multi: ncot cotangents per problem in one pass, d_G batch x ncot x nVar, d_grad_rhs batch x ncot x cap, d_grad_fixed
    /// batch x ncot x nVar (may be NULL).  The form follows from the shape (adjoint_multi_form, lexls_lds.h): lane = cotangent with the factor staged
    /// in LDS, the same with the factor read where it is kept, or launch_solve_adjoint once per cotangent through d_work (adjoint_multi_work_bytes,
    /// 0 where the shape needs none).  Enqueued only.
    /// A regularized factor (the types and the condition of launch_solve_adjoint; anything else: hipErrorInvalidValue) takes one of
    /// adjoint_reg_multi_form's forms (lexls_lds.h), from nVar, cap and nObj alone: solve_adjoint_reg_multi_kernel with the problem's matrices in
    /// LDS, the same with them in d_reg_multi_work (adjoint_reg_multi_work_bytes: one set per problem and TILE of 64 cotangents — the grid is batch x
    /// tiles and every tile repeats the work of the problem: basis, snapshots, D and its factorization), or launch_solve_adjoint once per
    /// cotangent through d_work, with d_reg_work what that launch wants (adjoint_reg_work_bytes).  a.reg_factor is read at the time of this call.
    /// LEXLS_ADJOINT_REG_MULTI_FORM = hbm | single in the environment names a later form of the list (measurements)
    size_t adjoint_multi_work_bytes(const LseArgs &a);
    size_t adjoint_reg_multi_work_bytes(const LseArgs &a, uint32_t ncot);
    hipError_t launch_solve_adjoint_multi(const LseArgs &a, const double *d_G, uint32_t ncot, double *d_grad_rhs, double *d_grad_fixed, double *d_work, hipStream_t s,
                                          const char **variant = nullptr, double *d_reg_work = nullptr, double *d_reg_multi_work = nullptr);
    /// d_out (batch x nVar, the order of x) = M d_rhs (batch x cap, LOD row order) for x = M b + N x_fixed of the kept factor, fixed values zero:
    /// the transpose of launch_solve_adjoint.  d_only_level (may be NULL): rows outside level d_only_level[b] of problem b count as zero.
    /// One wavefront per problem, enqueued only.  Internal (the matrix gradient's u); the public forward entry is launch_solve_rhs
    hipError_t launch_apply_solve_map(const LseArgs &a, const double *d_rhs, const int32_t *d_only_level, double *d_out, hipStream_t s);
    /// lexls_lse_solve_rhs: d_x (nrhs x batch x nVar, the order of x) = M d_rhs + N d_fixed for x = M b + N x_fixed of the kept factor, d_rhs
    /// nrhs x batch x cap (LOD row order; rows behind a problem's own are not read), d_fixed nrhs x batch x nVar (slot j < nfixed; NULL: a.fixed_val
    /// for every right-hand side).  Every problem is served (no rank-stability rule); a.x is not read.  Chains, in the stream: solve_rhs_front_kernel
    /// (R = rhs - A_fixed fixed, the fixed slots), then
    ///     a.reg_type == 0: apply_solve_map_kernel (nrhs == 1) or apply_solve_map_multi_kernel under tangent_map_placement (lexls_lds.h);
    ///     a regularized factor of type 1, 3, 4, 5, 8 or 9 with a.reg_variable == 0 (anything else: hipErrorInvalidValue):
    ///     apply_solve_map_reg_multi_kernel under solve_rhs_reg_form (every nrhs), a.reg_factor read at the time of this call.
    /// Everything they write besides d_x goes to d_work (solve_rhs_work_bytes for this nrhs).  Enqueued only; no atomics
    /// LEXLS_TANGENT_PLACEMENT = lds | work (plain) and LEXLS_SOLVE_RHS_REG_FORM = hbm | work (damped) in the environment name a later placement
    /// of the list (measurements and tests; nothing moves a shape up)
    size_t solve_rhs_work_bytes(const LseArgs &a, uint32_t nrhs);
    hipError_t launch_solve_rhs(const LseArgs &a, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x, void *d_work, hipStream_t s,
                                const char **variant = nullptr);
    /// lexls_lse_residual_rhs: for the right-hand sides and fixed values of launch_solve_rhs on an UNDAMPED kept factor (a.reg_type != 0:
    /// hipErrorInvalidValue), d_v (nrhs x batch x cap, LOD row order, zeros behind a problem's own rows) = get_v() of each, d_cost (nrhs x batch x
    /// nObj) = the sum of squares of each level's rows of it, d_x = launch_solve_rhs's x, bit for bit; each may be NULL, not all.  Chains, in the
    /// stream: solve_rhs_front_kernel, then residual_rhs_kernel under tangent_map_placement — launch_solve_rhs's pass with the residuals formed
    /// behind it on the same state (nrhs == 1 with d_x: apply_solve_map_kernel for x in front of it, as launch_solve_rhs takes it).  Everything
    /// else they write goes to d_work (residual_rhs_work_bytes for this nrhs).  Enqueued only; no atomics
    size_t residual_rhs_work_bytes(const LseArgs &a, uint32_t nrhs);
    hipError_t launch_residual_rhs(const LseArgs &a, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x, double *d_v, double *d_cost, void *d_work,
                                   hipStream_t s, const char **variant = nullptr);
    /// lexls_lse_solve_adjoint_matrix: d_grad_lod (batch x (nVar + 1) x cap, the layout of the problem data) = the gradient with respect to A and
    /// b for the cotangent d_g (batch x nVar), d_differentiable (batch bytes, may be NULL) = the rank-stability flags; a.x holds the solution of the
    /// kept factor.  Chains, in the stream: launch_solve_adjoint (y), the level search (k*), launch_sensitivity for level k* (lambda; its own rows
    /// are the residual), launch_apply_solve_map (u) and the assembly — everything they write goes to d_work (adjoint_matrix_work_bytes): a.lambda,
    /// a.v, a.sens, a.maxabs and the activation types stay as they are.  d_grad_fixed (batch x nVar, may be NULL: what the public calls pass) =
    /// N^T g, from the chain's own launch_solve_adjoint (lexls_lsi_batch_solve_adjoint_matrix routes it to the simple bounds).  Enqueued only
    size_t adjoint_matrix_work_bytes(const LseArgs &a);
    hipError_t launch_solve_adjoint_matrix(const LseArgs &a, const double *d_g, double *d_grad_lod, uint8_t *d_differentiable, void *d_work, uint32_t sweep_level_dim_hint,
                                           hipStream_t s, const char **variant = nullptr, double *d_grad_fixed = nullptr);
    /// lexls_lse_solve_tangent: d_dx (ntan x batch x nVar) = the tangents of x along the directions d_dlod (ntan x batch x the layout of the
    /// problem data, [dA | db]; rows behind a problem's own are not read) and d_dfixed (ntan x batch x nVar, slot j < nfixed; may be NULL: zeros),
    /// d_differentiable (batch bytes, may be NULL) = launch_solve_adjoint_matrix's flags; a.x holds the solution of the kept factor.
    ///     dx = M [(db - dA x - A_fixed dfixed) - E_k* M^T (dA^T lambda)] on the pivot variables, dfixed on the fixed ones, 0 on the free
    /// Chains, in the stream: the level search (k*), launch_sensitivity for level k* (lambda), tangent_rhs_kernel (the one pass over d_dlod: r and
    /// w), launch_solve_adjoint (ntan == 1) or launch_solve_adjoint_multi (M^T w; d_adjoint_multi_work: what that launch wants,
    /// adjoint_multi_work_bytes), apply_solve_map_multi_kernel with the per-lane vectors where tangent_map_placement (lexls_lds.h) puts them.
    /// Everything they write goes to d_work (tangent_work_bytes for this ntan).  Enqueued only; no atomics
    size_t tangent_work_bytes(const LseArgs &a, uint32_t ntan);
    hipError_t launch_solve_tangent(const LseArgs &a, const double *d_dlod, const double *d_dfixed, uint32_t ntan, double *d_dx, uint8_t *d_differentiable, void *d_work,
                                    double *d_adjoint_multi_work, uint32_t sweep_level_dim_hint, hipStream_t s, const char **variant = nullptr);
    // lse_postfactor.hip — the sensitivity, multiplier and least-norm kernels
    hipError_t launch_sensitivity(const LseArgs &a, const int32_t *d_obj_index, int32_t obj_all, double tolW, double tolC, hipStream_t s, bool scan_up = false,
                                  uint32_t sweep_level_dim_hint = 0, // hint = largest level dimension of the batch (enables the single-sweep kernel)
                                  bool collect = false,              // the wrong-sign SET into a.wrong_sign instead of one candidate (lexls_lse_sensitivity_collect)
                                  const char **variant = nullptr);
    bool sensitivity_sweep_serves(const LseArgs &a, uint32_t sweep_level_dim_hint); // launch_sensitivity takes the one-wavefront-per-problem sweep for these arguments
    /// lexls_lse_multipliers: d_out = batch x nObj x (nVar + cap), column k = the [lambda_fixed; lambda] of ObjectiveSensitivity(k).  One launch of the
    /// sweep's emitting form where multipliers_sweep_serves, else nObj sensitivity_kernel launches (d_scratch: multipliers_scratch_bytes)
    bool multipliers_sweep_serves(const LseArgs &a, uint32_t sweep_level_dim_hint);
    size_t multipliers_scratch_bytes(const LseArgs &a);
    /// *out = a with lambda | maxabs | sens | ctr_type | fixed_type carved out of d_scratch (multipliers_scratch_bytes counts them in this order; THE layout, for
    /// launch_multipliers and launch_solve_adjoint_matrix) and the copies of the two type arrays enqueued (the launch marks them; the handle's own stay); wrong_sign as in a
    hipError_t sensitivity_scratch_args(const LseArgs &a, void *d_scratch, hipStream_t s, LseArgs *out);
    hipError_t launch_multipliers(const LseArgs &a, double *d_out, uint32_t sweep_level_dim_hint, hipStream_t s, void *d_scratch, bool *swept, const char **variant = nullptr);
    hipError_t launch_leastnorm(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    hipError_t launch_leastnorm2(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    hipError_t launch_leastnorm3(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    hipError_t launch_gather_rows(const LseArgs &a, const double *d_cdata, uint64_t per_problem, const uint32_t *d_row_src, const uint32_t *d_row_ld,
                                  double *d_dst, hipStream_t s);

    // lqr_small.hip — the kernel table: the launcher of every LEXLS_KERNEL_LIST entry behind one signature
    struct FusedCall // what the persistent LexLSI launch (lsi_fused_impl.h) takes besides the problem: the driver's ResidentArgs (lexls_lsi_device.h), at most `count` iterations
    {
        uint32_t sweep_level_dim;
        const int32_t *d_obj_index;
        double tolW, tolC;
        bool scan_up;
        const void *resident_args;
        size_t resident_args_bytes;
        int count;
    };
    struct LaunchExtras
    {
        double *est              = nullptr; // estimating lqr_qtol: batch doubles
        uint32_t *ind            = nullptr; // ... its compaction counter (cleared); indirect lqr_quad: [count, problem list]
        const FusedCall *fused   = nullptr;
        uint32_t *reg_cfg        = nullptr; // out, regularized lqr_wave: the reg_cfg the kernel was launched with (lexls_lse_last_reg_placement; host bookkeeping only)
    };
    /// hipErrorNotSupported for ids the table has no launcher for (none, lqr_generic, lqr_large); the persistent launch also returns it when
    /// its LDS does not fit (the caller enqueues the three kernels per stage instead)
    hipError_t launch_kernel(KernelId id, const LseArgs &a, hipStream_t s, const LaunchExtras &x = LaunchExtras());
    size_t wave_reg_lds_share();       // DispatchQuery::reg_lds_share (environment, read once)
    uint32_t resident_wave_capacity(); // DispatchQuery::wave_capacity (current device)

    // lexls_guard.hip — the accuracy guard's compaction: status[b] from est[b] against the threshold (1 below it; 2 flagged, mode 1; 3 flagged,
    // mode 2) and, in mode 2, ind = [count, flagged problems] (ind[0] cleared by the estimating kernel in front of it in the stream)
    hipError_t launch_guard_compact(const double *est, uint8_t *status, uint32_t *ind, uint32_t batch, double threshold, int mode, hipStream_t s);
    // ... and the report of a bit-exact solve under a skip mask: estimate 0 and status 0 where skip[b] == 0, a skipped problem's report kept
    hipError_t launch_guard_clear(double *est, uint8_t *status, const uint8_t *skip, uint32_t batch, hipStream_t s);

    // lqr_large.hip — problems too large for one CU's LDS: one launch per stage, the whole chip per problem
    size_t large_state_bytes(uint32_t batch);
    hipError_t launch_lqr_large(const LseArgs &a, const uint32_t *h_level_max, uint32_t h_rows_max, void *d_state, double *d_norms, hipStream_t s);
    size_t large_fast_workspace_bytes(uint32_t batch, uint32_t n, uint32_t cap, uint32_t maxdim);
    /// levels (where given): {levels the one-launch form committed, levels it gave up and the host redid pivot by pivot} — lexls_lse_last_large_levels;
    /// host bookkeeping only
    hipError_t launch_lqr_large_fast(const LseArgs &a, const uint32_t *h_level_max, uint32_t h_rows_max, void *d_workspace, hipStream_t s, uint32_t *levels = nullptr);
} // namespace lexls
