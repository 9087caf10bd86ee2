// Host-side launchers of the liblexls_hip kernels (one per translation unit that defines kernels).
#pragma once
#include "lexls_kernels.h"

namespace lexls
{
    /// maximum dynamic LDS one workgroup may ask for on gfx950 (160 KiB per CU)
    constexpr size_t kMaxLdsBytes = 160 * 1024;

    /// odd leading dimension >= rows for the LDS image (conflict-free column-per-lane access)
    inline uint32_t odd_ld(uint32_t rows) { return rows | 1u; }

    // lqr_generic.hip — any shape, one workgroup per problem
    hipError_t launch_lqr_generic(LseArgs a, uint32_t max_rows, bool write_factor, bool do_solve, hipStream_t s, const char **variant);
    // (variant, where given: the name of the kernel variant launched — lexls_lse_last_consumer_kernel; host bookkeeping only)
    hipError_t launch_solve_generic(const LseArgs &a, hipStream_t s, bool reciprocal_diagonal = false, const char **variant = nullptr);
    hipError_t launch_residual(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    hipError_t launch_sensitivity(const LseArgs &a, const int32_t *d_obj_index, int32_t obj_all, double tolW, double tolC, hipStream_t s, bool scan_up = false,
                                  uint32_t sweep_level_dim_hint = 0, // hint = largest level dimension of the batch (enables the single-sweep kernel)
                                  bool collect = false,              // the wrong-sign SET into a.wrong_sign instead of one candidate (lexls_lse_sensitivity_collect)
                                  const char **variant = nullptr);
    bool sensitivity_sweep_serves(const LseArgs &a, uint32_t sweep_level_dim_hint); // launch_sensitivity takes the one-wavefront-per-problem sweep for these arguments
    /// lexls_lse_multipliers: d_out = batch x nObj x (nVar + cap), column k = the [lambda_fixed; lambda] of ObjectiveSensitivity(k).  One launch of the
    /// sweep's emitting form where multipliers_sweep_serves, else nObj sensitivity_kernel launches (d_scratch: multipliers_scratch_bytes)
    bool multipliers_sweep_serves(const LseArgs &a, uint32_t sweep_level_dim_hint);
    size_t multipliers_scratch_bytes(const LseArgs &a);
    hipError_t launch_multipliers(const LseArgs &a, double *d_out, uint32_t sweep_level_dim_hint, hipStream_t s, void *d_scratch, bool *swept, const char **variant = nullptr);
    hipError_t launch_leastnorm(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    hipError_t launch_leastnorm2(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    hipError_t launch_leastnorm3(const LseArgs &a, hipStream_t s, const char **variant = nullptr);
    hipError_t launch_gather_rows(const LseArgs &a, const double *d_cdata, uint64_t per_problem, const uint32_t *d_row_src, const uint32_t *d_row_ld,
                                  double *d_dst, hipStream_t s);

    // lqr_small.hip — dispatch of the shape kernels (n+1 <= 64, level dims <= 16): one wavefront per problem with the problem in VGPRs, the
    // left-looking forms (one or four problems per wavefront, any number of rows), the tolerance-contract kernels
    bool wave_kernel_supports(const LseArgs &a, uint32_t max_rows, uint32_t max_level_dim, bool has_fixed);
    bool deep_kernel_supports(const LseArgs &a, uint32_t max_level_dim, bool write_factor, bool has_fixed);
    bool wave_dispatch_is_register_resident(const LseArgs &a, uint32_t max_level_dim, bool has_fixed, int left_looking);
    bool wave_reg_kernel_fits(const LseArgs &a, uint32_t max_level_dim);
    size_t wave_reg_lds_share();
    /// tolerance: x-only solves of the shapes lqr_mfma_impl.h / lqr_qtol_impl.h serve may take those kernels (pivots / ranks exact, x within 1e-10
    /// instead of bit-identical to the oracle).  0 = bit-exact kernels only; 1 = automatic (lqr_qtol where it serves, else lqr_mfma); 6 = lqr_qtol
    /// only; 7 / 8 / 9 = lqr_mfma with two / one / four problems per wavefront, else lqr_qtol; 10 = as 6, and lqr_qtol's ragged instantiations
    /// (levels of at most 12 rows, per-problem dimensions) where the uniform ones do not serve
    /// guard (NULL: off): the accuracy guard's device arrays (lexls_lse_set_accuracy_guard).  With a guard, lqr_qtol runs as its estimating
    /// instantiation (est: batch doubles; ind[0], the compaction counter, is cleared) and *variant names it with ",guard"
    struct GuardArrays
    {
        double *est;   // batch: the estimate
        uint8_t *status; // batch
        uint32_t *ind; // 1 + batch: [count, problems flagged for the re-solve]
    };
    hipError_t launch_lqr_wave(const LseArgs &a, uint32_t max_level_dim, bool write_factor, bool has_fixed, int left_looking, hipStream_t s,
                               const char **variant, int tolerance = 0, const GuardArrays *guard = nullptr);
    /// the guard's re-solve (mode 2): the bit-exact x-only four-per-wavefront instantiation policy 4 takes for these arguments, in its indirect
    /// form over ind = [count, list]; hipErrorNotSupported where policy 4 would take no four-per-wavefront kernel
    hipError_t launch_quad_resolve(const LseArgs &a, uint32_t max_level_dim, const uint32_t *ind, hipStream_t s);

    // lexls_guard.hip — the accuracy guard's compaction: status[b] from est[b] against the threshold (1 below it; 2 flagged, mode 1; 3 flagged,
    // mode 2) and, in mode 2, ind = [count, flagged problems] (ind[0] cleared by the estimating kernel in front of it in the stream)
    hipError_t launch_guard_compact(const double *est, uint8_t *status, uint32_t *ind, uint32_t batch, double threshold, int mode, hipStream_t s);

    /// The resident active-set iterations of a lock-step LexLSI batch as one persistent launch (lsi_fused_impl.h): l-QR (the register-resident wave
    /// kernel's body, rows gathered by reference) -> removal sweep -> iteration, per instance until it stops or `count` iterations are done.
    /// resident_args: the driver's ResidentArgs (lexls_lsi_device.h).  hipErrorNotSupported: the shape has no persistent instantiation (the caller
    /// enqueues the three kernels per stage instead); the conditions are those under which launch_lqr_wave(a, ..., factor kept, left_looking < 0)
    /// takes the same register-resident instantiation and launch_sensitivity the sweep.  a.reg_type != 0: the launch whose l-QR phase is the
    /// regularized body (every type but 7); a.reg_factor / a.reg_scratch are on the device already; it neither reads nor leaves prefix-reuse state
    hipError_t launch_lsi_fused(const LseArgs &a, uint32_t max_level_dim, bool has_fixed, const int32_t *d_obj_index, double tolW, double tolC, bool scan_up,
                                const void *resident_args, size_t resident_args_bytes, int count, hipStream_t s, const char **variant);

    // lqr_large.hip — problems too large for one CU's LDS: one launch per stage, the whole chip per problem
    bool generic_fits_lds(const LseArgs &a, uint32_t max_rows);
    bool large_kernel_supports(const LseArgs &a, uint32_t max_level_dim, bool has_fixed);
    size_t large_state_bytes(uint32_t batch);
    hipError_t launch_lqr_large(const LseArgs &a, const uint32_t *h_level_max, uint32_t h_rows_max, void *d_state, double *d_norms, hipStream_t s);
    size_t large_fast_workspace_bytes(uint32_t batch, uint32_t n, uint32_t cap, uint32_t maxdim);
    hipError_t launch_lqr_large_fast(const LseArgs &a, const uint32_t *h_level_max, uint32_t h_rows_max, void *d_workspace, hipStream_t s);
} // namespace lexls
