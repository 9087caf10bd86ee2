// Dynamic-LDS byte formulas of the LexLSE kernels: ONE function per formula, read by each kernel's launcher (its carve-up must match) and by
// the dispatch plan (lexls_dispatch.h: "does the shape fit").  Plain host arithmetic, no device code: compiles with any C++17 compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef QT_WPB
#define QT_WPB 4 // wavefronts per workgroup of lqr_qtol (1 or 4)
#endif

namespace lexls
{
    /// maximum dynamic LDS one workgroup may ask for on gfx950 (160 KiB per CU)
    constexpr size_t kMaxLdsBytes = 160 * 1024;

    /// odd leading dimension >= rows for the LDS image (conflict-free column-per-lane access)
    inline uint32_t odd_ld(uint32_t rows) { return rows | 1u; }

    constexpr int kQuadMaxObj = 8; // levels: one byte per level in a column's 64-bit image-index word
    constexpr int kMfMaxObj   = 8;
    constexpr int SWEEP_MD    = 16; // rows per level of the sensitivity sweep
    constexpr size_t kGenericSharedBytes = 40; // sizeof(Shared) of lqr_generic.hip (asserted there)

    // ---- lqr_quad (lqr_quad_impl.h) ----
    /// exact worst case of sum_k (n+1-Fc_k) * rank_k over rank distributions with rank_k <= md
    inline uint32_t quad_image_doubles(uint32_t n, uint32_t nObj, uint32_t md)
    {
        uint32_t fc = 0, total = 0;
        for (uint32_t k = 0; k < nObj && fc < n; k++)
        {
            const uint32_t r = md < n - fc ? md : n - fc;
            total += (n + 1 - fc) * r;
            fc += r;
        }
        return (total + 1) & ~1u;
    }

    template <int NS>
    inline size_t quad_group_bytes(uint32_t n, uint32_t nObj, uint32_t md)
    {
        return (8 * ((size_t)quad_image_doubles(n, nObj, md) + 16 * NS + 18) + 64 + 64 + 16 * kQuadMaxObj + 512 + 4 * kQuadMaxObj + 15) & ~(size_t)15;
    }

    /// dynamic LDS one wavefront (four problems) of the four-per-wavefront kernel asks for; 0 = the shape is not served
    inline size_t quad_lds_bytes(uint32_t slots, uint32_t md, uint32_t nVar, uint32_t nObj)
    {
        if (nObj > (uint32_t)kQuadMaxObj || nVar + 1 > 16u * slots || nVar > 63u) return 0;
        const size_t g = slots == 3 ? quad_group_bytes<3>(nVar, nObj, md) : quad_group_bytes<4>(nVar, nObj, md);
        return 4 * g;
    }

    // ---- lqr_qtol (lqr_qtol_impl.h) ----
    /// exact worst case of the triangular images: sum_k ((n+1-Fc_k) rank_k - rank_k (rank_k - 1) / 2) over rank distributions with rank_k <= md
    inline uint32_t qtol_image_doubles(uint32_t n, uint32_t nObj, uint32_t md)
    {
        uint32_t fc = 0, total = 0;
        for (uint32_t k = 0; k < nObj && fc < n; k++)
        {
            const uint32_t r = md < n - fc ? md : n - fc;
            total += (n + 1 - fc) * r - r * (r - 1) / 2;
            fc += r;
        }
        return (total + 1) & ~1u;
    }

    template <int NS, int MD>
    inline size_t qtol_group_bytes(uint32_t n, uint32_t nObj)
    {
        // staging block: the level pieces (half the rows at a time) or the sixteen hand-off slots of the pivot steps, whichever is larger
        const size_t stage = 8 * (size_t)(n + 1) * (MD / 2) > 16u * (8 * MD + 16) ? 8 * (size_t)(n + 1) * (MD / 2) : 16u * (8 * MD + 16);
        const size_t raw   = 8 * ((size_t)qtol_image_doubles(n, nObj, MD) + 16 * NS + MD) + 64 + 64 + 16 * kQuadMaxObj + 8 * 16 * NS + stage;
        // rounded up to an ODD multiple of 128 bytes: the four problems of a wavefront read the same relative addresses of their slices at
        // the same time; slices half a bank row apart do not collide
        return ((raw + 127) / 256) * 256 + 128;
    }

    /// dynamic LDS of one lqr_qtol workgroup (the ragged and estimating instantiations of a shape take what the uniform one takes)
    template <int NS, int MD>
    inline size_t qtol_lds_bytes(uint32_t n, uint32_t nObj) { return 4 * QT_WPB * qtol_group_bytes<NS, MD>(n, nObj); }

    // ---- lqr_mfma (lqr_mfma_impl.h) ----
    /// exact worst case of the reduced rows and their inverse maps: max over rank distributions (rank_k <= md, sum <= n) of
    /// sum_k rank_k S_k + ceil(S_k / 8), S_k = n + 1 - Fc_k - rank_k (n <= 64)
    inline uint32_t mfma_nd_doubles(uint32_t n, uint32_t nObj, uint32_t md)
    {
        // best[fc]: the most doubles the levels from the current one on can need when the current one starts at column fc
        uint32_t best[65], next[65];
        for (uint32_t fc = 0; fc <= n; fc++) next[fc] = 0;
        for (uint32_t k = nObj; k--;)
        {
            for (uint32_t fc = 0; fc <= n; fc++)
            {
                uint32_t m = 0;
                for (uint32_t r = 0; r <= md && fc + r <= n; r++)
                {
                    const uint32_t S = n + 1 - fc - r;
                    const uint32_t v = r * S + (r ? (S + 7) / 8 : 0) + next[fc + r]; // the rows and their inverse map
                    m                = v > m ? v : m;
                }
                best[fc] = m;
            }
            for (uint32_t fc = 0; fc <= n; fc++) next[fc] = best[fc];
        }
        return (next[0] + 1) & ~1u;
    }

    template <int MD>
    inline size_t mfma_group_bytes(uint32_t n, uint32_t nObj)
    {
        const size_t pfb = 8u * MD * (size_t)(n + 1) > 128u * MD ? 8u * MD * (size_t)(n + 1) : 128u * MD;
        const size_t raw = 8 * (size_t)mfma_nd_doubles(n, nObj, MD) + pfb + 8 * MD + 16 + 16 + 48 + 8 * (size_t)nObj + 8 * (size_t)(n + 1);
        // (no padding against bank conflicts between the problems of a wavefront: the LDS serves a wave's 8- and 16-byte accesses in lane groups
        // that never mix the two halves of the wavefront, MI355X_MICROARCH.md LDS table)
        return (raw + 15) & ~(size_t)15;
    }

    /// dynamic LDS of one lqr_mfma workgroup with LP lanes per problem
    template <int LP, int MD>
    inline size_t mfma_lds_bytes(uint32_t n, uint32_t nObj) { return 4 * (64 / LP) * mfma_group_bytes<MD>(n, nObj); }

    // ---- lqr_wave (lqr_small_impl.h) and the persistent LexLSI launch (lsi_fused_impl.h) ----
    /// doubles of the compact level images: worst case of sum_k (n+1-Fc_k) * even(rank_k) over rank distributions with rank_k <= MD
    template <int MD>
    inline uint32_t wave_img_doubles(uint32_t n, uint32_t nObj)
    {
        return (n * n) / 2 + n + (n * MD) / 2 + nObj * (n + 1) + 64 + MD * MD; // (+ zeros behind the last image: a padded level reads MD columns of it)
    }
    template <int NC, int MD>
    inline size_t wave_lds_bytes(uint32_t nObj, uint32_t img)
    {
        return 8 * ((size_t)NC * MD + 128 + img + 64) + 4 * (64 + 4 * (size_t)nObj) + 64 + 64 * (size_t)nObj + 128 + 16;
    }

    /// REG: what lqr_wave_body's regularization routines take of the LDS behind the plain carve-up of `lds` bytes (the sum is returned) and
    /// where the host found room for the optional pieces (reg_cfg, as the body reads it).  One rule for every launch that runs the body —
    /// lqr_wave_kernel and the persistent LexLSI launch (lsi_fused_impl.h):
    /// the routines' vectors always; then their work matrix (order bounded by the type: the damped triangle alone for R / R_NO_Z /
    /// RT_NO_Z, under n/2 + the largest level for TIKHONOV — tikhonov_2 is taken while Fc + rank <= n/2, tikhonov_1 has order n - Fc —,
    /// n for TIKHONOV_2) and the null-space basis, each while LEXLS_REG_LDS_WAVES wavefronts (default 8: the occupancy is worth more than either, measured) still share a CU's LDS
    /// (share: wave_reg_lds_share(), lqr_small.hip — read from the environment ONCE per process, so that the driver's gate and every
    /// launcher place the same pieces)
    template <int MD>
    inline size_t wave_reg_lds_bytes(uint32_t n, uint32_t reg_type, size_t share, size_t lds, uint32_t &reg_cfg)
    {
        const bool cg = reg_type == 2 || reg_type == 6;
        lds           = ((lds + 15) & ~(size_t)15) + 16 + 8 * (2 * (size_t)n + 8 + (cg ? 10 * (size_t)n : 0));
        uint32_t order = 0;
        switch (reg_type)
        {
        case 3: case 4: case 5: order = MD; break;
        case 1: order = n / 2 + MD + 1 < n ? n / 2 + MD + 1 : n; break;
        case 8: order = n; break;
        default: break;
        }
        if (order > 255) order = 0;
        reg_cfg = 0;
        if (order && lds + 8 * (size_t)order * order <= share)
        {
            reg_cfg |= order;
            lds += 8 * (size_t)order * order;
        }
        const bool basis = reg_type == 1 || reg_type == 2 || reg_type == 3 || reg_type == 8;
        if (basis && lds + 8 * (size_t)(n | 1u) * (n + 1) <= share)
        {
            reg_cfg |= 0x100u;
            lds += 8 * (size_t)(n | 1u) * (n + 1);
        }
        return lds;
    }

    // ---- the sensitivity sweep (lexls_sweep_impl.h) ----
    inline size_t sweep_lds_bytes(uint32_t nVar, uint32_t cap);

    // ---- the persistent LexLSI launch (lsi_fused_impl.h) ----
    constexpr size_t kLsiFusedMaxLdsBytes = 64 * 1024;
    /// dynamic LDS of one workgroup of the <NC, MD> instantiation: the largest of its phases' — the l-QR's (reg_type != 0: with the regularization
    /// routines' pieces, reg_cfg as the body reads it), the removal sweep's and the driver's own (resident_lds: resident_lds_per_wave).  The ONE sum: the
    /// launcher launches with it and lexls_internal_resident_fused_serves decides on it; above kLsiFusedMaxLdsBytes the launch is not taken
    template <int NC, int MD>
    inline size_t lsi_fused_lds_bytes(uint32_t nVar, uint32_t nObj, uint32_t cap, uint32_t reg_type, size_t reg_share, size_t resident_lds, uint32_t &reg_cfg)
    {
        size_t lds = wave_lds_bytes<NC, MD>(nObj, wave_img_doubles<MD>(nVar, nObj));
        reg_cfg    = 0;
        if (reg_type != 0) lds = wave_reg_lds_bytes<MD>(nVar, reg_type, reg_share, lds, reg_cfg);
        const size_t l2 = sweep_lds_bytes(nVar, cap);
        lds             = lds > l2 ? lds : l2;
        return lds > resident_lds ? lds : resident_lds;
    }

    /// dynamic LDS of one sweep: staged factor, Householder scalars, multipliers / right-hand sides / fixed-variable multipliers of 8 objectives, types
    inline size_t sweep_lds_bytes(uint32_t nVar, uint32_t cap)
    {
        return 8 * ((size_t)(cap | 1u) * (nVar + 1) + cap + 8 * ((size_t)cap + 2 * nVar)) + (((size_t)cap + nVar + 15) & ~(size_t)15);
    }
    /// the shapes the one-wavefront-per-problem sweep serves (level_dim: the largest level of the batch; 0 = unknown)
    inline bool sweep_shape_serves(uint32_t nVar, uint32_t nObj, uint32_t cap, uint32_t reg_type, uint32_t level_dim)
    {
        return reg_type != 7 && level_dim > 0 && level_dim <= (uint32_t)SWEEP_MD && nObj <= 8 && nVar <= 64 && sweep_lds_bytes(nVar, cap) <= 64 * 1024;
    }

    // ---- lqr_generic (lqr_generic.hip) ----
    /// NT threads; ldsmat: the problem staged in LDS with leading dimension ldp (else it stays in HBM)
    inline size_t generic_lds_bytes(uint32_t ldp, uint32_t nVar, uint32_t nObj, int NT, bool ldsmat)
    {
        size_t b = 8 * ((ldsmat ? (size_t)ldp * (nVar + 1) : 0) + 2 * (size_t)nVar + NT);
        b += kGenericSharedBytes + 4 * ((size_t)NT + nVar + 3 * (size_t)nObj) + 16;
        return b;
    }

    // ---- solve_adjoint, apply_solve_map (lse_adjoint.hip) ----
    /// g in factor column order (nVar doubles), the gradient of the right-hand side with y inside it (cap doubles), the transpositions (nVar words)
    inline size_t adjoint_lds_bytes(uint32_t nVar, uint32_t cap) { return (8 * ((size_t)nVar + cap) + 4 * (size_t)nVar + 15) & ~(size_t)15; }

    // ---- solve_adjoint_multi (lse_adjoint.hip): lane = cotangent ----
    constexpr uint32_t kAdjointMultiLd = 65; // odd leading dimension of the per-lane state, stored [index][lane]
    /// the per-lane state gh (nVar) and cb (cap), [index][lane] with leading dimension 65; the transpositions and the position every variable
    /// reaches by them (2 x nVar words, shared by the lanes); staged: + the problem's factor without its right-hand-side column (odd leading
    /// dimension, as stage_factor — lse_kept_factor.h — writes it) and hh (cap doubles)
    inline size_t adjoint_multi_lds_bytes(uint32_t nVar, uint32_t cap, bool staged)
    {
        size_t b = 8 * (size_t)kAdjointMultiLd * ((size_t)nVar + cap) + 8 * (size_t)nVar;
        if (staged) b += 8 * ((size_t)odd_ld(cap) * nVar + cap);
        return (b + 15) & ~(size_t)15;
    }
    /// the fit rule of lexls_lse_solve_adjoint_multi, decided from the shape alone: state + staged factor in one workgroup's LDS; else the state
    /// alone (the factor read from global memory at wavefront-uniform addresses); else the single-cotangent kernel once per cotangent
    enum class AdjointMultiForm { staged, hbm, per_cotangent };
    inline AdjointMultiForm adjoint_multi_form(uint32_t nVar, uint32_t cap)
    {
        if (adjoint_multi_lds_bytes(nVar, cap, true) <= kMaxLdsBytes) return AdjointMultiForm::staged;
        if (adjoint_multi_lds_bytes(nVar, cap, false) <= kMaxLdsBytes) return AdjointMultiForm::hbm;
        return AdjointMultiForm::per_cotangent;
    }
    inline const char *adjoint_multi_form_name(AdjointMultiForm f)
    {
        return f == AdjointMultiForm::staged ? "solve_adjoint_multi<64,staged>" : f == AdjointMultiForm::hbm ? "solve_adjoint_multi<64,hbm>" : "solve_adjoint<64> x K";
    }

    // ---- solve_adjoint_reg (lse_adjoint.hip): the adjoint of a regularized solve ----
    /// the doubles of one problem's matrices: the null-space basis rebuilt from the factor (nVar x nVar), the work matrix D of the level's normal
    /// equations (order <= nVar), the snapshots of the basis at entry to each level — a level of non-zero rank keeps m0 x (nVar - Fc) entries,
    /// m0 <= Fc, so at most nVar^2 / 4, and there are at most min(nObj, nVar) such levels
    constexpr size_t adjoint_reg_matrix_doubles(uint32_t nVar, uint32_t nObj) // (constexpr: the kernel lays its work buffer out by it)
    {
        const size_t n = nVar, levels = nObj < nVar ? nObj : nVar;
        return 2 * n * n + levels * ((n / 2) * ((n + 1) / 2));
    }
    /// the vectors every form keeps in LDS: g in factor column order, the cotangent r of the basis' right-hand-side column, the level's
    /// right-hand side of D (nVar doubles each), the gradient of the right-hand side (cap doubles), the transpositions (nVar words);
    /// in_lds: + the matrices
    inline size_t adjoint_reg_lds_bytes(uint32_t nVar, uint32_t cap, uint32_t nObj, bool in_lds)
    {
        const size_t b = 8 * (3 * (size_t)nVar + cap + (in_lds ? adjoint_reg_matrix_doubles(nVar, nObj) : 0)) + 4 * (size_t)nVar;
        return (b + 15) & ~(size_t)15;
    }
    /// the fit rule of the regularized lexls_lse_solve_adjoint, decided from the shape alone: the matrices in one workgroup's LDS, else in a
    /// work buffer of the call (adjoint_reg_matrix_doubles per problem)
    inline bool adjoint_reg_in_lds(uint32_t nVar, uint32_t cap, uint32_t nObj) { return adjoint_reg_lds_bytes(nVar, cap, nObj, true) <= kMaxLdsBytes; }
    inline const char *adjoint_reg_form_name(bool in_lds) { return in_lds ? "solve_adjoint_reg<64,lds>" : "solve_adjoint_reg<64,hbm>"; }
    /// the regularization types whose damped solve is an affine map of the kept factor (TIKHONOV, R, R_NO_Z, RT_NO_Z, TIKHONOV_2, TEST)
    inline bool adjoint_reg_serves(uint32_t reg_type) { return reg_type == 1 || reg_type == 3 || reg_type == 4 || reg_type == 5 || reg_type == 8 || reg_type == 9; }

    // ---- solve_adjoint_reg_multi (lse_adjoint.hip): the adjoint of a regularized solve, lane = cotangent ----
    /// the per-lane state gh, the cotangent r~ of the basis' right-hand-side column, the level's right-hand side of D (nVar each) and cb (cap),
    /// [index][lane] with leading dimension 65; the transpositions and the position every variable reaches by them (2 x nVar words, shared by
    /// the lanes); in_lds: + the problem's matrices (adjoint_reg_matrix_doubles: the basis, D and the snapshots, shared by the lanes)
    inline size_t adjoint_reg_multi_lds_bytes(uint32_t nVar, uint32_t cap, uint32_t nObj, bool in_lds)
    {
        const size_t b = 8 * (size_t)kAdjointMultiLd * (3 * (size_t)nVar + cap) + 8 * (size_t)nVar + (in_lds ? 8 * adjoint_reg_matrix_doubles(nVar, nObj) : 0);
        return (b + 15) & ~(size_t)15;
    }
    /// the fit rule of the regularized lexls_lse_solve_adjoint_multi, decided from the shape alone: state + matrices in one workgroup's LDS; else
    /// the state alone, ALL THREE matrices (D too: one rule, one carve-up) in a work buffer of the handle, adjoint_reg_matrix_doubles per
    /// (problem, tile) and read at wavefront-uniform addresses; else the single-cotangent kernel once per cotangent
    enum class AdjointRegMultiForm { lds, hbm, per_cotangent };
    inline AdjointRegMultiForm adjoint_reg_multi_form(uint32_t nVar, uint32_t cap, uint32_t nObj)
    {
        if (adjoint_reg_multi_lds_bytes(nVar, cap, nObj, true) <= kMaxLdsBytes) return AdjointRegMultiForm::lds;
        if (adjoint_reg_multi_lds_bytes(nVar, cap, nObj, false) <= kMaxLdsBytes) return AdjointRegMultiForm::hbm;
        return AdjointRegMultiForm::per_cotangent;
    }
    /// (the per-cotangent form is named after the single-cotangent kernel it runs: adjoint_reg_in_lds of the same shape)
    inline const char *adjoint_reg_multi_form_name(AdjointRegMultiForm f, bool single_in_lds)
    {
        return f == AdjointRegMultiForm::lds   ? "solve_adjoint_reg_multi<64,lds>"
               : f == AdjointRegMultiForm::hbm ? "solve_adjoint_reg_multi<64,hbm>"
               : single_in_lds                 ? "solve_adjoint_reg<64,lds> x K"
                                               : "solve_adjoint_reg<64,hbm> x K";
    }

    // ---- apply_solve_map_multi (lse_adjoint.hip): the solve map on many right-hand sides, lane = right-hand side (lexls_lse_solve_tangent) ----
    /// where the per-lane vectors z (nVar) and t (cap) of a wavefront's 64 right-hand sides live: in LDS beside the staged factor, in LDS with
    /// the factor read where it is kept, or in a work buffer of the call ([index][lane], leading dimension 64: a lane's walk and the
    /// load and store phases both take consecutive words) where one workgroup's LDS does not hold them
    enum class TangentPlacement { staged, lds, work };
    constexpr uint32_t kTangentWorkLd = 64;
    /// the carve-up is solve_adjoint_multi's (z for gh, t for cb); the work placement keeps only the transpositions and the positions in LDS
    inline size_t tangent_map_lds_bytes(uint32_t nVar, uint32_t cap, uint32_t /*nObj*/, TangentPlacement p)
    {
        if (p == TangentPlacement::work) return (8 * (size_t)nVar + 15) & ~(size_t)15;
        return adjoint_multi_lds_bytes(nVar, cap, p == TangentPlacement::staged);
    }
    /// the placement rule of lexls_lse_solve_tangent, decided from the shape alone (the launcher and tests/tangent_fit_check.cpp read it here)
    inline TangentPlacement tangent_map_placement(uint32_t nVar, uint32_t cap, uint32_t nObj)
    {
        if (tangent_map_lds_bytes(nVar, cap, nObj, TangentPlacement::staged) <= kMaxLdsBytes) return TangentPlacement::staged;
        if (tangent_map_lds_bytes(nVar, cap, nObj, TangentPlacement::lds) <= kMaxLdsBytes) return TangentPlacement::lds;
        return TangentPlacement::work;
    }
    /// doubles of the work buffer per (problem, tile of 64 right-hand sides) under the work placement
    /// (constexpr: the kernel lays its work buffer out by it)
    constexpr size_t tangent_map_work_doubles(uint32_t nVar, uint32_t cap) { return (size_t)kTangentWorkLd * ((size_t)nVar + cap); }
    inline const char *tangent_placement_name(TangentPlacement p)
    {
        return p == TangentPlacement::staged ? "solve_tangent<64,staged>" : p == TangentPlacement::lds ? "solve_tangent<64,lds>" : "solve_tangent<64,work>";
    }
    /// tangent_rhs_kernel: x, the multipliers of level k*, the column sums w and the fixed slots' tangents
    inline size_t tangent_rhs_lds_bytes(uint32_t nVar, uint32_t cap) { return 8 * (3 * (size_t)nVar + cap); }

    // ---- lexls_lse_solve_rhs (lse_adjoint.hip): new right-hand sides on the kept factor, lane = right-hand side ----
    /// plain factors: apply_solve_map_multi_kernel under tangent_map_placement, named after this call
    inline const char *solve_rhs_placement_name(TangentPlacement p)
    {
        return p == TangentPlacement::staged ? "solve_rhs<64,staged>" : p == TangentPlacement::lds ? "solve_rhs<64,lds>" : "solve_rhs<64,work>";
    }
    /// lexls_lse_residual_rhs (residual_rhs_kernel): the same state under the same rule — the residuals are formed in place on it
    inline const char *residual_rhs_placement_name(TangentPlacement p)
    {
        return p == TangentPlacement::staged ? "residual_rhs<64,staged>" : p == TangentPlacement::lds ? "residual_rhs<64,lds>" : "residual_rhs<64,work>";
    }
    /// damped factors (apply_solve_map_reg_multi_kernel): the per-lane state t (cap), z, r, the right-hand side of D (nVar each), [index][lane];
    /// the problem's matrices, shared by the lanes: the null-space basis and D (nVar x nVar each — the forward pass reads the basis as it
    /// stands at a level's entry, so it keeps no snapshots)
    constexpr size_t solve_rhs_reg_matrix_doubles(uint32_t nVar) { return 2 * (size_t)nVar * nVar; }
    constexpr size_t solve_rhs_reg_state_doubles(uint32_t nVar, uint32_t cap, uint32_t ld) { return (size_t)ld * (3 * (size_t)nVar + cap); }
    /// where they live: state (leading dimension 65) and matrices in LDS; the state in LDS, the matrices in a work buffer of the handle (read at
    /// wavefront-uniform addresses); both in the work buffer (state: leading dimension 64, a lane's walk takes consecutive words) where one
    /// workgroup's LDS does not hold the state.  The transpositions and positions (2 x nVar words) are in LDS under every form
    enum class SolveRhsRegForm { lds, hbm, work };
    inline size_t solve_rhs_reg_lds_bytes(uint32_t nVar, uint32_t cap, uint32_t /*nObj*/, SolveRhsRegForm f)
    {
        size_t b = 8 * (size_t)nVar;
        if (f != SolveRhsRegForm::work) b += 8 * solve_rhs_reg_state_doubles(nVar, cap, kAdjointMultiLd);
        if (f == SolveRhsRegForm::lds) b += 8 * solve_rhs_reg_matrix_doubles(nVar);
        return (b + 15) & ~(size_t)15;
    }
    /// the placement rule of lexls_lse_solve_rhs on damped factors, decided from the shape alone (the launcher and tests/solve_rhs_fit_check.cpp
    /// read it here)
    inline SolveRhsRegForm solve_rhs_reg_form(uint32_t nVar, uint32_t cap, uint32_t nObj)
    {
        if (solve_rhs_reg_lds_bytes(nVar, cap, nObj, SolveRhsRegForm::lds) <= kMaxLdsBytes) return SolveRhsRegForm::lds;
        if (solve_rhs_reg_lds_bytes(nVar, cap, nObj, SolveRhsRegForm::hbm) <= kMaxLdsBytes) return SolveRhsRegForm::hbm;
        return SolveRhsRegForm::work;
    }
    /// doubles of the work buffer per (problem, tile of 64 right-hand sides): the matrices first, then (work form) the state
    inline size_t solve_rhs_reg_work_doubles(uint32_t nVar, uint32_t cap, SolveRhsRegForm f)
    {
        return f == SolveRhsRegForm::lds ? 0 : solve_rhs_reg_matrix_doubles(nVar) + (f == SolveRhsRegForm::work ? solve_rhs_reg_state_doubles(nVar, cap, kTangentWorkLd) : 0);
    }
    inline const char *solve_rhs_reg_form_name(SolveRhsRegForm f)
    {
        return f == SolveRhsRegForm::lds ? "solve_rhs_reg<64,lds>" : f == SolveRhsRegForm::hbm ? "solve_rhs_reg<64,hbm>" : "solve_rhs_reg<64,work>";
    }

    // ---- lexls_lsi_batch_solve_bounds (lsi_final.h): lsi_bounds_check_kernel, lane = bound set ----
    /// rows of one chunk of the caller's lb / ub that a wavefront turns from "along the rows" (how they are loaded) to "along the bound sets" (how
    /// the lanes read them), through LDS: two tiles of kBoundsCheckRows x kAdjointMultiLd doubles under either placement
    constexpr uint32_t kBoundsCheckRows = 16;
    /// what one workgroup may ask for: a quarter of a CU's LDS, so that four wavefronts of it share a CU whatever nVar is
    constexpr size_t kBoundsCheckLdsBudget = 40 * 1024;
    /// where the x vectors of a wavefront's 64 bound sets live: transposed in LDS ([variable][lane], odd leading dimension 65), or where
    /// lexls_lse_solve_rhs_device left them (global memory, each lane its own vector)
    enum class BoundsCheckPlacement { lds, hbm };
    inline size_t bounds_check_lds_bytes(uint32_t nVar, BoundsCheckPlacement p)
    {
        return 8 * (size_t)kAdjointMultiLd * (2 * (size_t)kBoundsCheckRows + (p == BoundsCheckPlacement::lds ? (size_t)nVar : 0));
    }
    /// the placement rule of lexls_lsi_batch_solve_bounds, decided from nVar alone (the launcher and tests/lsi_bounds_fit_check.cpp read it here)
    inline BoundsCheckPlacement bounds_check_placement(uint32_t nVar)
    {
        return bounds_check_lds_bytes(nVar, BoundsCheckPlacement::lds) <= kBoundsCheckLdsBudget ? BoundsCheckPlacement::lds : BoundsCheckPlacement::hbm;
    }
    inline const char *bounds_check_placement_name(BoundsCheckPlacement p) { return p == BoundsCheckPlacement::lds ? "lsi_bounds_check<lds>" : "lsi_bounds_check<hbm>"; }
    /// lexls_lsi_batch_solve_bounds_cost: lsi_bounds_check_kernel<placement, true>, the variant with the per-objective costs, under the same rule
    inline const char *bounds_cost_placement_name(BoundsCheckPlacement p) { return p == BoundsCheckPlacement::lds ? "lsi_bounds_cost<lds>" : "lsi_bounds_cost<hbm>"; }

    // ---- lqr_large (lqr_large.hip): lqr_large_plan.h ----
} // namespace lexls
