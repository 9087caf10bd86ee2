// Which kernel serves a LexLSE factorization: the WHOLE decision, as a pure function of plain values.  The caller (lexls_capi.hip) fills a
// DispatchQuery — shape, handle switches, environment and device facts — and gets a KernelPlan: the kernel, its name, and the properties the
// C ABI's bookkeeping follows.  Nothing here reads the environment or calls the HIP runtime; it compiles with any C++17 compiler
// (tests/dispatch_plan_check.cpp walks tests/dispatch_table.json through it on the host).
//
// To register a kernel: add a line to LEXLS_KERNEL_LIST (id, name, launcher kind, launcher), its LDS formula to lexls_lds.h, the condition
// under which it is taken to plan_lqr's helpers below — and re-record nothing: tests/dispatch_table.json shows what changed.
#pragma once
#include "lexls_lds.h"
#include "lqr_large_plan.h"

// X(id, name as lexls_lse_last_kernel reports it, launcher kind, launcher).  The ORDER carries meaning: the planner reaches the variants of a
// shape by offset (x only, + 1 factor kept, + 2 fixed variables; lqr_qtol: + 5 estimating, + 10 ragged; lsi_fused: + 3 regularized).  Kinds (lqr_small.hip): PLAIN (a, s); EST (a, s, est, count) — the
// accuracy guard's estimating form; IND (a, s, ind) — over a list of problems; REG (a, s, reg_cfg) — the regularized wave kernel, which reports the
// placement it launched with; FUSED — the persistent LexLSI launch; NONE — launched by name
// in lexls_capi.hip (the generic kernel's and the large path's launchers take more than a table entry carries)
#define LEXLS_KERNEL_LIST(X)                                                                                  \
    X(none, "", NONE, 0)                                                                                      \
    X(wave_41x12e_x, "lqr_wave<41,12,exact>", PLAIN, launch_wave_41x12e_x)                                    \
    X(wave_41x12e_f, "lqr_wave<41,12,exact>", PLAIN, launch_wave_41x12e_f)                                    \
    X(wave_41x12_x, "lqr_wave<41,12>", PLAIN, launch_wave_41x12_x)                                            \
    X(wave_41x12_f, "lqr_wave<41,12>", PLAIN, launch_wave_41x12_f)                                            \
    X(wave_64x16_x, "lqr_wave<64,16>", PLAIN, launch_wave_64x16_x)                                            \
    X(wave_64x16_f, "lqr_wave<64,16>", PLAIN, launch_wave_64x16_f)                                            \
    X(wave_41x12_fR, "lqr_wave<41,12,regularized>", REG, launch_wave_41x12_fR)                                \
    X(wave_64x16_fR, "lqr_wave<64,16,regularized>", REG, launch_wave_64x16_fR)                                \
    X(lwave_41x12e_x, "lqr_lwave<41,12,exact>", PLAIN, launch_lwave_41x12e_x)                                 \
    X(lwave_41x12e_f, "lqr_lwave<41,12,exact>", PLAIN, launch_lwave_41x12e_f)                                 \
    X(lwave_41x12_x, "lqr_lwave<41,12>", PLAIN, launch_lwave_41x12_x)                                         \
    X(lwave_41x12_f, "lqr_lwave<41,12>", PLAIN, launch_lwave_41x12_f)                                         \
    X(quad_1x12_x, "lqr_quad<1,12>", PLAIN, launch_quad_1x12_x)                                               \
    X(quad_1x12_f, "lqr_quad<1,12,factor>", PLAIN, launch_quad_1x12_f)                                        \
    X(quad_2x12_x, "lqr_quad<2,12>", PLAIN, launch_quad_2x12_x)                                               \
    X(quad_2x12_f, "lqr_quad<2,12,factor>", PLAIN, launch_quad_2x12_f)                                        \
    X(quad_3x12_x, "lqr_quad<3,12>", PLAIN, launch_quad_3x12_x)                                               \
    X(quad_3x12_f, "lqr_quad<3,12,factor>", PLAIN, launch_quad_3x12_f)                                        \
    X(quad_3x12_xF, "lqr_quad<3,12,fixed>", PLAIN, launch_quad_3x12_xF)                                       \
    X(quad_3x12_fF, "lqr_quad<3,12,factor,fixed>", PLAIN, launch_quad_3x12_fF)                                \
    X(quad_3x12s7_x, "lqr_quad<3,12,shift 7>", PLAIN, launch_quad_3x12s7_x)                                   \
    X(quad_3x12s7_f, "lqr_quad<3,12,shift 7,factor>", PLAIN, launch_quad_3x12s7_f)                            \
    X(quad_3x12s7_xF, "lqr_quad<3,12,shift 7,fixed>", PLAIN, launch_quad_3x12s7_xF)                           \
    X(quad_3x12s7_fF, "lqr_quad<3,12,shift 7,factor,fixed>", PLAIN, launch_quad_3x12s7_fF)                    \
    X(quad_4x16_x, "lqr_quad<4,16>", PLAIN, launch_quad_4x16_x)                                               \
    X(quad_4x16_f, "lqr_quad<4,16,factor>", PLAIN, launch_quad_4x16_f)                                        \
    X(quad_4x16_xF, "lqr_quad<4,16,fixed>", PLAIN, launch_quad_4x16_xF)                                       \
    X(quad_4x16_fF, "lqr_quad<4,16,factor,fixed>", PLAIN, launch_quad_4x16_fF)                                \
    X(quad_1x12_xi, "lqr_quad<1,12,indirect>", IND, launch_quad_1x12_xi)                                      \
    X(quad_2x12_xi, "lqr_quad<2,12,indirect>", IND, launch_quad_2x12_xi)                                      \
    X(quad_3x12_xi, "lqr_quad<3,12,indirect>", IND, launch_quad_3x12_xi)                                      \
    X(quad_3x12s7_xi, "lqr_quad<3,12,shift 7,indirect>", IND, launch_quad_3x12s7_xi)                          \
    X(qtol_3x12s7, "lqr_qtol<3,12,shift 7>", PLAIN, launch_qtol_3x12s7)                                       \
    X(qtol_3x12, "lqr_qtol<3,12>", PLAIN, launch_qtol_3x12)                                                   \
    X(qtol_2x12, "lqr_qtol<2,12>", PLAIN, launch_qtol_2x12)                                                   \
    X(qtol_3x8, "lqr_qtol<3,8>", PLAIN, launch_qtol_3x8)                                                      \
    X(qtol_2x8, "lqr_qtol<2,8>", PLAIN, launch_qtol_2x8)                                                      \
    X(qtol_3x12s7e, "lqr_qtol<3,12,shift 7,guard>", EST, launch_qtol_3x12s7e)                                 \
    X(qtol_3x12e, "lqr_qtol<3,12,guard>", EST, launch_qtol_3x12e)                                             \
    X(qtol_2x12e, "lqr_qtol<2,12,guard>", EST, launch_qtol_2x12e)                                             \
    X(qtol_3x8e, "lqr_qtol<3,8,guard>", EST, launch_qtol_3x8e)                                                \
    X(qtol_2x8e, "lqr_qtol<2,8,guard>", EST, launch_qtol_2x8e)                                                \
    X(qtol_3x12s7r, "lqr_qtol<3,12,shift 7,ragged>", PLAIN, launch_qtol_3x12s7r)                              \
    X(qtol_3x12r, "lqr_qtol<3,12,ragged>", PLAIN, launch_qtol_3x12r)                                          \
    X(qtol_2x12r, "lqr_qtol<2,12,ragged>", PLAIN, launch_qtol_2x12r)                                          \
    X(qtol_3x8r, "lqr_qtol<3,8,ragged>", PLAIN, launch_qtol_3x8r)                                             \
    X(qtol_2x8r, "lqr_qtol<2,8,ragged>", PLAIN, launch_qtol_2x8r)                                             \
    X(mfma_16x12n40, "lqr_mfma<16,12,n40>", PLAIN, launch_mfma_16x12n40)                                      \
    X(mfma_32x12n40, "lqr_mfma<32,12,n40>", PLAIN, launch_mfma_32x12n40)                                      \
    X(mfma_32x12, "lqr_mfma<32,12>", PLAIN, launch_mfma_32x12)                                                \
    X(mfma_64x12, "lqr_mfma<64,12>", PLAIN, launch_mfma_64x12)                                                \
    X(lsi_fused_41x12e, "lsi_fused<lqr_wave<41,12,exact>>", FUSED, launch_lsi_fused_41x12e)                   \
    X(lsi_fused_41x12, "lsi_fused<lqr_wave<41,12>>", FUSED, launch_lsi_fused_41x12)                           \
    X(lsi_fused_64x16, "lsi_fused<lqr_wave<64,16>>", FUSED, launch_lsi_fused_64x16)                           \
    X(lsi_fused_41x12e_R, "lsi_fused<lqr_wave<41,12,exact,regularized>>", FUSED, launch_lsi_fused_41x12e_R)   \
    X(lsi_fused_41x12_R, "lsi_fused<lqr_wave<41,12,regularized>>", FUSED, launch_lsi_fused_41x12_R)           \
    X(lsi_fused_64x16_R, "lsi_fused<lqr_wave<64,16,regularized>>", FUSED, launch_lsi_fused_64x16_R)           \
    X(generic_64_lds, "lqr_generic<64,lds>", NONE, 0)                                                         \
    X(generic_256_lds, "lqr_generic<256,lds>", NONE, 0)                                                       \
    X(generic_1024_lds, "lqr_generic<1024,lds>", NONE, 0)                                                     \
    X(generic_1024_hbm, "lqr_generic<1024,hbm>", NONE, 0)                                                     \
    X(large_multi, "lqr_large<multi-launch>", NONE, 0)                                                        \
    X(large_fast, "lqr_large<step-per-pivot,mfma>", NONE, 0)

namespace lexls
{
    enum class KernelId : int
    {
#define LEXLS_X(id, name, kind, fn) id,
        LEXLS_KERNEL_LIST(LEXLS_X)
#undef LEXLS_X
            count
    };

    inline const char *kernel_name(KernelId id)
    {
        static const char *const names[] = {
#define LEXLS_X(id, name, kind, fn) name,
            LEXLS_KERNEL_LIST(LEXLS_X)
#undef LEXLS_X
        };
        return names[(int)id];
    }

    /// lexls_lse_set_kernel_policy / LEXLS_KERNEL_POLICY (include/lexls_hip.h); any other integer behaves as `bit_exact` does on the shape kernels
    enum class KernelPolicy : int
    {
        automatic          = 0,
        generic_only       = 1,
        register_resident  = 2, // never the left-looking kernels
        left_looking       = 3, // lqr_lwave wherever the shape allows it
        four_per_wavefront = 4, // the bit-exact lqr_quad wherever the shape allows it
        bit_exact          = 5, // bit-exact everywhere (the large path's multi-launch form)
        qtol               = 6, // lqr_qtol wherever it serves
        mfma_two           = 7, // lqr_mfma, two problems per wavefront, else lqr_qtol
        mfma_one           = 8, // ... one problem per wavefront
        mfma_four          = 9, // ... four problems per wavefront (the IK shape only)
        qtol_ragged        = 10 // as qtol, and lqr_qtol's ragged instantiations
    };

    struct DispatchQuery
    {
        uint32_t batch = 0, nVar = 0, nObj = 0, cap = 0;
        uint32_t uniform_dim   = 0; // every level of every problem has this many rows (0: not so, or unknown)
        uint32_t max_rows      = 0; // most rows of one problem
        uint32_t max_level_dim = 0; // largest level of the batch
        bool has_fixed         = false;
        uint32_t reg_type      = 0;
        bool has_dims          = true;  // per-problem dimensions exist on the device
        uint32_t align         = 16;    // the input's alignment in bytes: 16, 8 or less
        bool gather_by_reference = false; // this round's rows are read through the row references (g_cdata), `in` is unassembled
        bool write_factor = true, do_solve = true;
        bool opportunistic_solve = false; // only the factor was asked for; kernels that produce x at no extra launch do
        KernelPolicy policy = KernelPolicy::automatic;
        bool guard          = false; // accuracy guard on
        bool qtol_off       = false; // LEXLS_QTOL=0
        uint32_t wave_capacity = 2048; // waves of the register-resident kernel the device holds at once (CUs x 4 SIMDs x 2)
        size_t reg_lds_share   = kMaxLdsBytes / 8; // wave_reg_lds_share()
        bool sweep_serves      = false; // the removal sweep serves the batch (sensitivity_sweep_serves): the persistent LexLSI launch needs it
    };

    struct KernelPlan
    {
        KernelId id      = KernelId::none;
        const char *name = "";
        bool estimating         = false; // lqr_qtol's guard instantiation: the compaction (and the re-solve) follow
        bool register_resident  = false; // lqr_wave: may gather rows by reference, leaves prefix-reuse state when it keeps its factor
        bool solves_x           = false; // x is there when the plan's launches are done
        bool needs_solve_launch = false; // ... through a launch_solve_generic behind the factorization
        bool factor_in_hbm      = false; // the factor is kept (asked for, or the kernel always writes it)
        bool reciprocal_solve   = false; // a solve against this factor may multiply by reciprocal diagonals (the step-per-pivot path's contract)
    };

    namespace dispatch
    {
        inline uint32_t nc(const DispatchQuery &q) { return q.nVar + 1; }
        inline KernelId offset(KernelId id, int k) { return static_cast<KernelId>((int)id + k); }
        static_assert((int)KernelId::quad_3x12_fF == (int)KernelId::quad_3x12_x + 3 && (int)KernelId::quad_4x16_fF == (int)KernelId::quad_4x16_x + 3 &&
                          (int)KernelId::qtol_2x8r == (int)KernelId::qtol_2x8 + 10 && (int)KernelId::wave_64x16_f == (int)KernelId::wave_41x12e_x + 5 &&
                          (int)KernelId::lsi_fused_64x16_R == (int)KernelId::lsi_fused_41x12e + 5,
                      "LEXLS_KERNEL_LIST: the variants of a shape stand in the order the planner's offsets assume");

        /// the shapes the one-wavefront-per-problem family takes (fixed variables are handled in-kernel)
        inline bool wave_family_supports(const DispatchQuery &q)
        {
            if (q.reg_type == 7) return false; // the experimental type's by-products need the level lists: generic kernel (lexls_regularize.h)
            return nc(q) <= 64 && q.max_rows <= 64 && q.max_level_dim <= 16 && q.nObj <= 16;
        }

        /// Which tolerance-contract kernels (pivots / ranks exact, x within 1e-10) an x-only solve may take
        struct Tolerance
        {
            bool qtol          = false; // lqr_qtol where it serves
            bool ragged        = false; // ... and its ragged instantiations for levels of at most 12 rows
            int mfma_lanes     = 0;     // lqr_mfma asked for, in front of lqr_qtol: lanes per problem (32 two / 64 one / 16 four problems per wavefront, 16: the IK shape only)
            bool mfma_fallback = false; // lqr_mfma for the shapes lqr_qtol's four slices per wavefront do not hold
        };
        /// Policies 6 .. 10 name them; automatic dispatch takes lqr_qtol wherever it serves (the faster of the two on MI355X: 41 us against 57 us
        /// per 4096 IK problems), else lqr_mfma, unless the process runs under LEXLS_QTOL=0; every other policy, and a round whose rows are
        /// read by reference, stays on the bit-exact kernels.  Accuracy guard: lqr_qtol alone, as its estimating instantiation, where the
        /// policy had it first in line; every other tolerance-contract kernel (the ragged lqr_qtol included) gives way to the bit-exact one
        inline Tolerance tolerance_of(const DispatchQuery &q)
        {
            Tolerance t;
            if (q.gather_by_reference) return t;
            switch (q.policy)
            {
            case KernelPolicy::automatic: t.qtol = t.mfma_fallback = !q.qtol_off; break;
            case KernelPolicy::qtol: t.qtol = true; break;
            case KernelPolicy::mfma_two: t.qtol = true, t.mfma_lanes = 32; break;
            case KernelPolicy::mfma_one: t.qtol = true, t.mfma_lanes = 64; break;
            case KernelPolicy::mfma_four: t.qtol = true, t.mfma_lanes = 16; break;
            case KernelPolicy::qtol_ragged: t.qtol = t.ragged = true; break;
            default: break;
            }
            if (q.guard) t.qtol = t.qtol && t.mfma_lanes == 0, t.ragged = t.mfma_fallback = false, t.mfma_lanes = 0;
            return t;
        }

        /// which of register-resident / left-looking / four-per-wavefront may serve among the bit-exact kernels
        enum class Looking
        {
            never,    // the register-resident kernel
            by_batch, // decide by batch size
            lwave,    // the left-looking wave kernel wherever the shape allows it
            quad      // the four-per-wavefront kernel wherever the shape allows it (deep hierarchies, policy 4, parity tests)
        };
        inline Looking looking_of(const DispatchQuery &q)
        {
            if (q.gather_by_reference || q.policy == KernelPolicy::register_resident) return Looking::never;
            if (q.policy == KernelPolicy::left_looking) return Looking::lwave;
            return q.policy == KernelPolicy::four_per_wavefront ? Looking::quad : Looking::by_batch;
        }

        /// what lqr_mfma and lqr_qtol share: x-only solves, no fixed variables, no regularization, at most 8 levels, an assembled input
        inline bool tolerance_shape(const DispatchQuery &q) { return !q.write_factor && !q.has_fixed && q.reg_type == 0 && q.nObj <= 8 && !q.gather_by_reference; }

        /// the matrix-core kernel (lqr_mfma_impl.h): every level of every problem has exactly 12 rows, n + 1 <= 48 — two problems per wavefront
        /// (n = 40, the IK shape of BASELINE configs[2]/[3], has its own instantiation) or one
        inline KernelId mfma_choice(const DispatchQuery &q, bool one_per_wave)
        {
            if (!tolerance_shape(q) || q.uniform_dim != 12 || (q.cap & 1u) != 0 || q.align < 16 || q.nVar < 1 || nc(q) > 48) return KernelId::none;
            if (one_per_wave) return 4 * mfma_lds_bytes<64, 12>(q.nVar, q.nObj) <= kMaxLdsBytes ? KernelId::mfma_64x12 : KernelId::none;
            if (2 * mfma_lds_bytes<32, 12>(q.nVar, q.nObj) > kMaxLdsBytes) return KernelId::none;
            return q.nVar == 40 ? KernelId::mfma_32x12n40 : KernelId::mfma_32x12;
        }

        /// lqr_qtol's uniform instantiation for levels of md rows (12 or 8): n = 40 with 12 rows, the IK shape (n a compile-time constant,
        /// columns right-aligned in the slots); else 33 .. 48 columns; else up to 32
        inline KernelId qtol_shape(const DispatchQuery &q, uint32_t md)
        {
            const uint32_t n = q.nVar, k = q.nObj;
            const bool eight = md == 8; // levels of eight rows (round 4)
            if (n == 40 && !eight) return qtol_lds_bytes<3, 12>(n, k) <= kMaxLdsBytes ? KernelId::qtol_3x12s7 : KernelId::none;
            if (n + 1 <= 32)
                return n >= 2 && (eight ? qtol_lds_bytes<2, 8>(n, k) : qtol_lds_bytes<2, 12>(n, k)) <= kMaxLdsBytes ? (eight ? KernelId::qtol_2x8 : KernelId::qtol_2x12) : KernelId::none;
            if (n + 1 <= 48) return (eight ? qtol_lds_bytes<3, 8>(n, k) : qtol_lds_bytes<3, 12>(n, k)) <= kMaxLdsBytes ? (eight ? KernelId::qtol_3x8 : KernelId::qtol_3x12) : KernelId::none;
            return KernelId::none;
        }

        /// lqr_qtol (lqr_qtol_impl.h), four problems per wavefront: every level of every problem has exactly 12 (or exactly 8) rows, n + 1 <= 48;
        /// with the accuracy guard its estimating instantiation
        inline KernelId qtol_choice(const DispatchQuery &q)
        {
            if (!tolerance_shape(q) || (q.uniform_dim != 12 && q.uniform_dim != 8) || (q.cap & 1u) != 0 || q.align < 16) return KernelId::none;
            const KernelId id = qtol_shape(q, q.uniform_dim);
            return id == KernelId::none ? id : offset(id, q.guard ? 5 : 0);
        }

        /// lqr_qtol's RAGGED instantiations (kernel policy 10): levels of at most 12 rows each — per-problem dimensions, any mix, zeros
        /// included; cap may be odd and the input needs the alignment of a double only: so do the ragged loads.  The eight-row pair where no
        /// level has more than 8 rows, else the twelve-row trio.  Uniform batches of 12 or 8 rows are qtol_choice's
        inline KernelId qtol_ragged_choice(const DispatchQuery &q)
        {
            if (!tolerance_shape(q) || q.max_level_dim > 12 || q.cap < 2 || !q.has_dims || q.align < 8) return KernelId::none;
            const KernelId id = qtol_shape(q, q.max_level_dim <= 8 ? 8 : 12);
            return id == KernelId::none ? id : offset(id, 10);
        }

        /// the batch needs more than one round of the register-resident kernel, or a policy asks for the left-looking forms
        inline bool lwave_pays(const DispatchQuery &q, Looking ll) { return ll == Looking::lwave || ll == Looking::quad || (ll == Looking::by_batch && q.batch > q.wave_capacity); }

        /// the four-per-wavefront bit-exact kernel (lqr_quad_impl.h): one wave per SIMD serves 4 x 4 x CUs problems per round; fixed variables in
        /// the FIX instantiations.  none: automatic dispatch / the policy takes another kernel
        inline KernelId quad_choice(const DispatchQuery &q, bool write_factor, Looking ll, bool has_fixed)
        {
            if (q.reg_type != 0 || ll == Looking::never || ll == Looking::lwave) return KernelId::none; // REG / register-resident / left-looking wave kernel asked for
            // Measured on MI355X (scripts/crossover.py, n = 40, 5 x 12, us per batch, register-resident / four-per-wavefront): x only — 512: 58 / 53,
            // 1024: 62 / 54, 2048: 78 / 58, 4096: 146 / 63: the four-per-wavefront kernel at every batch size; factor kept — 1024: 71 / 98,
            // 2048: 89 / 103, 3072: 144 / 109, 4096: 166 / 115: the register-resident kernel while the batch fits one round of it.
            // Factor kept, automatic dispatch (scripts/dispatch_scan.py, register-resident / four-per-wavefront, us per batch): one slot (n = 12,
            // 3 x 4) 33 / 28 at 256, 42 / 29 at 2048: four-per-wavefront at every batch size; two slots (n = 20, 30) within 10 % up to 1024,
            // 62 / 56 and 66 / 56 at 2048: from 2048 on; 42..48 columns, where the register-resident alternative is the 64-column
            // instantiation (n = 47, 4 x 12): 120 / 96 at 256, 299 / 109 at 2048: at every batch size
            const uint32_t c  = nc(q);
            const bool pays   = lwave_pays(q, ll);
            const bool full   = q.batch >= q.wave_capacity; // the register-resident kernel is at two wavefronts per SIMD
            const bool forced = ll == Looking::quad;
            const int variant = (write_factor ? 1 : 0) + (has_fixed ? 2 : 0);
            size_t lds = (q.max_level_dim <= 12) ? quad_lds_bytes(3, 12, q.nVar, q.nObj) : 0;
            if (lds && lds <= kMaxLdsBytes)
            {
                if (!(forced || !write_factor || pays || (!has_fixed && c <= 16) || (!has_fixed && c <= 32 && full) || c > 41)) return KernelId::none;
                if (!has_fixed && c <= 16) return offset(KernelId::quad_1x12_x, variant); // one slot
                if (!has_fixed && c <= 32) return offset(KernelId::quad_2x12_x, variant); // two slots
                return offset(q.nVar == 40 ? KernelId::quad_3x12s7_x : KernelId::quad_3x12_x, variant); // s7: the IK shape, columns right-aligned in the slots (see SIG in lqr_quad_impl.h)
            }
            // n + 1 <= 64, level dims <= 16: x only at every batch size; with the factor kept when forced (deep hierarchies, kernel policy 4) or when
            // the batch needs more than one round of the register-resident kernel (n = 55, [16,14,16,12], factor kept, us per batch, register-
            // resident / four-per-wavefront: 1024: 168 / 183, 2048: 332 / 206, 4096: 640 / 404, 8192: 1155 / 799: from 2048 on)
            lds = (q.max_level_dim <= 16 && (!write_factor || forced || pays || full)) ? quad_lds_bytes(4, 16, q.nVar, q.nObj) : 0;
            return (lds && lds <= kMaxLdsBytes) ? offset(KernelId::quad_4x16_x, variant) : KernelId::none;
        }

        /// the register-resident kernel's instantiation for a shape: 0 the 41-column one with n + 1 = 41 exactly (EXACT), 1 up to 41 columns,
        /// 2 the 64-column / 16-row one.  The LSE kernel and the persistent LexLSI launch both go by it
        inline int wave_shape(const DispatchQuery &q) { return q.max_level_dim <= 12 && nc(q) <= 41 ? (nc(q) == 41 ? 0 : 1) : 2; }

        /// the bit-exact member of the one-wavefront-per-problem family (in order of preference: the regularization family, four-per-wavefront,
        /// left-looking, register-resident)
        inline KernelId exact_choice(const DispatchQuery &q, bool write_factor, Looking ll, bool has_fixed)
        {
            const int shape = wave_shape(q);
            if (q.reg_type != 0) return shape <= 1 ? KernelId::wave_41x12_fR : KernelId::wave_64x16_fR; // the REG instantiations (factor always kept)
            const KernelId quad = quad_choice(q, write_factor, ll, has_fixed);
            if (quad != KernelId::none) return quad;
            // left-looking form (lqr_lwave_impl.h): one level block live per wave, 4 waves/SIMD; no fixed variables.  Measured on MI355X
            // (scripts/latency_scan.py, n = 40, 5 x 12): while the batch fits one round of the register-resident kernel (<= 2048 problems)
            // that kernel has the shorter latency (factor kept: 66-72 us vs 97-101 us; x only: equal); beyond that the left-looking kernel
            // still runs in one round (4096: 115 us vs 158 us)
            if (lwave_pays(q, ll) && !has_fixed && shape <= 1 && q.nObj <= 8) return offset(KernelId::lwave_41x12e_x, 2 * shape + (write_factor ? 1 : 0));
            return offset(KernelId::wave_41x12e_x, 2 * shape + (write_factor ? 1 : 0));
        }

        inline bool is_register_resident(KernelId id) { return id >= KernelId::wave_41x12e_x && id <= KernelId::wave_64x16_fR; }

        /// the one-wavefront-per-problem family with its tolerance-contract members in front
        inline KernelId wave_family_choice(const DispatchQuery &q, Looking ll)
        {
            const Tolerance t = tolerance_of(q);
            KernelId id       = KernelId::none;
            if (t.mfma_lanes == 16 && mfma_choice(q, false) == KernelId::mfma_32x12n40) return KernelId::mfma_16x12n40;
            if (t.mfma_lanes >= 32 && (id = mfma_choice(q, t.mfma_lanes == 64)) != KernelId::none) return id;
            if (t.qtol && (id = qtol_choice(q)) != KernelId::none) return id;
            if (t.ragged && (id = qtol_ragged_choice(q)) != KernelId::none) return id;
            if (t.mfma_fallback && (id = mfma_choice(q, false)) != KernelId::none) return id;
            return exact_choice(q, q.write_factor, ll, q.has_fixed);
        }

        /// lqr_generic's form: the problem staged in LDS by 64 / 256 / 1024 threads, else left in HBM (none: nVar too large for the norm table)
        inline KernelId generic_choice(const DispatchQuery &q)
        {
            const uint32_t ldp = odd_ld(q.max_rows), w = nc(q) > q.max_rows ? nc(q) : q.max_rows;
            auto fits          = [&](int nt, bool ldsmat) { return generic_lds_bytes(ldp, q.nVar, q.nObj, nt, ldsmat) <= kMaxLdsBytes; };
            if (w <= 64 && fits(64, true)) return KernelId::generic_64_lds;
            if (w <= 512 && fits(256, true)) return KernelId::generic_256_lds;
            if (fits(1024, true)) return KernelId::generic_1024_lds;
            return fits(1024, false) ? KernelId::generic_1024_hbm : KernelId::none;
        }

        /// problems too large for one CU's LDS: one launch per stage, the whole chip per problem (lqr_large.hip)
        inline bool large_supports(const DispatchQuery &q)
        {
            const LargeLds l = large_lds_bytes(q.nVar, q.max_level_dim);
            return !q.has_fixed && l.trsm <= kMaxLdsBytes && l.piv <= kMaxLdsBytes && l.app <= kMaxLdsBytes && q.max_level_dim < 65536 && q.nObj < 65536;
        }
    } // namespace dispatch

    /// The kernel that serves one factorization (lexls_lse_factorize / lexls_lse_factorize_solve) and what follows from the choice
    inline KernelPlan plan_lqr(const DispatchQuery &q)
    {
        using namespace dispatch;
        KernelPlan p;
        const bool shape_kernels = q.policy != KernelPolicy::generic_only;
        // (the regularization family lives in the register-resident wave kernel's REG instantiations and in the generic kernel)
        if (shape_kernels && wave_family_supports(q))
        {
            p.id       = wave_family_choice(q, looking_of(q));
            p.solves_x = true; // always solves as well
        }
        // Deep hierarchies — more than 64 rows in all, which the register-resident kernel's LDS image of the rows below a level cannot hold —
        // go to the left-looking kernels (a level's rows come from HBM when the level starts; LDS holds only the finished pivot rows) where
        // lqr_quad or lqr_lwave takes the shape; the tolerance-contract kernels under their own rules: they read a level's rows that way, too
        else if (shape_kernels && q.policy != KernelPolicy::register_resident && q.max_rows > 64 && q.max_level_dim <= 16 && q.nObj <= 16 && q.reg_type == 0 && nc(q) <= 64 &&
                 !is_register_resident(exact_choice(q, q.write_factor, Looking::quad, q.has_fixed)))
        {
            p.id       = wave_family_choice(q, Looking::quad);
            p.solves_x = true;
        }
        else if (shape_kernels && q.reg_type == 0 && generic_lds_bytes(odd_ld(q.max_rows), q.nVar, q.nObj, 1024, true) > kMaxLdsBytes && large_supports(q))
        {
            // the bit-exact multi-launch path (ordered chains: parity tests, reference for the fast path) under policy 5 and the accuracy guard;
            // else one launch per pivot step, whose contract allows reciprocals in the solve behind it
            const bool exact     = q.policy == KernelPolicy::bit_exact || q.guard;
            p.id                 = exact ? KernelId::large_multi : KernelId::large_fast;
            p.reciprocal_solve   = !exact;
            p.needs_solve_launch = p.solves_x = q.do_solve;
            p.factor_in_hbm      = true;
        }
        else
        {
            p.id            = generic_choice(q);
            p.solves_x      = q.do_solve || q.opportunistic_solve;
            p.factor_in_hbm = p.id == KernelId::generic_1024_hbm;
        }
        p.name              = kernel_name(p.id);
        p.estimating        = p.id >= KernelId::qtol_3x12s7e && p.id <= KernelId::qtol_2x8e;
        p.register_resident = is_register_resident(p.id);
        p.factor_in_hbm     = p.factor_in_hbm || q.write_factor;
        return p;
    }

    /// the accuracy guard's re-solve (mode 2): the bit-exact x-only four-per-wavefront instantiation policy 4 takes for these arguments, in its
    /// indirect form over [count, list]; none where policy 4 would take no such kernel (the 4 x 16 shape has no indirect form)
    inline KernelId plan_guard_resolve(const DispatchQuery &q)
    {
        switch (dispatch::quad_choice(q, false, dispatch::Looking::quad, false))
        {
        case KernelId::quad_1x12_x: return KernelId::quad_1x12_xi;
        case KernelId::quad_2x12_x: return KernelId::quad_2x12_xi;
        case KernelId::quad_3x12_x: return KernelId::quad_3x12_xi;
        case KernelId::quad_3x12s7_x: return KernelId::quad_3x12s7_xi;
        default: return KernelId::none;
        }
    }

    /// Does a resident LexLSI round (capacities as dimensions, factor kept) read its rows by reference inside the register-resident wave
    /// kernel — one launch and one pass over the problems less — or assemble them with a gather launch for another kernel?
    /// A forced left-looking / four-per-wavefront policy is honoured; otherwise the register-resident kernel at every batch size: on the
    /// ragged problems of a lock-step LSI stage, with the gather fused, it beats the four-per-wavefront kernel + gather launch also beyond
    /// one round — 4096 instances, warm-started ~30 iterations: 37.1 ms vs 39.1 ms.
    /// 42..48 columns are the exception: their register-resident form is the 64-column instantiation, and the four-per-wavefront kernel
    /// behind a gather launch is ahead of it at every batch size (1024 instances, n = 47, 5 x 12, cold: 21.3 -> 17.1 ms).
    /// (a regularized round: the REG instantiation of that kernel, the same load; type 7 has none)
    inline bool plan_round_gathers_by_reference(const DispatchQuery &q)
    {
        using namespace dispatch;
        const bool wide_slot = nc(q) > 41 && nc(q) <= 48 && q.max_level_dim <= 12;
        Looking ll           = looking_of(q);
        if (ll == Looking::by_batch && !(wide_slot && q.policy == KernelPolicy::automatic)) ll = Looking::never;
        return q.policy != KernelPolicy::generic_only && wave_family_supports(q) && is_register_resident(exact_choice(q, true, ll, q.has_fixed));
    }

    /// The persistent LexLSI launch (lsi_fused_impl.h) for a resident batch: the instantiation of the register-resident kernel the stage path
    /// would take, where that path gathers by reference under automatic dispatch and the removal sweep serves the batch; none: the driver
    /// enqueues the stage's three kernels (the launcher may still decline: its LDS depends on the driver's own arrays)
    inline KernelId plan_lsi_fused(const DispatchQuery &q)
    {
        if (q.policy != KernelPolicy::automatic || !plan_round_gathers_by_reference(q) || !q.sweep_serves) return KernelId::none;
        return dispatch::offset(KernelId::lsi_fused_41x12e, dispatch::wave_shape(q) + (q.reg_type != 0 ? 3 : 0));
    }

    /// the instantiation behind a plan of plan_lsi_fused: <64, 16> (true) or <41, 12> — the launch table's own columns (X-list above), for whoever sums the LDS
    inline bool lsi_fused_is_64x16(KernelId id) { return id == KernelId::lsi_fused_64x16 || id == KernelId::lsi_fused_64x16_R; }

    /// true when the REG instantiation a regularized batch of these capacities takes gets its LDS (the launcher's own test)
    inline bool wave_reg_kernel_fits(const DispatchQuery &q)
    {
        uint32_t reg_cfg = 0;
        if (dispatch::wave_shape(q) <= 1)
            return wave_reg_lds_bytes<12>(q.nVar, q.reg_type, q.reg_lds_share, wave_lds_bytes<41, 12>(q.nObj, wave_img_doubles<12>(q.nVar, q.nObj)), reg_cfg) <= kMaxLdsBytes;
        return wave_reg_lds_bytes<16>(q.nVar, q.reg_type, q.reg_lds_share, wave_lds_bytes<64, 16>(q.nObj, wave_img_doubles<16>(q.nVar, q.nObj)), reg_cfg) <= kMaxLdsBytes;
    }
} // namespace lexls
