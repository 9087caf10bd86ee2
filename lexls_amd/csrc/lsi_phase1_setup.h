// Phase 1 of a lock-step LexLSI batch without host objects: the serial, order-defining part of what runner::setup + LexLSI::begin() +
// BatchCtx::hand_over leave behind — the input checks and equality activations of LexLSI::setData (lexlsi.h:160-206), api_activate over the
// guess (lsi_runner.h:75-81), the working-set lists in the order workingset.h gives them, the activation stamps, and the equality problem an
// instance's working set stands for (Objective::formLexLSE, objective.h:434-494).  Plain functions that compile for the host as well (no HIP
// header is needed): the device runs them inside lsi_phase1_setup_kernel / lsi_iterate_finish, tests/lsi_phase1_setup_check.cpp runs the very
// same code against a host LexLSI.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <lexls/typedefs.h>

#if defined(__HIPCC__)
#define LEXLS_P1_FN __host__ __device__ __forceinline__
#else
#define LEXLS_P1_FN inline
#endif

namespace
{
    using namespace LexLS;

    constexpr uint32_t STEP_MAX_OBJ = 16;
    struct StepShape
    {
        uint32_t n, nObj, total, SD; // SD = n + 2 total: per instance [x | v | A x]
        uint32_t dim[STEP_MAX_OBJ], simple[STEP_MAX_OBJ], first[STEP_MAX_OBJ];
        uint64_t off[STEP_MAX_OBJ]; // first element of the objective's [A | lb | ub] (or [lb | ub]) block inside a problem's data
        uint64_t per_data;
        uint32_t dim0;
        double tol_feasibility;
    };

    /// what is wrong with an instance's input (the smallest code an instance has is the one reported)
    enum : uint32_t { P1_OK = 0, P1_LB_ABOVE_UB = 1, P1_VAR_RANGE = 2, P1_VAR_DUPLICATE = 3, P1_GUESS_TYPE = 4, P1_OBJ_DIM = 5 };
    inline const char *p1_fault_text(uint32_t fault)
    {
        switch (fault)
        {
        case P1_LB_ABOVE_UB: return "Lower bound is greater than upper bound.";
        case P1_VAR_RANGE: return "An element of VarIndex is not below the number of variables.";
        case P1_VAR_DUPLICATE: return "Elements of VarIndex are not unique.";
        case P1_GUESS_TYPE: return "An entry of the active-set guess is not an activation type (0 .. 3).";
        case P1_OBJ_DIM: return "An objective row count is above the batch's capacity.";
        default: return "";
        }
    }
    /// Per-instance objective row counts (lexls_lsi_batch_set_instance_obj_dims).  RAGGED and `cnt`, wherever they appear below: the instance's nObj
    /// counts; without RAGGED cnt is not looked at and every objective has its capacity sh.dim[k] rows — the code a batch without counts has always
    /// run.  Objective k of the instance is the first cnt[k] rows of its block; sh.dim[k] stays the leading dimension of the block and sh.first[k]
    /// its first row among the instance's `total`.  Rows from cnt[k] on are absent: nothing of them is read.  (The resident iteration has
    /// resident_rows, lexls_lsi_device.h)
    template <bool RAGGED = false>
    LEXLS_P1_FN uint32_t p1_rows(const StepShape &sh, const uint32_t *cnt, uint32_t k)
    {
        if constexpr (RAGGED)
            return cnt[k];
        else
            return sh.dim[k];
    }

    /// p1_row_class: the row's bounds are in the wrong order
    constexpr uint8_t P1_ROW_FAULT = 0x80;

    /// LexLSI::setData on row c of objective k (lexlsi.h:166-180 general, :192-200 simple bounds): CTR_ACTIVE_EQ when the row enters the working set
    /// as an equality (|lb - ub| < 1e-15 and, for a general row, a non-zero normal by the ordered fma chain of :172-174), P1_ROW_FAULT for lb > ub,
    /// 0 otherwise.  Independent per row: on the device lane = row
    LEXLS_P1_FN uint8_t p1_row_class(const StepShape &sh, const double *data, uint32_t k, uint32_t c)
    {
        const uint32_t dim = sh.dim[k], n = sh.n;
        const double *blk  = data + sh.off[k];
        const double bl = sh.simple[k] ? blk[c] : blk[c + (size_t)n * dim], bu = sh.simple[k] ? blk[c + dim] : blk[c + (size_t)(n + 1) * dim];
        if (std::fabs(bl - bu) < 1e-15) // internal::isEqual
        {
            if (sh.simple[k]) return (uint8_t)CTR_ACTIVE_EQ;
            double s = 0.0;
            for (uint32_t j = 0; j < n; j++)
            {
                const double a = blk[c + (size_t)j * dim];
                s              = __builtin_fma(a, a, s);
            }
            return s > 0 ? (uint8_t)CTR_ACTIVE_EQ : (uint8_t)0;
        }
        return bl > bu ? P1_ROW_FAULT : (uint8_t)0;
    }

    /// entry c of the variable indices of a simple-bounds objective 0 (lexlsi.h:201-203, and the range the host takes for granted)
    template <bool RAGGED = false>
    LEXLS_P1_FN uint32_t p1_var_fault(const StepShape &sh, const uint32_t *var, uint32_t c, const uint32_t *cnt = nullptr)
    {
        if (var[c] >= sh.n) return P1_VAR_RANGE;
        uint32_t d0 = sh.dim0;
        if constexpr (RAGGED) d0 = cnt[0];
        for (uint32_t j = 0; j < d0; j++)
            if (j != c && var[j] == var[c]) return P1_VAR_DUPLICATE;
        return P1_OK;
    }

    /// a flag of the active-set guess (the host path warns and passes over it, lexlsi.h:120-136; here it is an input fault)
    LEXLS_P1_FN uint32_t p1_guess_fault(uint8_t flag) { return flag > 3 ? (uint32_t)P1_GUESS_TYPE : (uint32_t)P1_OK; }

    /// every check of one instance by ONE thread (the setup kernel spreads the same calls over its lanes): the smallest code found, P1_OK = none.
    /// cls (total entries) receives p1_row_class of every constraint; var / guess may be NULL where the instance has none
    LEXLS_P1_FN uint32_t p1_instance_fault(const StepShape &sh, const double *data, const uint32_t *var, const uint8_t *guess, uint8_t *cls)
    {
        uint32_t fault = 0xffffffffu;
        for (uint32_t k = 0; k < sh.nObj; k++)
            for (uint32_t c = 0; c < sh.dim[k]; c++)
            {
                const uint32_t g = sh.first[k] + c;
                cls[g]           = p1_row_class(sh, data, k, c);
                if (cls[g] == P1_ROW_FAULT && (uint32_t)P1_LB_ABOVE_UB < fault) fault = P1_LB_ABOVE_UB;
                if (guess && p1_guess_fault(guess[g]) != P1_OK && (uint32_t)P1_GUESS_TYPE < fault) fault = P1_GUESS_TYPE;
            }
        for (uint32_t c = 0; c < sh.dim0; c++)
        {
            const uint32_t f = p1_var_fault(sh, var, c);
            if (f != P1_OK && f < fault) fault = f;
        }
        return fault == 0xffffffffu ? (uint32_t)P1_OK : fault;
    }

    /// WorkingSet::activate (workingset.h:60-69) on the lists of objective k (f = its first constraint, nak = its active constraints so far): swap
    /// with last in the inactive list, append to the active one.  The same statements as the ADD of lsi_iterate_finish
    template <bool RAGGED = false>
    LEXLS_P1_FN void p1_activate(const StepShape &sh, uint32_t k, uint32_t c, uint8_t type, uint8_t *cs, uint16_t *act, uint16_t *ina, uint16_t *ipos, uint16_t *na,
                                 const uint32_t *cnt = nullptr)
    {
        const uint32_t f = sh.first[k], nak = na[k], nik = p1_rows<RAGGED>(sh, cnt, k) - nak;
        const uint32_t pos = ipos[f + c], last = ina[f + nik - 1];
        ina[f + pos]   = (uint16_t)last;
        ipos[f + last] = (uint16_t)pos;
        cs[f + c]      = type;
        act[f + nak]   = (uint16_t)c;
        na[k]          = (uint16_t)(nak + 1);
    }

    /// The working set an instance starts from, ONE thread's work (at most 2 total steps).  cls: p1_row_class of every constraint; guess: total
    /// activation flags or NULL.  The reference's list WS (lexlsi.h:148-173) receives the equality activations of setData first, objective by
    /// objective and row by row, then the guess's LB / UB activations in (objective, row) order — rows that are active already and guess flags
    /// of type EQ are passed over (api_activate, lexlsi.h:120-136); a constraint's position in WS is its stamp.  cs / act / ina / ipos: total
    /// entries each, objective k from first[k] on; na: STEP_MAX_OBJ entries; stamp: total entries (written for the active constraints only).
    /// With cnt the lists are those of the object that has the present rows only; an absent row is inactive and in no list (its entries are 0)
    template <bool RAGGED = false>
    LEXLS_P1_FN void p1_build_working_set(const StepShape &sh, const uint8_t *cls, const uint8_t *guess, uint8_t *cs, uint16_t *act, uint16_t *ina, uint16_t *ipos,
                                          uint16_t *na, uint32_t *stamp, uint32_t *next_stamp, const uint32_t *cnt = nullptr)
    {
        for (uint32_t k = 0; k < STEP_MAX_OBJ; k++) na[k] = 0;
        for (uint32_t k = 0; k < sh.nObj; k++) // WorkingSet::reset (workingset.h:51-58)
        {
            const uint32_t rk = p1_rows<RAGGED>(sh, cnt, k);
            for (uint32_t c = 0; c < rk; c++)
            {
                const uint32_t g = sh.first[k] + c;
                cs[g] = (uint8_t)CTR_INACTIVE, act[g] = 0, ina[g] = (uint16_t)c, ipos[g] = (uint16_t)c;
            }
            if constexpr (RAGGED)
                for (uint32_t c = rk; c < sh.dim[k]; c++) // absent rows
                {
                    const uint32_t g = sh.first[k] + c;
                    cs[g] = (uint8_t)CTR_INACTIVE, act[g] = 0, ina[g] = 0, ipos[g] = 0;
                }
        }
        uint32_t next = 0;
        for (uint32_t k = 0; k < sh.nObj; k++)
            for (uint32_t c = 0, rk = p1_rows<RAGGED>(sh, cnt, k); c < rk; c++)
                if (cls[sh.first[k] + c] == (uint8_t)CTR_ACTIVE_EQ)
                {
                    p1_activate<RAGGED>(sh, k, c, (uint8_t)CTR_ACTIVE_EQ, cs, act, ina, ipos, na, cnt);
                    stamp[sh.first[k] + c] = next++;
                }
        if (guess)
            for (uint32_t k = 0; k < sh.nObj; k++)
                for (uint32_t c = 0, rk = p1_rows<RAGGED>(sh, cnt, k); c < rk; c++)
                {
                    const uint8_t t = guess[sh.first[k] + c];
                    if ((t == (uint8_t)CTR_ACTIVE_LB || t == (uint8_t)CTR_ACTIVE_UB) && cs[sh.first[k] + c] == (uint8_t)CTR_INACTIVE)
                    {
                        p1_activate<RAGGED>(sh, k, c, t, cs, act, ina, ipos, na, cnt);
                        stamp[sh.first[k] + c] = next++;
                    }
                }
        *next_stamp = next;
    }

    // ---------------------------------------------------------------------------------------------------------------------------------------
    // The hot-start options of phase 1 (typedefs.h:213-216; h_params slots 12 .. 15): what Objective::phase1 (objective.h:226-236) does with them,
    // objective by objective, on the lists above.  HOT, wherever it appears as a template parameter: some option differs from its default; a run
    // with the defaults compiles none of this in.
    // ---------------------------------------------------------------------------------------------------------------------------------------
    enum : uint32_t { P1_HOT_MODIFY_X = 1u, P1_HOT_TYPE_ACTIVE = 2u, P1_HOT_TYPE_INACTIVE = 4u, P1_HOT_V_MIDPOINT = 8u /* set_min_init_ctr_violation = false */ };
    /// the word a run's options make (0: the defaults)
    inline uint32_t p1_hot_word(const ParametersLexLSI &par)
    {
        return (par.modify_x_guess_enabled ? (uint32_t)P1_HOT_MODIFY_X : 0u) | (par.modify_type_active_enabled ? (uint32_t)P1_HOT_TYPE_ACTIVE : 0u) |
               (par.modify_type_inactive_enabled ? (uint32_t)P1_HOT_TYPE_INACTIVE : 0u) | (par.set_min_init_ctr_violation ? 0u : (uint32_t)P1_HOT_V_MIDPOINT);
    }

    /// the branches of formInitialWorkingSet, of the simple-bounds x rewrite and of initialize_v0, for callers that count them (NULL: nobody does)
    enum : uint32_t
    {
        P1B_INA_LB = 0, P1B_INA_UB, P1B_LB_KEPT, P1B_LB_INA, P1B_LB_UB, P1B_UB_KEPT, P1B_UB_INA, P1B_UB_LB, P1B_EQ, // formInitialWorkingSet
        P1B_X_MID, P1B_X_LB, P1B_X_UB,                                                                             // ensureZeroCtrViolationForSimpleBounds
        P1B_V_ZERO, P1B_V_MID,                                                                                     // initialize_v0, set_min_init_ctr_violation = false
        P1B_COUNT
    };

    /// WorkingSet::deactivate (workingset.h:71-79) on the lists of objective k: ordered erase of entry p of the active list, append to the inactive one.
    /// The same statements as the REMOVE of lsi_iterate_finish
    template <bool RAGGED = false>
    LEXLS_P1_FN void p1_deactivate(const StepShape &sh, uint32_t k, uint32_t p, uint8_t *cs, uint16_t *act, uint16_t *ina, uint16_t *ipos, uint16_t *na, const uint32_t *cnt = nullptr)
    {
        const uint32_t f = sh.first[k], nak = na[k], nik = p1_rows<RAGGED>(sh, cnt, k) - nak;
        const uint32_t c = act[f + p];
        for (uint32_t i = p; i + 1 < nak; i++) act[f + i] = act[f + i + 1];
        cs[f + c]    = (uint8_t)CTR_INACTIVE;
        ina[f + nik] = (uint16_t)c;
        ipos[f + c]  = (uint16_t)nik;
        na[k]        = (uint16_t)(nak - 1);
    }

    /// lb (which = 0) or ub (1) of row c of objective k
    LEXLS_P1_FN double p1_bound(const StepShape &sh, const double *data, uint32_t k, uint32_t c, uint32_t which)
    {
        const uint32_t dim = sh.dim[k];
        return data[sh.off[k] + c + (size_t)(sh.simple[k] ? which : sh.n + which) * dim];
    }

    /// entry c of A x of objective k (Objective::apply_A, objective.h:435-455): x(var(c)) for simple bounds, the ordered fma chain of the row otherwise
    LEXLS_P1_FN double p1_ax(const StepShape &sh, const double *data, const uint32_t *var, const double *x, uint32_t k, uint32_t c)
    {
        if (sh.simple[k]) return x[var[c]];
        const uint32_t dim = sh.dim[k];
        const double *blk  = data + sh.off[k];
        double s           = 0.0;
        for (uint32_t j = 0; j < sh.n; j++) s = __builtin_fma(blk[c + (size_t)j * dim], x[j], s);
        return s;
    }

    /// Objective::formInitialWorkingSet (objective.h:123-159) on objective k for the x guess in x (n doubles, rewritten for a simple-bounds objective
    /// with P1_HOT_MODIFY_X: ensureZeroCtrViolationForSimpleBounds, objective.h:98-120 — the objectives behind see the new x).  ONE thread's work: every
    /// re-typing is an erase from the active list plus an append, and the list order is the row order of the equality problem.  hotmark (total
    /// bytes, zero on entry of objective 0): set for every constraint activated or re-activated here (p1_rebuild_stamps).  branch: P1B_COUNT counters or NULL
    template <bool RAGGED = false>
    LEXLS_P1_FN void p1_form_initial_working_set(const StepShape &sh, const double *data, const uint32_t *var, double *x, uint32_t hot, uint32_t k, uint8_t *cs, uint16_t *act,
                                                 uint16_t *ina, uint16_t *ipos, uint16_t *na, uint8_t *hotmark, const uint32_t *cnt = nullptr, uint32_t *branch = nullptr)
    {
        const uint32_t f = sh.first[k], rk = p1_rows<RAGGED>(sh, cnt, k);
        if (hot & (P1_HOT_TYPE_ACTIVE | P1_HOT_TYPE_INACTIVE))
            for (uint32_t c = 0; c < rk; c++)
            {
                const uint8_t t = cs[f + c];
                if (t == (uint8_t)CTR_ACTIVE_EQ)
                {
                    if (branch) branch[P1B_EQ]++;
                    continue;
                }
                if (t == (uint8_t)CTR_INACTIVE ? !(hot & P1_HOT_TYPE_INACTIVE) : !(hot & P1_HOT_TYPE_ACTIVE)) continue;
                const double ax = p1_ax(sh, data, var, x, k, c), lb = p1_bound(sh, data, k, c, 0), ub = p1_bound(sh, data, k, c, 1);
                uint8_t to = t; // the type the constraint ends with
                if (t == (uint8_t)CTR_INACTIVE)
                    to = ax <= lb ? (uint8_t)CTR_ACTIVE_LB : (ax >= ub ? (uint8_t)CTR_ACTIVE_UB : (uint8_t)CTR_INACTIVE);
                else if (t == (uint8_t)CTR_ACTIVE_LB)
                    to = ax > lb ? (ax >= ub ? (uint8_t)CTR_ACTIVE_UB : (uint8_t)CTR_INACTIVE) : t;
                else
                    to = ax < ub ? (ax <= lb ? (uint8_t)CTR_ACTIVE_LB : (uint8_t)CTR_INACTIVE) : t;
                if (branch)
                {
                    if (t == (uint8_t)CTR_INACTIVE && to != t) branch[to == (uint8_t)CTR_ACTIVE_LB ? P1B_INA_LB : P1B_INA_UB]++;
                    if (t == (uint8_t)CTR_ACTIVE_LB) branch[to == t ? P1B_LB_KEPT : (to == (uint8_t)CTR_INACTIVE ? P1B_LB_INA : P1B_LB_UB)]++;
                    if (t == (uint8_t)CTR_ACTIVE_UB) branch[to == t ? P1B_UB_KEPT : (to == (uint8_t)CTR_INACTIVE ? P1B_UB_INA : P1B_UB_LB)]++;
                }
                if (to == t) continue;
                if (t != (uint8_t)CTR_INACTIVE)
                {
                    uint32_t p = 0; // WorkingSet::getCtrIndex (workingset.h:90-94)
                    while (act[f + p] != c) p++;
                    p1_deactivate<RAGGED>(sh, k, p, cs, act, ina, ipos, na, cnt);
                }
                if (to != (uint8_t)CTR_INACTIVE)
                {
                    p1_activate<RAGGED>(sh, k, c, to, cs, act, ina, ipos, na, cnt);
                    hotmark[f + c] = 1;
                }
            }
        if (sh.simple[k] && (hot & P1_HOT_MODIFY_X))
            for (uint32_t c = 0; c < rk; c++)
            {
                const uint8_t t = cs[f + c];
                const double lb = p1_bound(sh, data, k, c, 0), ub = p1_bound(sh, data, k, c, 1);
                x[var[c]]       = t == (uint8_t)CTR_INACTIVE ? 0.5 * (lb + ub) : (t == (uint8_t)CTR_ACTIVE_LB ? lb : ub);
                if (branch) branch[t == (uint8_t)CTR_INACTIVE ? P1B_X_MID : (t == (uint8_t)CTR_ACTIVE_LB ? P1B_X_LB : P1B_X_UB)]++;
            }
    }

    /// The activation order behind formInitialWorkingSet (LexLSI_T::phase1_objectives, lexlsi.h): first the constraints that are still active with the
    /// type they had (hotmark clear), in the order of their stamps; then the marked ones, objective by objective in active-list order.  In place: the
    /// stamps of the first kind are tagged with the top bit and replaced, smallest first, by 0, 1, ...  ONE thread's work, at most total^2 steps
    LEXLS_P1_FN void p1_rebuild_stamps(const StepShape &sh, const uint16_t *act, const uint16_t *na, const uint8_t *hotmark, uint32_t *stamp, uint32_t *next_stamp)
    {
        uint32_t kept = 0;
        for (uint32_t k = 0; k < sh.nObj; k++)
            for (uint32_t a = 0; a < na[k]; a++)
            {
                const uint32_t g = sh.first[k] + act[sh.first[k] + a];
                if (!hotmark[g]) stamp[g] |= 0x80000000u, kept++;
            }
        for (uint32_t r = 0; r < kept; r++)
        {
            uint32_t best = 0xffffffffu, at = 0;
            for (uint32_t k = 0; k < sh.nObj; k++)
                for (uint32_t a = 0; a < na[k]; a++)
                {
                    const uint32_t g = sh.first[k] + act[sh.first[k] + a];
                    if (!hotmark[g] && (stamp[g] & 0x80000000u) && stamp[g] < best) best = stamp[g], at = g;
                }
            stamp[at] = r;
        }
        uint32_t next = kept;
        for (uint32_t k = 0; k < sh.nObj; k++)
            for (uint32_t a = 0; a < na[k]; a++)
            {
                const uint32_t g = sh.first[k] + act[sh.first[k] + a];
                if (hotmark[g]) stamp[g] = next++;
            }
        *next_stamp = next;
    }

    /// Every objective's formInitialWorkingSet in order, then the activation order: what LexLSI_T::phase1_objectives leaves of a given x guess when
    /// no v0 is given.  ONE thread's work.  x: the guess, rewritten where P1_HOT_MODIFY_X says so (the caller's array is never this one).  hotmark: total
    /// bytes of scratch
    template <bool RAGGED = false>
    LEXLS_P1_FN void p1_hot_working_set(const StepShape &sh, const double *data, const uint32_t *var, double *x, uint32_t hot, uint8_t *cs, uint16_t *act, uint16_t *ina,
                                        uint16_t *ipos, uint16_t *na, uint32_t *stamp, uint32_t *next_stamp, uint8_t *hotmark, const uint32_t *cnt = nullptr,
                                        uint32_t *branch = nullptr)
    {
        for (uint32_t g = 0; g < sh.total; g++) hotmark[g] = 0;
        for (uint32_t k = 0; k < sh.nObj; k++) p1_form_initial_working_set<RAGGED>(sh, data, var, x, hot, k, cs, act, ina, ipos, na, hotmark, cnt, branch);
        if (hot & (P1_HOT_TYPE_ACTIVE | P1_HOT_TYPE_INACTIVE)) p1_rebuild_stamps(sh, act, na, hotmark, stamp, next_stamp);
    }

    /// Objective::initialize_v0 (objective.h:162-193) for one constraint of activation type t: A x minus the active bound, minus the midpoint for an
    /// equality; an inactive one takes its violation (set_min_init_ctr_violation) or, with P1_HOT_V_MIDPOINT, zero inside [lb - tol, ub + tol] and the
    /// midpoint residual outside.  Independent per row: on the device lane = row
    LEXLS_P1_FN double p1_initial_v(uint32_t t, double ax, double lb, double ub, bool midpoint, double tol_feasibility, uint32_t *branch = nullptr)
    {
        if (t == CTR_ACTIVE_LB) return ax - lb;
        if (t == CTR_ACTIVE_UB) return ax - ub;
        if (t != CTR_INACTIVE) return ax - 0.5 * (lb + ub);
        if (!midpoint) return ax <= lb ? ax - lb : (ax >= ub ? ax - ub : 0.0);
        const bool inside = ax >= lb - tol_feasibility && ax <= ub + tol_feasibility;
        if (branch) branch[inside ? P1B_V_ZERO : P1B_V_MID]++;
        return inside ? 0.0 : ax - 0.5 * (lb + ub);
    }

    /// where an equality problem is posted: the arrays of the equality solver's in slab (lexls_lse_round_layout), all instances
    struct EqualityProblemSlab
    {
        uint32_t *dims, *nfixed, *fixed_idx;
        double *fixed_val;
        uint32_t *row_src, *row_ld;
        uint8_t *fixed_type, *ctr_type;
    };

    /// The equality problem of instance b's working set (lexlsi.h:968-982, objective.h:434-494): the active simple bounds become fixed variables
    /// (LB -> lb, UB / EQ -> ub), the active general rows are named by reference — first element in the instance's constraint data, leading
    /// dimension, the top bit for "right-hand side = ub".  Thread `lane` of `lanes` takes every lanes-th active constraint (one thread: 0 of 1).
    /// data is read here and may have been written by the caller (a relaxed bound): no const, no restrict
    LEXLS_P1_FN void lsi_form_equality_problem(const StepShape &sh, uint32_t off, uint32_t nObjL, uint32_t cap, uint32_t b, double *data, const uint32_t *var,
                                               const uint16_t *na, const uint16_t *act, const uint8_t *cs, const EqualityProblemSlab &o, uint32_t lane, uint32_t lanes)
    {
        const uint32_t n = sh.n;
        uint32_t counter = 0;
        for (uint32_t k = 0; k < sh.nObj; k++)
        {
            const uint32_t f = sh.first[k], dim = sh.dim[k], nak = na[k];
            const double *blk = data + sh.off[k];
            if (sh.simple[k])
            {
                if (lane == 0) o.nfixed[b] = nak;
                for (uint32_t i = lane; i < nak; i += lanes)
                {
                    const uint32_t c = act[f + i], t = cs[f + c];
                    const size_t p   = (size_t)b * n + i;
                    o.fixed_idx[p]   = var[c];
                    o.fixed_val[p]   = (t == CTR_ACTIVE_LB) ? blk[c] : blk[c + dim];
                    o.fixed_type[p]  = (uint8_t)t;
                }
            }
            else
            {
                if (lane == 0) o.dims[(size_t)b * nObjL + k - off] = nak;
                for (uint32_t i = lane; i < nak; i += lanes)
                {
                    const uint32_t c = act[f + i], t = cs[f + c];
                    const size_t p   = (size_t)b * cap + counter + i;
                    o.row_src[p]     = (uint32_t)(sh.off[k] + c);
                    o.row_ld[p]      = dim | (t == CTR_ACTIVE_LB ? 0u : 0x80000000u);
                    o.ctr_type[p]    = (uint8_t)t;
                }
                counter += nak;
            }
        }
        for (uint32_t r = counter + lane; r < cap; r += lanes) o.row_ld[(size_t)b * cap + r] = 0u;
    }
} // namespace
