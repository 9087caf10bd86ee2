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
