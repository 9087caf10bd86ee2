// SlotLSE: the equality-solver facade a host LexLSI_T instance of a lock-step batch sees (look-ups into its group, lsi_batch_ctx.h); SlotStep: its side of the opt-in device-side step.
#pragma once
#include "lsi_batch_ctx.h"

namespace
{
    class SlotLSE
    {
    public:
        SlotLSE() : c(NULL), b(0), nVarFixed(0), nVarFixedInit(0) {}
        void bind(BatchCtx *ctx, uint32_t slot)
        {
            c = ctx;
            b = slot;
            x.resize(c->n);
            first_row.assign(c->nObjL, 0);
        }
        void resize(Index nVar_, Index nObj_, Index *maxObjDim)
        {
            if (!c) throw Exception("SlotLSE: not bound to a batch");
            if (nVar_ != c->n || nObj_ != c->nObjL) throw Exception("SlotLSE: shape differs from the batch");
            for (Index k = 0; k < nObj_; k++)
                if (maxObjDim[k] != c->maxdim[k]) throw Exception("SlotLSE: capacity differs from the batch");
        }
        void setParameters(const ParametersLexLSE &) {} // tolerance and regularization type of the batch handle are set once by the batch driver
        void setRegularizationFactor(Index ObjIndex, RealScalar factor)
        {
            double &f = c->reg_factor[(size_t)b * c->nObjL + ObjIndex];
            if (f != factor)
            {
                f = factor;
                c->reg_dirty.store(true);
            }
        }
        void setObjDim(Index *ObjDim_)
        {
            Index r = 0;
            for (Index k = 0; k < c->nObjL; k++)
            {
                c->dims[(size_t)b * c->nObjL + k] = ObjDim_[k];
                first_row[k]                      = r;
                r += ObjDim_[k];
            }
            nVarFixedInit = 0;
            if (c->gather) std::fill(c->row_ld.begin() + (size_t)b * c->cap, c->row_ld.begin() + (size_t)(b + 1) * c->cap, 0u);
        }
        /// row `CtrIndex` of the LOD = row of the resident constraint data (Objective::formLexLSE); false: not available, send numbers
        bool setCtrIndexed(Index CtrIndex, size_t first_element, Index ld, unsigned use_ub)
        {
            if (!c->gather) return false;
            c->row_src[(size_t)b * c->cap + CtrIndex] = static_cast<uint32_t>(first_element);
            c->row_ld[(size_t)b * c->cap + CtrIndex]  = static_cast<uint32_t>(ld) | (use_ub ? 0x80000000u : 0u);
            return true;
        }
        void setFixedVariablesCount(Index nf)
        {
            if (nf > c->n) throw Exception("Cannot fix more than nVar variables");
            nVarFixed    = nf;
            c->nfixed[b] = nf;
        }
        void fixVariable(Index VarIndex, RealScalar VarValue, ConstraintActivationType type = CTR_ACTIVE_UB)
        {
            const size_t o   = (size_t)b * c->n + nVarFixedInit++;
            c->fixed_idx[o]  = VarIndex;
            c->fixed_val[o]  = VarValue;
            c->fixed_type[o] = static_cast<uint8_t>(type);
        }
        void setCtrType(Index ObjIndex, Index CtrIndex, ConstraintActivationType type) { c->ctr_type[(size_t)b * c->cap + first_row[ObjIndex] + CtrIndex] = static_cast<uint8_t>(type); }
        void setCtrStrided(Index CtrIndex, const RealScalar *row, Index stride, RealScalar rhs)
        {
            double *L = c->lod + (size_t)b * c->pstride;
            for (Index j = 0; j < c->n; j++) L[CtrIndex + (size_t)j * c->cap] = row[(size_t)j * stride];
            L[CtrIndex + (size_t)c->n * c->cap] = rhs;
        }
        // served by the batch call of this round
        void factorize() {}
        void solve()
        {
            for (Index i = 0; i < c->n; i++) x(i) = c->x[(size_t)b * c->n + i];
        }
        bool ObjectiveSensitivity(Index, Index &CtrIndex2Remove, int &ObjIndex2Remove, RealScalar, RealScalar, RealScalar &maxAbsValue)
        {
            const int32_t *s3 = &c->sens[(size_t)b * 3];
            maxAbsValue       = c->maxabs[b];
            if (s3[0])
            {
                CtrIndex2Remove = static_cast<Index>(s3[1]);
                ObjIndex2Remove = s3[2];
            }
            return s3[0] != 0;
        }
        /// the collecting overload (lexlse.h:511-602): the set the stage's lexls_lse_sensitivity_collect left, in the reference's push order (levels
        /// from the objective the search stopped at downwards, then the fixed variables).  The stage went through the objectives by itself
        /// (lexls_lse_set_sensitivity_scan): a call for a later objective finds the same — empty — set.
        void ObjectiveSensitivity(Index, RealScalar, RealScalar, std::vector<ConstraintInfo> &ctr_wrong_sign)
        {
            if (!c->first_wrong_sign) throw Exception("SlotLSE: the stage did not collect the wrong-sign set");
            const int32_t *s3 = &c->sens[(size_t)b * 3];
            if (!s3[0]) return;
            const uint8_t *ws = c->wrong_sign_host.data() + (size_t)b * (c->n + c->cap);
            for (Index k = static_cast<Index>(s3[2]) + 1; k--;)
                for (Index i = 0; i < getDim(k); i++)
                    if (ws[c->n + first_row[k] + i]) ctr_wrong_sign.push_back(ConstraintInfo(static_cast<int>(k), static_cast<int>(i)));
            for (Index i = 0; i < nVarFixed; i++)
                if (ws[i]) ctr_wrong_sign.push_back(ConstraintInfo(-1, static_cast<int>(i)));
        }
        const dVectorType &get_x() const { return x; }
        Index getTotalRank() const { return c->totalrank[b]; }
        Index getDim(Index k) const { return c->dims[(size_t)b * c->nObjL + k]; }
        Index getFixedVariablesCount() const { return nVarFixed; }

    private:
        BatchCtx *c;
        uint32_t b;
        Index nVarFixed, nVarFixedInit;
        std::vector<Index> first_row;
        dVectorType x;
    };

    typedef internal::LexLSI_T<SlotLSE> SlotLSI;

    /// One instance's side of the device-side step (LexLSI_T::StepHook): posts the working set of the equality problem just formed,
    /// hands x / v / A x over to the device the first time, and reads the ratio test's verdict back.
    struct SlotStep : SlotLSI::StepHook
    {
        BatchCtx *c = NULL;
        uint32_t b  = 0;
        void prepare(const dVectorType &x, const std::vector<internal::Objective> &obj) override
        {
            const StepShape &sh = c->shape;
            uint8_t *cs         = c->wl.ctr_state(c->wset_host.data(), b);
            std::memset(cs, 0, sh.total);
            uint16_t *ip        = c->wl.inact_pos(c->wset_host.data(), b);
            walk_working_set(obj, sh.nObj, [&](uint32_t k, Index, Index ctr, ConstraintActivationType t) { cs[sh.first[k] + ctr] = static_cast<uint8_t>(t); },
                             [&](uint32_t k, Index i, Index ctr) { ip[sh.first[k] + ctr] = static_cast<uint16_t>(i); });
            if (!c->on_device[b])
            {
                pack_state(c->state_host.data() + (size_t)b * sh.SD, sh, x, obj);
                c->on_device[b] = 1;
                c->mode()[b]    = 2;
                c->handover.store(true);
            }
            else
                c->mode()[b] = 1;
        }
        bool blocking(Index &ObjIndex, Index &CtrIndex, ConstraintActivationType &CtrType, RealScalar &alpha) override
        {
            const double *r = c->res_host.data() + (size_t)b * 4;
            alpha           = r[0];
            if (r[1] < 0.0) return false;
            ObjIndex = static_cast<Index>(r[1]);
            CtrIndex = static_cast<Index>(r[2]);
            CtrType  = static_cast<ConstraintActivationType>(static_cast<int>(r[3]));
            return true;
        }
    };
} // namespace
