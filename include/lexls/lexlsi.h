/*
 * Derived work: this header restates, for a different equality-solver back end, host-side interface and control flow of
 * jrl-umi3218/lexls (include/lexls/lexlsi.h), whose notice is retained as its BSD 3-clause licence requires:
 *
 * Copyright 2013-2021 INRIA
 *
 * Redistribution and use in source and binary forms, with or without modification, are permitted provided that the following
 * conditions are met:
 * 1. Redistributions of source code must retain the above copyright notice, this list of conditions and the following disclaimer.
 * 2. Redistributions in binary form must reproduce the above copyright notice, this list of conditions and the following disclaimer
 *    in the documentation and/or other materials provided with the distribution.
 * 3. Neither the name of the copyright holder nor the names of its contributors may be used to endorse or promote products derived
 *    from this software without specific prior written permission.
 *
 * THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS "AS IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT
 * NOT LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR PURPOSE ARE DISCLAIMED. IN NO EVENT SHALL
 * THE COPYRIGHT HOLDER OR CONTRIBUTORS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES
 * (INCLUDING, BUT NOT LIMITED TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR PROFITS; OR BUSINESS
 * INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING NEGLIGENCE
 * OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE OF THIS SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
 */
// Primal active-set driver for lexicographic least-squares with inequalities (host side).
//
// North star: "LexLSI's outer active-set loop is kept on the host"; the equality solver it calls
// once per iteration is the accelerated hot path.  The driver is therefore a template over the
// equality-solver type LSE:
//     LexLS::internal::LexLSI            = LexLSI_T<LexLS::internal::LexLSE>  (HIP-backed, lexlse.h)
//     oracle: LexLSI_T<lexls_oracle::LexLSE>                                  (CPU restatement)
// so the very same driver logic runs on both sides of a parity test.
//
// Behaviour restated from the reference include/lexls/lexlsi.h (cited per method).  Known oddities
// of the reference are kept on purpose: reset() does not clear
// x_guess_is_specified (lexlsi.h:97 shadows it).
#pragma once

#include <lexls/cycling.h>
#include <lexls/objective.h>

namespace LexLS
{
    namespace internal
    {
        template <class LSE>
        class LexLSI_T
        {
        public:
            /// lexlsi.h:51-58
            LexLSI_T(Index nVar_, Index nObj_, Index *ObjDim_, ObjectiveType *ObjType_)
            : nVar(nVar_), nObj(nObj_), x_guess_is_specified(false), status(TERMINATION_STATUS_UNKNOWN)
            {
                parameters.setDefaults();
                setParameters(parameters);
                resize(ObjDim_, ObjType_);
            }

            /// lexlsi.h:63-67
            LexLSI_T() : nVar(0), nObj(0), x_guess_is_specified(false), status(TERMINATION_STATUS_UNKNOWN)
            {
                parameters.setDefaults();
                setParameters(parameters);
            }

            /// lexlsi.h:77-83
            void resize(Index nVar_, Index nObj_, Index *ObjDim_, ObjectiveType *ObjType_)
            {
                nVar = nVar_;
                nObj = nObj_;
                resize(ObjDim_, ObjType_);
            }

            /// lexlsi.h:88-104 (x_guess_is_specified intentionally NOT cleared: reference quirk)
            void reset()
            {
                for (Index k = 0; k < nObj; k++) objectives[k].resetActiveSet();
                initialize();
                std::fill(nActive.begin(), nActive.end(), 0u);
                status = TERMINATION_STATUS_UNKNOWN;
                working_set_log.clear();
                cycling_handler.reset();
                WS.clear();
            }

            /// lexlsi.h:120-136
            void api_activate(Index ObjIndex, Index CtrIndex, ConstraintActivationType type)
            {
                if (objectives[ObjIndex].isActive(CtrIndex)) return;
                if (type == CTR_ACTIVE_LB || type == CTR_ACTIVE_UB)
                    activate(ObjIndex, CtrIndex, type, false);
                else
                    printf("WARNING: the user cannot define explicitly which constraints are of type CTR_ACTIVE_EQ \n\n");
            }

            /// lexlsi.h:148-173
            void activate(Index ObjIndex, Index CtrIndex, ConstraintActivationType type, bool CountActivation = true)
            {
                if (ObjIndex >= nObj) throw Exception("ObjIndex >= nObj");
                WS.push_back(ConstraintInfo(ObjIndex, CtrIndex));
                objectives[ObjIndex].activate(CtrIndex, type);
                if (CountActivation)
                {
                    nActivations++;
                    if (objectives[ObjIndex].isZeroNormal(CtrIndex))
                        printf("WARNING: activated inequality constraint (0*x = b): (obj_index = %d, ctr_index = %d) \n", ObjIndex, CtrIndex);
                }
            }

            /// lexlsi.h:181-198
            void deactivate(Index ObjIndex, Index CtrIndexActive)
            {
                if (ObjIndex >= nObj) throw Exception("ObjIndex >= nObj");
                typename std::vector<ConstraintInfo>::iterator it =
                    std::find(WS.begin(), WS.end(), ConstraintInfo(ObjIndex, objectives[ObjIndex].getActiveCtrIndex(CtrIndexActive)));
                if (it != WS.end()) WS.erase(it); // (the reference erases WS.end() when the entry is missing: undefined behaviour)
                objectives[ObjIndex].deactivate(CtrIndexActive);
                nDeactivations++;
            }

            /// lexlsi.h:205-246.  ONE form of the driver: the resumable state machine below (begin / advance), which cuts an iteration
            /// (the reference's verifyWorkingSet, lexlsi.h:1144-1265) at the points where the equality solver is used; a stand-alone
            /// equality solver computes on the spot there, a lock-step batch serves the pending requests of all its instances first.
            TerminationStatus solve()
            {
                begin();
                while (!finished()) advance();
                return status;
            }

            /// lexlsi.h:306-310
            void set_x0(const dVectorType &x0)
            {
                x                    = x0;
                x_guess_is_specified = true;
            }

            /// lexlsi.h:317-320
            void set_v0(Index ObjIndex, dVectorType &v0_) { objectives[ObjIndex].set_v0(v0_); }

            /// lexlsi.h:325-342
            void setParameters(const ParametersLexLSI &parameters_)
            {
                parameters = parameters_;
                ParametersLexLSE p;
                p.tol_linear_dependence          = parameters.tol_linear_dependence;
                p.regularization_type            = parameters.regularization_type;
                p.max_number_of_CG_iterations    = parameters.max_number_of_CG_iterations;
                p.variable_regularization_factor = parameters.variable_regularization_factor;
                lexlse.setParameters(p);
                if (parameters.cycling_handling_enabled)
                {
                    cycling_handler.set_max_counter(parameters.cycling_max_counter);
                    cycling_handler.set_relax_step(parameters.cycling_relax_step);
                }
            }

            /// lexlsi.h:350-435: general objective, data = [A, lb, ub]; rows with |lb-ub| < 1e-15 and a
            /// non-zero normal are activated as equalities
            /// see Objective::setDataOffset (batched device backend only)
            void setDataOffset(Index ObjIndex, size_t off) { objectives[ObjIndex].setDataOffset(off); }

            void setData(Index ObjIndex, const dMatrixConstRef &data)
            {
                if (ObjIndex >= nObj) throw Exception("ObjIndex >= nObj");
                if (objectives[ObjIndex].getObjType() != GENERAL_OBJECTIVE) throw Exception("ObjType = GENERAL_OBJECTIVE is assumed");
                if (objectives[ObjIndex].getDim() != data.rows()) throw Exception("Incorrect number of equations");

                for (Index c = 0; c < objectives[ObjIndex].getDim(); c++)
                {
                    const RealScalar bl = data(c, nVar);
                    const RealScalar bu = data(c, nVar + 1);
                    if (isEqual(bl, bu))
                    {
                        RealScalar s = 0.0;
                        for (Index j = 0; j < nVar; j++) s = std::fma(data(c, j), data(c, j), s);
                        if (s > 0) activate(ObjIndex, c, CTR_ACTIVE_EQ, false);
                    }
                    else if (bl > bu)
                    {
                        throw Exception("(general) Lower bound is greater than upper bound.");
                    }
                }
                objectives[ObjIndex].setData(data);
            }

            /// lexlsi.h:444-491: simple bounds, data = [lb, ub], VarIndex 0-based and unique
            void setData(Index ObjIndex, Index *VarIndex, const dMatrixConstRef &data)
            {
                if (ObjIndex >= nObj) throw Exception("ObjIndex >= nObj");
                if (objectives[ObjIndex].getObjType() != SIMPLE_BOUNDS_OBJECTIVE) throw Exception("ObjType = SIMPLE_BOUNDS_OBJECTIVE is assumed");
                if (objectives[ObjIndex].getDim() != data.rows()) throw Exception("Incorrect number of equations");

                const Index dim = objectives[ObjIndex].getDim();
                for (Index c = 0; c < dim; c++)
                {
                    const RealScalar bl = data(c, 0);
                    const RealScalar bu = data(c, 1);
                    if (isEqual(bl, bu))
                        activate(ObjIndex, c, CTR_ACTIVE_EQ, false);
                    else if (bl > bu)
                        throw Exception("(simple) Lower bound is greater than upper bound.");
                }
                for (Index k = 0; k < dim; k++)
                    for (Index j = 0; j < dim; j++)
                        if (VarIndex[k] == VarIndex[j] && j != k) throw Exception("Elements of VarIndex are not unique.");

                objectives[ObjIndex].setData(VarIndex, data);
            }

            void setRegularizationFactor(Index ObjIndex, RealScalar factor) { objectives[ObjIndex].setRegularization(factor); }

            const dVectorType &get_x() const { return x; }

            /// lexlsi.h:519-526
            const dVectorType &get_xStar()
            {
                formLexLSE();
                lexlse.factorize();
                lexlse.solve();
                return lexlse.get_x();
            }

            const dVectorType &get_v(Index ObjIndex) const { return objectives[ObjIndex].get_v(); }
            void getConstraintViolation(Index ObjIndex, dVectorType &ctr_violation) const { objectives[ObjIndex].getConstraintViolation(ctr_violation); }

            /// lexlsi.h:552-605: Lagrange multipliers of every objective w.r.t. every constraint, in
            /// the user's constraint order; vec_lambda[k] is (dim_k x nObj)
            void getLambda(std::vector<dMatrixType> &vec_lambda)
            {
                Index nActiveCtr = 0;
                vec_lambda.resize(nObj);
                for (Index k = 0; k < nObj; k++)
                {
                    nActiveCtr += objectives[k].getActiveCtrCount();
                    vec_lambda[k].resize(getObjDim(k), nObj);
                }
                if (status != PROBLEM_SOLVED)
                {
                    formLexLSE();
                    lexlse.factorize();
                }

                OneLevelPerCall one_level(lexlse, sens_scans_all);
                dMatrixType L_active(nActiveCtr, nObj);
                Index nMeaningful = lexlse.getFixedVariablesCount();
                Index CtrIndex2Remove;
                int ObjIndex2Remove;
                RealScalar maxAbsValue;
                for (Index k = 0; k < nObj - nObjOffset; k++)
                {
                    lexlse.ObjectiveSensitivity(k, CtrIndex2Remove, ObjIndex2Remove, parameters.tol_wrong_sign_lambda, parameters.tol_correct_sign_lambda,
                                                maxAbsValue);
                    nMeaningful += lexlse.getDim(k);
                    const dVectorType &w = lexlse.getWorkspace();
                    for (Index i = 0; i < nMeaningful; i++) L_active(i, nObjOffset + k) = w(i);
                }

                Index accumulate_active_ctr = 0;
                for (Index k = 0; k < nObj; k++)
                {
                    for (Index a = 0; a < objectives[k].getActiveCtrCount(); a++)
                    {
                        const Index ind = objectives[k].getActiveCtrIndex(a);
                        for (Index j = 0; j < nObj; j++) vec_lambda[k](ind, j) = L_active(accumulate_active_ctr + a, j);
                    }
                    accumulate_active_ctr += objectives[k].getActiveCtrCount();
                }
            }

            const dMatrixType &get_lexqr() { return lexlse.get_lexqr(); }
            const dMatrixType &get_data() { return lexlse.get_data(); }
            /// lexlsi.h:617-630: by-products of REGULARIZATION_TIKHONOV_1 in the last equality problem
            const dMatrixType &get_X_mu() { return lexlse.get_X_mu(); }
            const dMatrixType &get_X_mu_rhs() { return lexlse.get_X_mu_rhs(); }
            const dVectorType &get_residual_mu() { return lexlse.get_residual_mu(); }

            Index getCyclingCounter() const { return cycling_handler.get_counter(); }
            /// the cycling handler itself: a backend that takes the iterations over at atIterationSolve() continues from its state
            CyclingHandler &getCyclingHandler() { return cycling_handler; }
            const CyclingHandler &getCyclingHandler() const { return cycling_handler; }
            Index getFactorizationsCount() const { return nFactorizations; }
            Index getActivationsCount() const { return nActivations; }
            Index getDeactivationsCount() const { return nDeactivations; }
            Index getIterationsCount() const { return nIterations; }
            Index getActiveCtrCount(Index ObjIndex) const { return objectives[ObjIndex].getActiveCtrCount(); }
            Index getActiveCtrCount() const
            {
                Index n = 0;
                for (Index k = 0; k < nObj; k++) n += objectives[k].getActiveCtrCount();
                return n;
            }

            /// lexlsi.h:688-698
            void getActiveCtr(Index ObjIndex, std::vector<ConstraintActivationType> &ctr_type) const
            {
                ctr_type.assign(objectives[ObjIndex].getDim(), CTR_INACTIVE);
                for (Index k = 0; k < objectives[ObjIndex].getActiveCtrCount(); k++)
                    ctr_type[objectives[ObjIndex].getActiveCtrIndex(k)] = objectives[ObjIndex].getActiveCtrType(k);
            }

            /// lexlsi.h:703-716
            void getActiveCtr_order(std::vector<ConstraintIdentifier> &ctr) const
            {
                for (Index o = 0; o < nObj; o++)
                    for (Index k = 0; k < objectives[o].getActiveCtrCount(); k++)
                        ctr.push_back(ConstraintIdentifier(o, objectives[o].getActiveCtrIndex(k), objectives[o].getActiveCtrType(k)));
            }

            Index getObjectivesCount() const { return nObj; }
            Index getObjDim(Index ObjIndex) const { return objectives[ObjIndex].getDim(); }
            std::vector<WorkingSetLogEntry> &getWorkingSetLog() { return working_set_log; }
            const std::vector<WorkingSetLogEntry> &getWorkingSetLog() const { return working_set_log; }
            Index getTotalRank() { return lexlse.getTotalRank(); }
            TerminationStatus getStatus() const { return status; }
            LSE &getLexLSE() { return lexlse; }
            const ParametersLexLSI &getParameters() const { return parameters; }

            // -------------------------------------------------------------------------------------
            // The steps of one active-set iteration, public so that a lock-step batched driver can
            // interleave the device calls of many instances (lexls_amd BatchedLexLSI).
            // -------------------------------------------------------------------------------------

            /// lexlsi.h:968-982
            void formLexLSE()
            {
                for (Index k = 0; k < nObj; k++) nActive[k] = objectives[k].getActiveCtrCount();
                lexlse.setObjDim(&nActive[0] + nObjOffset);
                Index counter = 0;
                for (Index k = 0; k < nObj; k++) objectives[k].formLexLSE(lexlse, counter, k - nObjOffset);
            }

            /// lexlsi.h:987-994
            void formStep()
            {
                const dVectorType &xs = lexlse.get_x();
                for (Index i = 0; i < nVar; i++) dx(i) = xs(i) - x(i);
                for (Index k = 0; k < nObj; k++) objectives[k].formStep(dx);
            }

            /// lexlsi.h:1006-1029: shared alpha across objectives, ascending objective index
            bool checkBlockingConstraints(Index &ObjIndexBlocking, Index &CtrIndexBlocking, ConstraintActivationType &CtrTypeBlocking, RealScalar &alpha)
            {
                alpha = 1;
                for (Index k = 0; k < nObj; k++)
                    if (objectives[k].checkBlockingConstraints(CtrIndexBlocking, CtrTypeBlocking, alpha, parameters.tol_feasibility)) ObjIndexBlocking = k;
                return alpha < 1;
            }

            /// lexlsi.h:816-869
            void phase1()
            {
                hot_start_related_tests();
                if (!x_guess_is_specified)
                {
                    formLexLSE();
                    lexlse.factorize();
                    lexlse.solve();
                    lexlse_rank = getTotalRank();
                    x           = lexlse.get_x();
                }
                phase1_objectives();
                if (x_guess_is_specified)
                {
                    formLexLSE();
                    lexlse.factorize();
                    lexlse.solve();
                    lexlse_rank = getTotalRank();
                    const dVectorType &xs = lexlse.get_x();
                    for (Index i = 0; i < nVar; i++) dx(i) = xs(i) - x(i);
                }
                for (Index k = 0; k < nObj; k++) objectives[k].formStep(dx);
                nFactorizations++;
            }

            /// lexlsi.h:880-915
            void phase1_v0()
            {
                if (!x_guess_is_specified) throw Exception("when use_phase1_v0 = true, x_guess has to be specified");
                hot_start_related_tests();
                phase1_objectives();
                for (Index k = 0; k < nObj; k++) objectives[k].formStep(dx);
            }

            // -------------------------------------------------------------------------------------
            // Resumable form of solve() for LOCK-STEP BATCHES (config 5: many LexLSI instances whose equality
            // solves are served by ONE batched device call per round).  Same statements as the reference's phase1() +
            // verifyWorkingSet() (lexlsi.h:1144-1265), cut at the points where the equality solver is used:
            //     begin();  while (!finished()) { <serve need()> ; advance(); }
            // advance() itself calls lexlse.factorize()/solve()/ObjectiveSensitivity(); an LSE whose results
            // were pre-computed by a batch call implements them as look-ups (lexls_amd/csrc/lexls_lsi_capi.hip),
            // a stand-alone LSE computes on the spot, so solve_resumable() == solve() for any LSE.
            // -------------------------------------------------------------------------------------
            /// Optional owner of the step of an iteration (a backend that keeps x, v, A*x and the constraint data resident
            /// can form the step, run the ratio test and update the state next to its equality solve).  Absent (NULL) everywhere but
            /// in lock-step device batches; with it the statements of lexlsi.h:987-1029 / :1234-1240 are executed by the hook, from the
            /// second iteration on (the first one belongs to phase 1 and stays here).
            struct StepHook
            {
                virtual ~StepHook() {}
                /// the working set of the equality problem just formed (lexlsi.h:968-982); on the first call x / v / A*x leave the host
                virtual void prepare(const dVectorType &x, const std::vector<Objective> &objectives) = 0;
                /// result of checkBlockingConstraints (lexlsi.h:1006-1029) for the iteration whose equality problem was just solved
                virtual bool blocking(Index &ObjIndex, Index &CtrIndex, ConstraintActivationType &CtrType, RealScalar &alpha) = 0;
            };
            /// an equality solver that can scan several levels per call (setSensitivityScan) is told to do one level per call while
            /// the multipliers of every single level are wanted
            struct OneLevelPerCall
            {
                template <class L>
                static auto set(L &l, bool on, int) -> decltype(l.setSensitivityScan(on), void())
                {
                    l.setSensitivityScan(on);
                }
                template <class L>
                static void set(L &, bool, ...)
                {
                }
                OneLevelPerCall(LSE &l, bool active_) : lse(l), active(active_)
                {
                    if (active) set(lse, false, 0);
                }
                ~OneLevelPerCall()
                {
                    if (active) set(lse, true, 0);
                }
                LSE &lse;
                bool active;
            };
            void setStepHook(StepHook *hook) { step_hook = hook; }
            /// the equality solver's ObjectiveSensitivity(level) goes on through the following levels by itself until one reports a
            /// wrong-sign multiplier (a backend that serves the removal search of lexlsi.h:1121-1132 in one call): "not found" is then final
            void setSensitivityScansAllLevels(bool on) { sens_scans_all = on; }

            enum DeviceNeed
            {
                NEED_NOTHING = 0,
                NEED_FACTORIZE_SOLVE,
                NEED_SENSITIVITY
            };

            /// what the next advance() will ask the equality solver for (and, for sensitivity, at which LexLSE level)
            DeviceNeed need() const { return pending; }
            /// the equality problem of a regular iteration (not phase 1) is formed and waits for its solve: from here on an iteration is
            /// "solve, step, one working-set change, form the next problem" — the point where a backend that keeps x, v, A*x AND the
            /// working sets resident can run whole iterations by itself (lock-step device batches)
            bool atIterationSolve() const { return pc == PC_IT_SOLVED && pending == NEED_FACTORIZE_SOLVE; }
            const std::vector<Objective> &getObjectives() const { return objectives; }
            /// the active constraints in the order they entered the working set (the list findFirstCtrWrongSign walks, lexlsi.h:1034-1046): a
            /// backend that takes the iterations over (lock-step device batches) carries the order on as one activation stamp per constraint
            const std::vector<ConstraintInfo> &getActivationOrder() const { return WS; }
            Index needLevel() const { return sens_level; }
            bool finished() const { return pc == PC_DONE; }

            void begin()
            {
                if (parameters.use_phase1_v0)
                {
                    phase1_v0();
                    iteration_prepare();
                    return;
                }
                hot_start_related_tests();
                if (!x_guess_is_specified)
                {
                    formLexLSE();
                    pc      = PC_P1_SOLVED_NO_GUESS;
                    pending = NEED_FACTORIZE_SOLVE;
                }
                else
                {
                    phase1_objectives_then_maybe_solve();
                }
            }

            void advance()
            {
                switch (pc)
                {
                case PC_P1_SOLVED_NO_GUESS:
                    lexlse.factorize();
                    lexlse.solve();
                    lexlse_rank = getTotalRank();
                    x           = lexlse.get_x();
                    phase1_objectives_then_maybe_solve();
                    break;
                case PC_P1_SOLVED_WITH_GUESS:
                {
                    lexlse.factorize();
                    lexlse.solve();
                    lexlse_rank           = getTotalRank();
                    const dVectorType &xs = lexlse.get_x();
                    for (Index i = 0; i < nVar; i++) dx(i) = xs(i) - x(i);
                    phase1_finish();
                    break;
                }
                case PC_IT_SOLVED:
                    lexlse.factorize();
                    lexlse.solve();
                    lexlse_rank = getTotalRank();
                    it_hooked   = step_hook != NULL;
                    if (!it_hooked) formStep();
                    nFactorizations++;
                    iteration_blocking();
                    break;
                case PC_IT_SENSITIVITY:
                {
                    Index CtrIndex2Remove = 0;
                    int ObjIndex2Remove   = 0;
                    RealScalar lambda_wrong_sign;
                    bool found;
                    if (parameters.deactivate_first_wrong_sign)
                    {
                        // lexlsi.h:1063-1105: collects every wrong-sign multiplier level by level (an equality solver of a lock-step batch hands
                        // out the set its stage collected); the objective index comes back absolute
                        Index o_abs = 0;
                        found       = findActiveCtr2Remove_first(o_abs, CtrIndex2Remove, lambda_wrong_sign);
                        ObjIndex2Remove = static_cast<int>(o_abs) - static_cast<int>(nObjOffset);
                        sens_level      = nObj - nObjOffset; // every level has been looked at
                    }
                    else
                        found = lexlse.ObjectiveSensitivity(sens_level, CtrIndex2Remove, ObjIndex2Remove, parameters.tol_wrong_sign_lambda,
                                                            parameters.tol_correct_sign_lambda, lambda_wrong_sign);
                    if (found)
                    {
                        const Index o = static_cast<Index>(ObjIndex2Remove + static_cast<int>(nObjOffset));
                        if (parameters.log_working_set_enabled)
                            working_set_log.push_back(WorkingSetLogEntry(o, objectives[o].getActiveCtrIndex(CtrIndex2Remove), CTR_INACTIVE, lambda_wrong_sign, lexlse_rank));
                        it_constraint.set(o, objectives[o].getActiveCtrIndex(CtrIndex2Remove), objectives[o].getActiveCtrType(CtrIndex2Remove));
                        it_operation = OPERATION_REMOVE;
                        deactivate(o, CtrIndex2Remove);
                        iteration_finish();
                    }
                    else if (!sens_scans_all && sens_level + 1 < nObj - nObjOffset)
                    {
                        sens_level++;
                        pending = NEED_SENSITIVITY;
                    }
                    else
                    {
                        status = PROBLEM_SOLVED;
                        iteration_finish();
                    }
                    break;
                }
                default:
                    throw Exception("LexLSI::advance() called in a state without pending work");
                }
            }

            /// kept for callers of the earlier two-form interface
            TerminationStatus solve_resumable() { return solve(); }

        private:
            enum ProgramCounter
            {
                PC_IDLE = 0,
                PC_P1_SOLVED_NO_GUESS,
                PC_P1_SOLVED_WITH_GUESS,
                PC_IT_SOLVED,
                PC_IT_SENSITIVITY,
                PC_DONE
            };

            /// The objectives' phase 1 (lexlsi.h:838-846 / :892-900), and the activation-order list behind it.  Objective::formInitialWorkingSet
            /// (modify_type_active_enabled / modify_type_inactive_enabled with an x guess) activates, deactivates and re-types constraints at objective
            /// level, behind the back of WS, the list findFirstCtrWrongSign walks.  The reference leaves WS as it was: a later removal of a
            /// constraint activated there erases WS.end(), and under deactivate_first_wrong_sign the walk runs off the list — undefined behaviour
            /// both.  Here WS is rebuilt behind the loop: first the entries that are still active with the type they had, in their order; then the
            /// constraints formInitialWorkingSet activated or re-activated, objective by objective, in the order they entered the objective's
            /// active list.  nActivations / nDeactivations are not touched and nothing is logged, as in the reference.  For modify_type_*
            /// combined with deactivate_first_wrong_sign the reference has no defined result and this order is ours; for every other
            /// combination x, v, the active set and the counters are the reference's.  With the flags off nothing is done.
            void phase1_objectives()
            {
                const bool hot = x_guess_is_specified && (parameters.modify_type_active_enabled || parameters.modify_type_inactive_enabled);
                std::vector<ConstraintActivationType> before;
                if (hot)
                    for (size_t p = 0; p < WS.size(); p++)
                        before.push_back(objectives[WS[p].get_obj_index()].getCtrType(static_cast<Index>(WS[p].get_ctr_index())));
                for (Index k = 0; k < nObj; k++)
                    objectives[k].phase1(x, x_guess_is_specified, parameters.modify_type_active_enabled, parameters.modify_type_inactive_enabled,
                                         parameters.modify_x_guess_enabled, parameters.set_min_init_ctr_violation, parameters.tol_feasibility);
                if (!hot) return;
                std::vector<ConstraintInfo> order;
                std::vector<std::vector<char>> kept(nObj);
                for (Index k = 0; k < nObj; k++) kept[k].assign(objectives[k].getDim(), 0);
                for (size_t p = 0; p < WS.size(); p++)
                {
                    const Index o = static_cast<Index>(WS[p].get_obj_index()), c = static_cast<Index>(WS[p].get_ctr_index());
                    if (objectives[o].getCtrType(c) != CTR_INACTIVE && objectives[o].getCtrType(c) == before[p])
                    {
                        order.push_back(WS[p]);
                        kept[o][c] = 1;
                    }
                }
                for (Index k = 0; k < nObj; k++)
                    for (Index a = 0; a < objectives[k].getActiveCtrCount(); a++)
                        if (!kept[k][objectives[k].getActiveCtrIndex(a)]) order.push_back(ConstraintInfo(k, objectives[k].getActiveCtrIndex(a)));
                WS.swap(order);
            }

            void phase1_objectives_then_maybe_solve()
            {
                phase1_objectives();
                if (x_guess_is_specified)
                {
                    formLexLSE();
                    pc      = PC_P1_SOLVED_WITH_GUESS;
                    pending = NEED_FACTORIZE_SOLVE;
                }
                else
                {
                    phase1_finish();
                }
            }

            void phase1_finish()
            {
                for (Index k = 0; k < nObj; k++) objectives[k].formStep(dx);
                nFactorizations++;
                iteration_prepare();
            }

            /// head of verifyWorkingSet() (lexlsi.h:1161-1179)
            void iteration_prepare()
            {
                it_operation = OPERATION_UNDEFINED;
                it_constraint.set(0, 0, CTR_INACTIVE);
                it_normal = true;
                it_hooked = false;
                if (nIterations != 0)
                {
                    formLexLSE();
                    if (step_hook) step_hook->prepare(x, objectives);
                    pc      = PC_IT_SOLVED;
                    pending = NEED_FACTORIZE_SOLVE;
                }
                else
                {
                    if (parameters.use_phase1_v0) it_normal = false;
                    iteration_blocking();
                }
            }

            /// lexlsi.h:1181-1232 up to the point where multipliers are needed
            void iteration_blocking()
            {
                Index o = 0, c = 0;
                ConstraintActivationType t = CTR_INACTIVE;
                if (it_hooked ? step_hook->blocking(o, c, t, it_alpha) : checkBlockingConstraints(o, c, t, it_alpha))
                {
                    it_constraint.set(o, c, t);
                    if (parameters.log_working_set_enabled) working_set_log.push_back(WorkingSetLogEntry(o, c, t, it_alpha, lexlse_rank));
                    it_operation = OPERATION_ADD;
                    activate(o, c, t);
                    iteration_finish();
                }
                else if (it_normal && nObj - nObjOffset > 0)
                {
                    sens_level = 0;
                    pc         = PC_IT_SENSITIVITY;
                    pending    = NEED_SENSITIVITY;
                }
                else
                {
                    if (it_normal) status = PROBLEM_SOLVED;
                    iteration_finish();
                }
            }

            /// tail of verifyWorkingSet() (lexlsi.h:1234-1264) + the termination test of solve() (:232-243)
            void iteration_finish()
            {
                step_length = (it_operation == OPERATION_ADD) ? it_alpha : -1;
                if (it_alpha > 0 && !it_hooked) // (a hook has applied the step to the state it owns)
                {
                    for (Index i = 0; i < nVar; i++) x(i) += it_alpha * dx(i);
                    for (Index k = 0; k < nObj; k++) objectives[k].step(it_alpha);
                }
                if (parameters.cycling_handling_enabled && it_operation != OPERATION_UNDEFINED)
                {
                    bool cycling_detected;
                    status = cycling_handler.update(it_operation, it_constraint, objectives, cycling_detected);
                    if (parameters.log_working_set_enabled) working_set_log.back().cycling_detected = cycling_detected;
                }
                nIterations++;
                pending = NEED_NOTHING;
                if (status == PROBLEM_SOLVED || status == PROBLEM_SOLVED_CYCLING_HANDLING)
                {
                    pc = PC_DONE;
                }
                else if (nFactorizations >= parameters.max_number_of_factorizations)
                {
                    status = MAX_NUMBER_OF_FACTORIZATIONS_EXCEEDED;
                    pc     = PC_DONE;
                }
                else
                {
                    iteration_prepare();
                }
            }

            ProgramCounter pc      = PC_IDLE;
            DeviceNeed pending     = NEED_NOTHING;
            Index sens_level       = 0;
            OperationType it_operation = OPERATION_UNDEFINED;
            ConstraintIdentifier it_constraint;
            RealScalar it_alpha = 1;
            bool it_normal      = true;
            bool it_hooked      = false; // this iteration's step is formed and applied by step_hook
            StepHook *step_hook = NULL;
            bool sens_scans_all = false;

            /// lexlsi.h:758-793
            void hot_start_related_tests()
            {
                bool v0_is_only_partially_specified = false;
                bool user_attempted_to_specify_v0   = objectives[0].getFlag_v0_is_specified();
                for (Index k = 1; k < nObj; k++)
                {
                    if (objectives[k].getFlag_v0_is_specified() != user_attempted_to_specify_v0)
                    {
                        printf("WARNING: disregarding v0 because it is only partially initialized. \n");
                        user_attempted_to_specify_v0   = true;
                        v0_is_only_partially_specified = true;
                        break;
                    }
                }
                bool forgot_x_guess = false;
                if (!x_guess_is_specified && user_attempted_to_specify_v0)
                {
                    printf("WARNING: disregarding v0 because x_guess is not set. \n");
                    forgot_x_guess = true;
                }
                if (v0_is_only_partially_specified || forgot_x_guess)
                    for (Index k = 0; k < nObj; k++) objectives[k].setFlag_v0_is_specified(false);
            }

            /// lexlsi.h:923-946
            void resize(Index *ObjDim_, ObjectiveType *ObjType_)
            {
                nObjOffset = (ObjType_[0] == SIMPLE_BOUNDS_OBJECTIVE) ? 1 : 0;
                lexlse.resize(nVar, nObj - nObjOffset, ObjDim_ + nObjOffset);
                nActive.assign(nObj, 0);
                objectives.resize(nObj);
                for (Index k = 0; k < nObj; k++) objectives[k].resize(ObjDim_[k], nVar, ObjType_[k]);
                x.resize(nVar);
                dx.resize(nVar);
                initialize();
            }

            /// lexlsi.h:951-963
            void initialize()
            {
                nIterations     = 0;
                nActivations    = 0;
                nDeactivations  = 0;
                nFactorizations = 0;
                lexlse_rank     = 0;
                step_length     = 0;
                x.setZero();
                dx.setZero();
            }

            /// lexlsi.h:1034-1046
            Index findFirstCtrWrongSign(std::vector<ConstraintInfo> &ctr_wrong_sign)
            {
                Index k = 0;
                while (std::find(ctr_wrong_sign.begin(), ctr_wrong_sign.end(), WS[k]) == ctr_wrong_sign.end()) k++;
                return k;
            }

            /// lexlsi.h:1048-1060
            bool findActiveCtr2Remove(Index &ObjIndex2Remove, Index &CtrIndex2Remove, RealScalar &lambda_wrong_sign)
            {
                if (parameters.deactivate_first_wrong_sign) return findActiveCtr2Remove_first(ObjIndex2Remove, CtrIndex2Remove, lambda_wrong_sign);
                return findActiveCtr2Remove_largest(ObjIndex2Remove, CtrIndex2Remove, lambda_wrong_sign);
            }

            /// lexlsi.h:1063-1105
            bool findActiveCtr2Remove_first(Index &ObjIndex2Remove, Index &CtrIndex2Remove, RealScalar &lambda_wrong_sign)
            {
                OneLevelPerCall one_level(lexlse, sens_scans_all);
                std::vector<ConstraintInfo> ctr_wrong_sign;
                lambda_wrong_sign = 0;
                bool found        = false;
                for (Index k = 0; k < nObj - nObjOffset; k++)
                {
                    lexlse.ObjectiveSensitivity(k, parameters.tol_wrong_sign_lambda, parameters.tol_correct_sign_lambda, ctr_wrong_sign);
                    if (!ctr_wrong_sign.empty())
                    {
                        found = true;
                        break;
                    }
                }
                if (found)
                {
                    for (size_t k = 0; k < ctr_wrong_sign.size(); k++)
                    {
                        ctr_wrong_sign[k].increment_obj_index(nObjOffset);
                        const int o = ctr_wrong_sign[k].get_obj_index();
                        ctr_wrong_sign[k].set_ctr_index(objectives[o].getActiveCtrIndex(ctr_wrong_sign[k].get_ctr_index()));
                    }
                    const Index k   = findFirstCtrWrongSign(ctr_wrong_sign);
                    ObjIndex2Remove = static_cast<Index>(WS[k].get_obj_index());
                    CtrIndex2Remove = objectives[ObjIndex2Remove].getCtrIndex(static_cast<Index>(WS[k].get_ctr_index()));
                }
                return found;
            }

            /// lexlsi.h:1115-1139: stop at the FIRST objective that reports a wrong-sign multiplier
            bool findActiveCtr2Remove_largest(Index &ObjIndex2Remove, Index &CtrIndex2Remove, RealScalar &lambda_wrong_sign)
            {
                bool found              = false;
                int ObjIndex2Remove_int = 0;
                for (Index k = 0; k < nObj - nObjOffset; k++)
                {
                    found = lexlse.ObjectiveSensitivity(k, CtrIndex2Remove, ObjIndex2Remove_int, parameters.tol_wrong_sign_lambda,
                                                        parameters.tol_correct_sign_lambda, lambda_wrong_sign);
                    if (found || sens_scans_all) break; // (sens_scans_all: the call above went through the remaining levels itself)
                }
                ObjIndex2Remove = static_cast<Index>(ObjIndex2Remove_int + static_cast<int>(nObjOffset));
                return found;
            }

            Index nVar;
            Index nObj;
            Index nObjOffset;
            Index nIterations;
            Index nActivations;
            Index nDeactivations;
            Index nFactorizations;
            Index lexlse_rank;
            RealScalar step_length;
            bool x_guess_is_specified;
            TerminationStatus status;
            dVectorType x;
            dVectorType dx;
            std::vector<Index> nActive;
            LSE lexlse;
            std::vector<Objective> objectives;
            ParametersLexLSI parameters;
            std::vector<WorkingSetLogEntry> working_set_log;
            CyclingHandler cycling_handler;
            std::vector<ConstraintInfo> WS;
        };
    } // namespace internal
} // namespace LexLS
