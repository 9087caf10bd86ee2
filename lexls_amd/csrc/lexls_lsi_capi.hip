// C ABI for inequality problems: the host-side active-set driver (include/lexls/lexlsi.h) instantiated over
// the HIP-backed equality solver (include/lexls/lexlse.h).  The equality solves happen inside the lexls_lse_* calls the driver
// issues; lock-step batches (lsi_batch.h) additionally run the step of an iteration (A*dx, ratio test, state update — SURVEY 8(f) item 1)
// and whole resident iterations in the kernels of lexls_lsi_device.h, on the constraint data that is resident anyway.  Here: the entry points only.
#include "lsi_batch.h"

namespace
{
    /// p[0..9): see lexls_lsi_solve; p[9..12) (only read when nparams >= 12): regularization_type, variable_regularization_factor,
    /// max_number_of_CG_iterations (typedefs.h:185-187); p[12..17) (only read when nparams == 17): modify_x_guess_enabled, modify_type_active_enabled,
    /// modify_type_inactive_enabled, set_min_init_ctr_violation, use_phase1_v0 (typedefs.h:213-217), 0 / 1 each
    ParametersLexLSI unpack(const double *p, uint32_t nparams = 9)
    {
        ParametersLexLSI par;
        if (p)
        {
            par.max_number_of_factorizations = static_cast<Index>(p[0]);
            par.tol_linear_dependence        = p[1];
            par.tol_wrong_sign_lambda        = p[2];
            par.tol_correct_sign_lambda      = p[3];
            par.tol_feasibility              = p[4];
            par.cycling_handling_enabled     = p[5] != 0;
            par.cycling_max_counter          = static_cast<Index>(p[6]);
            par.cycling_relax_step           = p[7];
            par.deactivate_first_wrong_sign  = p[8] != 0;
            if (nparams >= 12)
            {
                par.regularization_type            = static_cast<RegularizationType>(static_cast<int>(p[9]));
                par.variable_regularization_factor = p[10];
                par.max_number_of_CG_iterations    = static_cast<Index>(p[11]);
            }
            if (nparams >= 17) // the hot-start options, 0 / 1 each, in the order of typedefs.h:213-217
            {
                par.modify_x_guess_enabled       = p[12] != 0;
                par.modify_type_active_enabled   = p[13] != 0;
                par.modify_type_inactive_enabled = p[14] != 0;
                par.set_min_init_ctr_violation   = p[15] != 0;
                par.use_phase1_v0                = p[16] != 0;
            }
        }
        return par;
    }

    /// use_phase1_v0 without x0 at the entries whose phase 1 is device work: the reference's own complaint (lexlsi.h:882), before any device work — nothing
    /// is launched, the outputs stay as they are
    int refuse_phase1_v0(const ParametersLexLSI &par, bool has_x0)
    {
        if (!par.use_phase1_v0 || has_x0) return LEXLS_OK;
        lexls_internal_set_error("when use_phase1_v0 = true, x_guess has to be specified");
        return LEXLS_ERR_INVALID;
    }

    /// runs f and reports what it throws through lexls_last_error()
    template <class F>
    int guarded(F &&f)
    {
        try
        {
            return f();
        }
        catch (const std::exception &e)
        {
            lexls_internal_set_error(e.what());
            return LEXLS_ERR_INVALID;
        }
    }
} // namespace

extern "C"
{
    int lexls_lsi_batch_solve(int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types,
                              const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                              const double *h_params9, double *h_x, int32_t *h_info6, uint8_t *h_active, double *h_v, int32_t *h_rounds2)
    {
        return lexls_lsi_batch_solve_ex(device, batch, nVar, nObj, h_dims, h_types, h_data, h_var_index, h_active_guess, h_x0, NULL, h_params9, 9, h_x,
                                        h_info6, h_active, h_v, h_rounds2);
    }

    int lexls_lsi_batch_create(lexls_lsi_batch_t *out, int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types)
    {
        return guarded([&]() {
            if (!out || !h_dims || !h_types) throw Exception("lexls_lsi_batch_create: null argument");
            *out = new lexls_lsi_batch_s(device, batch, nVar, nObj, h_dims, h_types);
            return LEXLS_OK;
        });
    }

    int lexls_lsi_batch_stats(lexls_lsi_batch_t b, int32_t *h_stats4)
    {
        return guarded([&]() {
            if (!b || !h_stats4) throw Exception("lexls_lsi_batch_stats: null argument");
            b->refuse_pending("lexls_lsi_batch_stats");
            std::memcpy(h_stats4, b->last_stats, sizeof(b->last_stats));
            return LEXLS_OK;
        });
    }

    const char *lexls_lsi_batch_last_kernel(lexls_lsi_batch_t b) { return b ? b->last_kernel : ""; }

    int lexls_lsi_batch_destroy(lexls_lsi_batch_t b)
    {
        delete b;
        return LEXLS_OK;
    }

    int lexls_lsi_batch_run(lexls_lsi_batch_t b, const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                            const double *h_v0, const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6, uint8_t *h_active,
                            double *h_v, int32_t *h_rounds2)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_run: null handle");
            b->refuse_pending("lexls_lsi_batch_run");
            if (h_params && nparams != 9 && nparams != 12 && nparams != 17) throw Exception("lexls_lsi_batch_solve_ex: 9, 12 or 17 parameters expected"); // (the name its callers have always seen)
            const ParametersLexLSI par = unpack(h_params, nparams);
            if (const int refused = b->refuse_masked_run("lexls_lsi_batch_run")) return refused; // (nothing launched, the outputs as they are)
            if (const int refused = b->refuse_limited_run("lexls_lsi_batch_run")) return refused;
            if (const int refused = b->refuse_ragged_run("lexls_lsi_batch_run")) return refused;
            if (const int refused = b->refuse_run("lexls_lsi_batch_run", h_reg_factors, par, h_v0 != NULL)) return refused;
            b->run(h_data, h_var_index, h_active_guess, h_x0, h_v0, h_reg_factors, par, h_x, h_info6, h_active, h_v, h_rounds2);
            return static_cast<int>(LEXLS_OK);
        });
    }

    int lexls_lsi_batch_run_device(lexls_lsi_batch_t b, const double *d_data, const uint32_t *d_var_index, const uint8_t *d_active_guess, const double *d_x0,
                                   const double *h_reg_factors, const double *h_params, uint32_t nparams, double *d_x, int32_t *d_info6, uint8_t *d_active, double *d_v)
    {
        return lexls_lsi_batch_run_device_ex(b, d_data, d_var_index, d_active_guess, d_x0, NULL, h_reg_factors, h_params, nparams, d_x, d_info6, d_active, d_v, NULL, NULL);
    }

    int lexls_lsi_batch_run_device_ex(lexls_lsi_batch_t b, const double *d_data, const uint32_t *d_var_index, const uint8_t *d_active_guess, const double *d_x0,
                                      const double *d_v0, const double *h_reg_factors, const double *h_params, uint32_t nparams, double *d_x, int32_t *d_info6,
                                      uint8_t *d_active, double *d_v, double *d_lambda, uint32_t *d_cycling_counts)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_run_device: null handle");
            b->refuse_pending("lexls_lsi_batch_run_device");
            if (h_params && nparams != 9 && nparams != 12 && nparams != 17) throw Exception("lexls_lsi_batch_run_device: 9, 12 or 17 parameters expected");
            if (!d_data || !d_x) throw Exception("lexls_lsi_batch_run_device: null data / x");
            if (b->off && !d_var_index) throw Exception("lexls_lsi_batch_run_device: a simple-bounds objective needs variable indices");
            const ParametersLexLSI par = unpack(h_params, nparams);
            if (const int refused = b->refuse_run("lexls_lsi_batch_run_device", h_reg_factors, par, false)) return refused;
            if (const int refused = refuse_phase1_v0(par, d_x0 != NULL)) return refused;
            if (!b->would_be_resident(par)) // no detour over the host: nothing is launched, the outputs stay as they are
            {
                lexls_internal_set_error("lexls_lsi_batch_run_device: only runs that are resident on the device are served (not: LEXLS_LSI_RESIDENT=0, LEXLS_LSI_HOST_STAGING, "
                                         "regularization type 7, cycling handling of a regularized run, shapes without a register-resident kernel)");
                return static_cast<int>(LEXLS_ERR_UNSUPPORTED);
            }
            if (d_lambda && b->fin.lam_rc_after(par) != LEXLS_OK) // what lexls_lsi_batch_get_lambda would answer after this run: refused now, before any device work
            {
                lexls_internal_set_error("lexls_lsi_batch_run_device_ex: d_lambda is not served for a run with cycling handling enabled, a regularized run or more than 65535 "
                                         "constraints (lexls_lsi_batch_get_lambda is not available after such a run)");
                return static_cast<int>(LEXLS_ERR_UNSUPPORTED);
            }
            lexls_lsi_batch_s::DeviceArrays dev{d_data, d_var_index, d_active_guess, d_x0, d_x, d_info6, d_active, d_v};
            dev.v0 = d_x0 ? d_v0 : NULL; // v0 without x0 is disregarded (lexlsi.h:695-701)
            dev.cycling_counts = d_cycling_counts;
            b->run_device(dev, h_reg_factors, par);
            return d_lambda ? b->fin.get_lambda(NULL, d_lambda) : static_cast<int>(LEXLS_OK);
        });
    }

    int lexls_lsi_batch_enqueue_device(lexls_lsi_batch_t b, void *hip_stream, const double *d_data, const uint32_t *d_var_index, const uint8_t *d_active_guess,
                                       const double *d_x0, const double *d_v0, const double *h_reg_factors, const double *h_params, uint32_t nparams, double *d_x,
                                       int32_t *d_info6, uint8_t *d_active, double *d_v, double *d_lambda, uint32_t *d_cycling_counts, uint32_t *d_status)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_enqueue_device: null handle");
            if (h_params && nparams != 9 && nparams != 12 && nparams != 17) throw Exception("lexls_lsi_batch_enqueue_device: 9, 12 or 17 parameters expected");
            if (!d_data || !d_x) throw Exception("lexls_lsi_batch_enqueue_device: null data / x");
            if (b->off && !d_var_index) throw Exception("lexls_lsi_batch_enqueue_device: a simple-bounds objective needs variable indices");
            const ParametersLexLSI par = unpack(h_params, nparams);
            if (const int refused = b->refuse_run("lexls_lsi_batch_enqueue_device", h_reg_factors, par, false)) return refused;
            if (const int refused = refuse_phase1_v0(par, d_x0 != NULL)) return refused;
            if (!b->would_be_fused(par)) // no detour: nothing is enqueued, the outputs stay as they are
            {
                lexls_internal_set_error("lexls_lsi_batch_enqueue_device: only runs that lexls_lsi_batch_run_device serves and whose resident iterations are one persistent launch "
                                         "are served (not: LEXLS_LSI_NO_FUSED, shapes without a persistent instantiation or whose launch does not get its LDS, a batch "
                                         "split into several groups by LEXLS_LSI_GROUPS)");
                return static_cast<int>(LEXLS_ERR_UNSUPPORTED);
            }
            if (d_lambda && b->fin.lam_rc_after(par) != LEXLS_OK) // as lexls_lsi_batch_run_device_ex: refused before any device work
            {
                lexls_internal_set_error("lexls_lsi_batch_enqueue_device: d_lambda is not served for a run with cycling handling enabled, a regularized run or more than 65535 "
                                         "constraints (lexls_lsi_batch_get_lambda is not available after such a run)");
                return static_cast<int>(LEXLS_ERR_UNSUPPORTED);
            }
            lexls_lsi_batch_s::DeviceArrays dev{d_data, d_var_index, d_active_guess, d_x0, d_x, d_info6, d_active, d_v};
            dev.v0 = d_x0 ? d_v0 : NULL; // v0 without x0 is disregarded (lexlsi.h:695-701)
            dev.cycling_counts = d_cycling_counts;
            b->enqueue_device(static_cast<hipStream_t>(hip_stream), dev, h_reg_factors, par, d_status, d_lambda);
            return static_cast<int>(LEXLS_OK);
        });
    }

    int lexls_lsi_batch_finish(lexls_lsi_batch_t b, void *hip_stream)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_finish: null handle");
            return b->finish(static_cast<hipStream_t>(hip_stream));
        });
    }

    int lexls_lsi_batch_set_instance_regularization(lexls_lsi_batch_t b, const double *factors, int in_device_memory)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_set_instance_regularization: null handle");
            return b->set_instance_regularization(factors, in_device_memory);
        });
    }

    int lexls_lsi_batch_set_instance_mask(lexls_lsi_batch_t b, const uint8_t *d_mask)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_set_instance_mask: null handle");
            b->refuse_pending("lexls_lsi_batch_set_instance_mask"); // (an enqueued run reads the bytes it was given; a captured one goes on reading them)
            return b->set_instance_mask(d_mask);
        });
    }

    int lexls_lsi_batch_set_instance_max_factorizations(lexls_lsi_batch_t b, const int32_t *d_limits)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_set_instance_max_factorizations: null handle");
            b->refuse_pending("lexls_lsi_batch_set_instance_max_factorizations"); // (an enqueued run reads the array it was given; a captured one goes on reading it)
            return b->set_instance_max_factorizations(d_limits);
        });
    }

    int lexls_lsi_batch_set_instance_obj_dims(lexls_lsi_batch_t b, const uint32_t *d_dims)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_set_instance_obj_dims: null handle");
            b->refuse_pending("lexls_lsi_batch_set_instance_obj_dims"); // (an enqueued run reads the array it was given; a captured one goes on reading it)
            return b->set_instance_obj_dims(d_dims);
        });
    }

    int lexls_lsi_batch_get_lambda(lexls_lsi_batch_t b, double *h_lambda)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_get_lambda: null handle");
            b->refuse_pending("lexls_lsi_batch_get_lambda");
            return b->fin.get_lambda(h_lambda);
        });
    }

    /// both forms of the adjoint: every refusal comes before any device work and leaves the outputs alone
    static int lsi_batch_solve_adjoint(lexls_lsi_batch_t b, const double *g, double *grad_lb, double *grad_ub, bool on_device)
    {
        return guarded([&]() {
            const std::string who = on_device ? "lexls_lsi_batch_solve_adjoint_device" : "lexls_lsi_batch_solve_adjoint";
            if (!b) throw Exception(who + ": null handle");
            if (!g) throw Exception(who + ": null g");
            if (!grad_lb && !grad_ub) throw Exception(who + ": both outputs are null");
            b->refuse_pending(who.c_str());
            return b->fin.solve_adjoint(g, grad_lb, grad_ub, on_device);
        });
    }

    int lexls_lsi_batch_solve_adjoint(lexls_lsi_batch_t b, const double *h_g, double *h_grad_lb, double *h_grad_ub)
    {
        return lsi_batch_solve_adjoint(b, h_g, h_grad_lb, h_grad_ub, false);
    }

    int lexls_lsi_batch_solve_adjoint_device(lexls_lsi_batch_t b, const double *d_g, double *d_grad_lb, double *d_grad_ub)
    {
        return lsi_batch_solve_adjoint(b, d_g, d_grad_lb, d_grad_ub, true);
    }

    /// both forms of the multi-cotangent adjoint: the refusals of lsi_batch_solve_adjoint, and ncot == 0
    static int lsi_batch_solve_adjoint_multi(lexls_lsi_batch_t b, const double *G, uint32_t ncot, double *grad_lb, double *grad_ub, bool on_device)
    {
        return guarded([&]() {
            const std::string who = on_device ? "lexls_lsi_batch_solve_adjoint_multi_device" : "lexls_lsi_batch_solve_adjoint_multi";
            if (!b) throw Exception(who + ": null handle");
            if (!G) throw Exception(who + ": null G");
            if (ncot == 0) throw Exception(who + ": ncot == 0");
            if (!grad_lb && !grad_ub) throw Exception(who + ": both outputs are null");
            b->refuse_pending(who.c_str());
            return b->fin.solve_adjoint_multi(G, ncot, grad_lb, grad_ub, on_device);
        });
    }

    int lexls_lsi_batch_solve_adjoint_multi(lexls_lsi_batch_t b, const double *h_G, uint32_t ncot, double *h_grad_lb, double *h_grad_ub)
    {
        return lsi_batch_solve_adjoint_multi(b, h_G, ncot, h_grad_lb, h_grad_ub, false);
    }

    int lexls_lsi_batch_solve_adjoint_multi_device(lexls_lsi_batch_t b, const double *d_G, uint32_t ncot, double *d_grad_lb, double *d_grad_ub)
    {
        return lsi_batch_solve_adjoint_multi(b, d_G, ncot, d_grad_lb, d_grad_ub, true);
    }

    /// both forms of the matrix gradient: the refusals of lsi_batch_solve_adjoint, with grad_data the output that may not be null
    static int lsi_batch_solve_adjoint_matrix(lexls_lsi_batch_t b, const double *g, double *grad_data, uint8_t *differentiable, bool on_device)
    {
        return guarded([&]() {
            const std::string who = on_device ? "lexls_lsi_batch_solve_adjoint_matrix_device" : "lexls_lsi_batch_solve_adjoint_matrix";
            if (!b) throw Exception(who + ": null handle");
            if (!g) throw Exception(who + ": null g");
            if (!grad_data) throw Exception(who + ": null grad_data");
            b->refuse_pending(who.c_str());
            return b->fin.solve_adjoint_matrix(g, grad_data, differentiable, on_device);
        });
    }

    int lexls_lsi_batch_solve_adjoint_matrix(lexls_lsi_batch_t b, const double *h_g, double *h_grad_data, uint8_t *h_differentiable)
    {
        return lsi_batch_solve_adjoint_matrix(b, h_g, h_grad_data, h_differentiable, false);
    }

    int lexls_lsi_batch_solve_adjoint_matrix_device(lexls_lsi_batch_t b, const double *d_g, double *d_grad_data, uint8_t *d_differentiable)
    {
        return lsi_batch_solve_adjoint_matrix(b, d_g, d_grad_data, d_differentiable, true);
    }

    /// both forms of the forward-mode tangent: the refusals of lsi_batch_solve_adjoint_matrix, plus ntan == 0 and a null dx
    static int lsi_batch_solve_tangent(lexls_lsi_batch_t b, const double *ddata, uint32_t ntan, double *dx, uint8_t *differentiable, bool on_device)
    {
        return guarded([&]() {
            const std::string who = on_device ? "lexls_lsi_batch_solve_tangent_device" : "lexls_lsi_batch_solve_tangent";
            if (!b) throw Exception(who + ": null handle");
            if (!ddata) throw Exception(who + ": null ddata");
            if (!dx) throw Exception(who + ": null dx");
            if (ntan == 0) throw Exception(who + ": ntan == 0");
            b->refuse_pending(who.c_str());
            return b->fin.solve_tangent(ddata, ntan, dx, differentiable, on_device);
        });
    }

    int lexls_lsi_batch_solve_tangent(lexls_lsi_batch_t b, const double *h_ddata, uint32_t ntan, double *h_dx, uint8_t *h_differentiable)
    {
        return lsi_batch_solve_tangent(b, h_ddata, ntan, h_dx, h_differentiable, false);
    }

    int lexls_lsi_batch_solve_tangent_device(lexls_lsi_batch_t b, const double *d_ddata, uint32_t ntan, double *d_dx, uint8_t *d_differentiable)
    {
        return lsi_batch_solve_tangent(b, d_ddata, ntan, d_dx, d_differentiable, true);
    }

    /// both forms of the re-solve on new bounds: the refusals of lsi_batch_solve_tangent, plus nrhs > 65535 and null bounds
    /// (with_cost: lexls_lsi_batch_solve_bounds_cost(_device) — cost is the output that must be there, x may be NULL)
    static int lsi_batch_solve_bounds(lexls_lsi_batch_t b, const double *lb, const double *ub, uint32_t nrhs, double *x, double *violation, uint8_t *valid, bool on_device,
                                      bool with_cost = false, double *cost = NULL)
    {
        return guarded([&]() {
            const std::string who = std::string("lexls_lsi_batch_solve_bounds") + (with_cost ? "_cost" : "") + (on_device ? "_device" : "");
            if (!b) throw Exception(who + ": null handle");
            if (!lb || !ub) throw Exception(who + ": null lb / ub");
            if (!with_cost && !x) throw Exception(who + ": null x");
            if (with_cost && !cost) throw Exception(who + ": null cost");
            if (nrhs == 0) throw Exception(who + ": nrhs == 0");
            if (nrhs > 65535u) throw Exception(who + ": more than 65535 bound sets per instance");
            b->refuse_pending(who.c_str());
            return b->fin.solve_bounds(lb, ub, nrhs, x, violation, valid, on_device, with_cost, cost);
        });
    }

    int lexls_lsi_batch_solve_bounds(lexls_lsi_batch_t b, const double *h_lb, const double *h_ub, uint32_t nrhs, double *h_x, double *h_violation, uint8_t *h_valid)
    {
        return lsi_batch_solve_bounds(b, h_lb, h_ub, nrhs, h_x, h_violation, h_valid, false);
    }

    int lexls_lsi_batch_solve_bounds_device(lexls_lsi_batch_t b, const double *d_lb, const double *d_ub, uint32_t nrhs, double *d_x, double *d_violation, uint8_t *d_valid)
    {
        return lsi_batch_solve_bounds(b, d_lb, d_ub, nrhs, d_x, d_violation, d_valid, true);
    }

    int lexls_lsi_batch_solve_bounds_cost(lexls_lsi_batch_t b, const double *h_lb, const double *h_ub, uint32_t nrhs, double *h_x, double *h_violation, double *h_cost,
                                          uint8_t *h_valid)
    {
        return lsi_batch_solve_bounds(b, h_lb, h_ub, nrhs, h_x, h_violation, h_valid, false, true, h_cost);
    }

    int lexls_lsi_batch_solve_bounds_cost_device(lexls_lsi_batch_t b, const double *d_lb, const double *d_ub, uint32_t nrhs, double *d_x, double *d_violation, double *d_cost,
                                                 uint8_t *d_valid)
    {
        return lsi_batch_solve_bounds(b, d_lb, d_ub, nrhs, d_x, d_violation, d_valid, true, true, d_cost);
    }

    const char *lexls_lsi_batch_last_consumer_kernel(lexls_lsi_batch_t b) { return b ? b->fin.bounds_kernel : ""; }

    int lexls_lsi_batch_final_factorizations(lexls_lsi_batch_t b, uint32_t *h_count)
    {
        return guarded([&]() {
            if (!b || !h_count) throw Exception("lexls_lsi_batch_final_factorizations: null argument");
            *h_count = b->fin.final_formations;
            return LEXLS_OK;
        });
    }

    int lexls_lsi_batch_get_cycling_counters(lexls_lsi_batch_t b, uint32_t *h_counts)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_get_cycling_counters: null handle");
            b->refuse_pending("lexls_lsi_batch_get_cycling_counters");
            return b->get_cycling_counters(h_counts);
        });
    }

    int lexls_lsi_batch_set_working_set_log(lexls_lsi_batch_t b, uint32_t max_entries)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_set_working_set_log: null handle");
            return b->set_working_set_log(max_entries);
        });
    }

    int lexls_lsi_batch_set_adjoint_regularized(lexls_lsi_batch_t b, int on)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_set_adjoint_regularized: null handle");
            b->refuse_pending("lexls_lsi_batch_set_adjoint_regularized");
            b->fin.adj_regularized = on != 0; // (the rule of the last run stands: the next run is the first one it applies to)
            return static_cast<int>(LEXLS_OK);
        });
    }

    int lexls_lsi_batch_set_adjoint_regularized_multi(lexls_lsi_batch_t b, int on)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_set_adjoint_regularized_multi: null handle");
            b->refuse_pending("lexls_lsi_batch_set_adjoint_regularized_multi");
            b->fin.adj_regularized_multi = on != 0; // (the rule of the last run stands: the next run is the first one it applies to)
            return static_cast<int>(LEXLS_OK);
        });
    }

    int lexls_lsi_batch_get_working_set_log(lexls_lsi_batch_t b, int32_t *h_log, double *h_alpha, uint32_t *h_counts)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_get_working_set_log: null handle");
            b->refuse_pending("lexls_lsi_batch_get_working_set_log");
            return b->get_working_set_log(h_log, h_alpha, h_counts);
        });
    }

    int lexls_lsi_batch_working_set_log_device(lexls_lsi_batch_t b, void **d_log, void **d_alpha, void **d_counts)
    {
        return guarded([&]() {
            if (!b) throw Exception("lexls_lsi_batch_working_set_log_device: null handle");
            if (!b->wlog) throw Exception("lexls_lsi_batch_working_set_log_device: the working-set log is off (lexls_lsi_batch_set_working_set_log)");
            if (d_log) *d_log = b->wlog->d_log;
            if (d_alpha) *d_alpha = b->wlog->d_alpha;
            if (d_counts) *d_counts = b->wlog->d_count;
            return static_cast<int>(LEXLS_OK);
        });
    }

    int lexls_lsi_batch_solve_ex2(int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types,
                                  const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                                  const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6,
                                  uint8_t *h_active, double *h_v, int32_t *h_rounds2, double *h_lambda)
    {
        lexls_lsi_batch_t b = NULL;
        int rc              = lexls_lsi_batch_create(&b, device, batch, nVar, nObj, h_dims, h_types);
        if (rc == LEXLS_OK) rc = lexls_lsi_batch_run(b, h_data, h_var_index, h_active_guess, h_x0, NULL, h_reg_factors, h_params, nparams, h_x, h_info6, h_active, h_v, h_rounds2);
        if (rc == LEXLS_OK && h_lambda) rc = lexls_lsi_batch_get_lambda(b, h_lambda);
        lexls_lsi_batch_destroy(b);
        return rc;
    }

    int lexls_lsi_batch_solve_ex(int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types,
                                 const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                                 const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6,
                                 uint8_t *h_active, double *h_v, int32_t *h_rounds2)
    {
        return lexls_lsi_batch_solve_ex2(device, batch, nVar, nObj, h_dims, h_types, h_data, h_var_index, h_active_guess, h_x0, h_reg_factors, h_params, nparams, h_x, h_info6,
                                         h_active, h_v, h_rounds2, NULL);
    }

    int lexls_lsi_solve(int device, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types, const double *h_data,
                        const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0, const double *h_params9, double *h_x,
                        int32_t *h_info6, uint8_t *h_active, double *h_v)
    {
        return lexls_lsi_solve_ex(device, nVar, nObj, h_dims, h_types, h_data, h_var_index, h_active_guess, h_x0, NULL, NULL, h_params9, 9, h_x, h_info6, h_active, h_v);
    }

    int lexls_lsi_solve_ex(int device, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types, const double *h_data,
                           const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0, const double *h_v0,
                           const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6, uint8_t *h_active,
                           double *h_v)
    {
        return guarded([&]() {
            if (h_params && nparams != 9 && nparams != 12 && nparams != 17) throw Exception("lexls_lsi_solve_ex: 9, 12 or 17 parameters expected");
            internal::LexLSI lsi;
            solve_one(lsi, device, {nVar, nObj, h_dims, h_types, h_data, h_var_index, h_active_guess, h_x0, h_v0, h_reg_factors}, unpack(h_params, nparams), h_x, h_info6, h_active, h_v);
            return LEXLS_OK;
        });
    }

    int lexls_lsi_solve_debug(int device, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types, const double *h_data,
                              const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0, const double *h_v0,
                              const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6, uint8_t *h_active,
                              double *h_v, const lexls_lsi_debug *debug)
    {
        return guarded([&]() {
            if (h_params && nparams != 9 && nparams != 12 && nparams != 17) throw Exception("lexls_lsi_solve_debug: 9, 12 or 17 parameters expected");
            if (!debug) throw Exception("lexls_lsi_solve_debug: debug is NULL (use lexls_lsi_solve_ex)");
            const runner::LsiProblem p = {nVar, nObj, h_dims, h_types, h_data, h_var_index, h_active_guess, h_x0, h_v0, h_reg_factors};
            ParametersLexLSI par        = unpack(h_params, nparams);
            par.log_working_set_enabled = true;
            internal::LexLSI lsi;
            solve_one(lsi, device, p, par, h_x, h_info6, h_active, h_v);
            const runner::LsiDebug d = {debug->lambda, debug->lexqr, debug->data, debug->x_star, debug->active_ctr, debug->log, debug->log_alpha, debug->max_log,
                                        debug->x_mu, debug->x_mu_rhs, debug->residual_mu, debug->counts};
            runner::collect_debug(lsi, p, par, d);
            return LEXLS_OK;
        });
    }

    int lexls_lsi_solve_dat(int device, const char *path, int one_based, int use_active_guess, int use_x_guess, double *h_x, int32_t *h_info6,
                            double *h_solution)
    {
        return guarded([&]() {
            tools::Hierarchy h;
            tools::HierarchyFileProcessor().import(path, h);
            runner::FlatHierarchy f;
            runner::flatten(h, one_based != 0, use_active_guess != 0, use_x_guess != 0, f);
            internal::LexLSI lsi;
            solve_one(lsi, device, f.problem, ParametersLexLSI(), h_x, h_info6, NULL, NULL);
            if (h_solution)
                for (Index i = 0; i < h.solution.size(); i++) h_solution[i] = h.solution(i);
            return LEXLS_OK;
        });
    }
}
