// The calls of the C ABI (include/lexls_hip.h) that work on a kept LexLSE factor beyond the solves of lexls_capi.hip, which includes this file once:
// lexls_lse_solve_adjoint, _adjoint_multi, _adjoint_matrix, _tangent, _rhs and lexls_lse_residual_rhs.  Every family has a device form (checks, work buffers, launch: enqueue
// only), a host form (the handle's HostResults of the family: make room, upload, the device form's function, stamp) and a getter (HostResults::fetch).
#pragma once

namespace
{
    int HostResults::fetch(lexls_lse_s *h, const char *getter, const char *call, std::initializer_list<Copy> copies) const
    {
        const std::string who = getter;
        if (!valid) return fail(LEXLS_ERR_INVALID, who + ": call " + call + " first");
        if (!h->factor_valid || epoch != h->factor_epoch) return fail(LEXLS_ERR_INVALID, who + ": the problem or its factorization changed since " + call + " (call it again)");
        HIP_TRY(hipSetDevice(h->device));
        for (const Copy &c : copies)
            if (c.dst) HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }

    /// a kept factor — unregularized, or regularized with one of the types whose damped solve is an affine map of the kept factor, the factors
    /// constant.  not_served: what a call that serves no damped factor, or not while its switch is off, says of one (else NULL)
    int need_affine_factor(lexls_lse_t h, const char *who, const char *not_served = nullptr)
    {
        if (int rc = need_factor(h, who)) return rc;
        if (h->reg_type == 0) return LEXLS_OK;
        if (not_served) return fail(LEXLS_ERR_UNSUPPORTED, std::string(who) + not_served);
        if (!adjoint_reg_serves(h->reg_type))
            return fail(LEXLS_ERR_UNSUPPORTED, std::string(who) + ": regularization_type " + std::to_string(h->reg_type) +
                                                   " is not an affine map of the right-hand side (the CG types 2 and 6 iterate from x = 0, type 7 is experimental); served: 1, 3, 4, 5, 8, 9");
        if (h->reg_variable != 0.0)
            return fail(LEXLS_ERR_UNSUPPORTED, std::string(who) + ": variable_regularization_factor != 0 under regularization_type " + std::to_string(h->reg_type) +
                                                   " (the factor depends on the right-hand side: x is not an affine map of it)");
        return LEXLS_OK;
    }

    /// what every form of the adjoint checks before any device work: g, and need_affine_factor — a damped factor is served by AdjointCall::single
    /// (lexls_lse_solve_adjoint and its device form) once lexls_lse_set_adjoint_regularized switched it on, by AdjointCall::multi (the multi-cotangent
    /// calls) once lexls_lse_set_adjoint_regularized_multi did, by no other call
    enum class AdjointCall { other, single, multi };
    int need_adjoint_factor(lexls_lse_t h, const char *who, const void *g, AdjointCall call = AdjointCall::other)
    {
        CHECK_HANDLE(h);
        if (!g) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null g");
        const char *not_served = nullptr;
        if (call == AdjointCall::other)
            not_served = ": the factorization ran with regularization_type != 0 (lexls_lse_solve_adjoint, the single-cotangent call, serves "
                         "regularization types 1, 3, 4, 5, 8 and 9; this call serves none)";
        else if (call == AdjointCall::multi && !h->adj_regularized_multi)
            not_served = ": the factorization ran with regularization_type != 0 and the many-cotangent adjoint of damped solves is not "
                         "switched on for this handle (lexls_lse_set_adjoint_regularized_multi; it serves regularization types 1, 3, 4, 5, 8 "
                         "and 9, as lexls_lse_solve_adjoint, the single-cotangent call, does under lexls_lse_set_adjoint_regularized)";
        else if (call == AdjointCall::single && !h->adj_regularized)
            not_served = ": the factorization ran with regularization_type != 0 and the adjoint of damped solves is not switched on "
                         "for this handle (lexls_lse_set_adjoint_regularized; it serves regularization types 1, 3, 4, 5, 8 and 9)";
        return need_affine_factor(h, who, not_served);
    }

    /// the host form of a call, ahead of the function its device form runs too (whose checks it has run before it touches h or h_in): the call's
    /// input into the handle's buffer
    int upload_input(lexls_lse_t h, const DeviceBuffer &d_in, const double *h_in, size_t bytes)
    {
        HIP_TRY(hipMemcpyAsync(d_in.ptr, h_in, bytes, hipMemcpyHostToDevice, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream)); // h_in may be reused by the caller
        return LEXLS_OK;
    }

    /// every form of lexls_lse_solve_adjoint on device memory: the checks, the work buffer, the launch
    int run_solve_adjoint(lexls_lse_t h, const char *who, const double *d_g, double *d_grad_rhs, double *d_grad_fixed)
    {
        if (int rc = need_adjoint_factor(h, who, d_g, AdjointCall::single)) return rc;
        if (!d_grad_rhs) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null d_grad_rhs");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->adj_work.reserve(adjoint_reg_work_bytes(h->args())));
        HIP_TRY(launch_solve_adjoint(h->args(), d_g, d_grad_rhs, d_grad_fixed, h->stream, &h->last_consumer, h->adj_work.as<double>()));
        return LEXLS_OK;
    }

    /// what both multi-cotangent forms check before any device work
    int need_adjoint_multi(lexls_lse_t h, const char *who, const void *G, uint32_t ncot)
    {
        CHECK_HANDLE(h);
        if (!G) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null G");
        if (ncot == 0) return fail(LEXLS_ERR_INVALID, std::string(who) + ": ncot == 0");
        return need_adjoint_factor(h, who, G, AdjointCall::multi);
    }
    /// every form of lexls_lse_solve_adjoint_multi on device memory: the checks, the work buffers, the launch
    int run_solve_adjoint_multi(lexls_lse_t h, const char *who, const double *d_G, uint32_t ncot, double *d_grad_rhs, double *d_grad_fixed)
    {
        if (int rc = need_adjoint_multi(h, who, d_G, ncot)) return rc;
        if (!d_grad_rhs) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null d_grad_rhs");
        HIP_TRY(hipSetDevice(h->device));
        const size_t bytes = adjoint_multi_work_bytes(h->args());
        HIP_TRY(h->adjm_work.reserve(bytes));
        if (bytes) HIP_TRY(h->adj_work.reserve(adjoint_reg_work_bytes(h->args()))); // (the per-cotangent form runs lexls_lse_solve_adjoint's launch)
        HIP_TRY(h->adjrm_work.reserve(adjoint_reg_multi_work_bytes(h->args(), ncot))); // the matrices of the hbm form, for the most tiles so far
        HIP_TRY(launch_solve_adjoint_multi(h->args(), d_G, ncot, d_grad_rhs, d_grad_fixed, h->adjm_work.as<double>(), h->stream, &h->last_consumer, h->adj_work.as<double>(),
                                           h->adjrm_work.as<double>()));
        return LEXLS_OK;
    }

    /// what every form of the matrix gradient checks before any device work: a kept, unregularized factor and the x that belongs to it
    int need_adjoint_matrix(lexls_lse_t h, const char *who, const void *g)
    {
        if (int rc = need_adjoint_factor(h, who, g)) return rc;
        if (h->x_epoch != h->factor_epoch)
            return fail(LEXLS_ERR_INVALID, std::string(who) + ": no x belongs to the current factor (lexls_lse_factorize_solve(keep_factor = 1), or lexls_lse_factorize + lexls_lse_solve)");
        return LEXLS_OK;
    }
    /// every form of lexls_lse_solve_adjoint_matrix on device memory: the checks, the work buffer, the launch (d_grad_fixed: lexls_internal_solve_adjoint_matrix's)
    int run_solve_adjoint_matrix(lexls_lse_t h, const char *who, const double *d_g, double *d_grad_lod, uint8_t *d_differentiable, double *d_grad_fixed)
    {
        if (int rc = need_adjoint_matrix(h, who, d_g)) return rc;
        if (!d_grad_lod) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null d_grad_lod");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->adjA_work.reserve(adjoint_matrix_work_bytes(h->args())));
        HIP_TRY(launch_solve_adjoint_matrix(h->args(), d_g, d_grad_lod, d_differentiable, h->adjA_work.ptr, h->max_level_dim, h->stream, &h->last_consumer, d_grad_fixed));
        return LEXLS_OK;
    }

    /// what every form of lexls_lse_solve_tangent checks before any device work: lexls_lse_solve_adjoint_matrix's preconditions, ntan
    int need_tangent(lexls_lse_t h, const char *who, const void *dlod, uint32_t ntan)
    {
        CHECK_HANDLE(h);
        if (!dlod) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null dlod");
        if (ntan == 0) return fail(LEXLS_ERR_INVALID, std::string(who) + ": ntan == 0");
        if (ntan > 65535u) return fail(LEXLS_ERR_INVALID, std::string(who) + ": ntan > 65535 (split the directions over several calls)");
        return need_adjoint_matrix(h, who, dlod);
    }
    /// every form of lexls_lse_solve_tangent on device memory: the checks, the work buffers, the launch
    int run_solve_tangent(lexls_lse_t h, const char *who, const double *d_dlod, const double *d_dfixed, uint32_t ntan, double *d_dx, uint8_t *d_differentiable)
    {
        if (int rc = need_tangent(h, who, d_dlod, ntan)) return rc;
        if (!d_dx) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null d_dx");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->tan_work.reserve(tangent_work_bytes(h->args(), ntan)));
        HIP_TRY(h->adjm_work.reserve(ntan > 1 ? adjoint_multi_work_bytes(h->args()) : 0)); // (M^T w of several tangents: the per-cotangent form's buffers)
        HIP_TRY(launch_solve_tangent(h->args(), d_dlod, d_dfixed, ntan, d_dx, d_differentiable, h->tan_work.ptr, h->adjm_work.as<double>(), h->max_level_dim, h->stream,
                                     &h->last_consumer));
        return LEXLS_OK;
    }

    /// what every form of lexls_lse_solve_rhs checks before any device work: the arguments, need_affine_factor (behind no switch: a new entry)
    int need_solve_rhs(lexls_lse_t h, const char *who, const void *rhs, uint32_t nrhs)
    {
        CHECK_HANDLE(h);
        if (!rhs) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null rhs");
        if (nrhs == 0) return fail(LEXLS_ERR_INVALID, std::string(who) + ": nrhs == 0");
        if (nrhs > 65535u) return fail(LEXLS_ERR_INVALID, std::string(who) + ": nrhs > 65535 (split the right-hand sides over several calls)");
        return need_affine_factor(h, who);
    }
    /// every form of lexls_lse_solve_rhs on device memory: the checks, the work buffer, the launch
    int run_solve_rhs(lexls_lse_t h, const char *who, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x)
    {
        if (int rc = need_solve_rhs(h, who, d_rhs, nrhs)) return rc;
        if (!d_x) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null d_x");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->srhs_work.reserve(solve_rhs_work_bytes(h->args(), nrhs)));
        HIP_TRY(launch_solve_rhs(h->args(), d_rhs, d_fixed, nrhs, d_x, h->srhs_work.ptr, h->stream, &h->last_consumer));
        return LEXLS_OK;
    }

    /// what every form of lexls_lse_residual_rhs checks before any device work: lexls_lse_solve_rhs's, and an UNDAMPED factor
    int need_residual_rhs(lexls_lse_t h, const char *who, const void *rhs, bool any_output, uint32_t nrhs)
    {
        CHECK_HANDLE(h);
        if (!rhs) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null rhs");
        if (!any_output) return fail(LEXLS_ERR_INVALID, std::string(who) + ": every output is null");
        if (nrhs == 0) return fail(LEXLS_ERR_INVALID, std::string(who) + ": nrhs == 0");
        if (nrhs > 65535u) return fail(LEXLS_ERR_INVALID, std::string(who) + ": nrhs > 65535 (split the right-hand sides over several calls)");
        return need_affine_factor(h, who, ": the factorization ran with regularization_type != 0 (v is the residual of the undamped basic solution; "
                                          "lexls_lse_solve_rhs serves damped factors, this call serves none)");
    }
    /// every form of lexls_lse_residual_rhs on device memory: the checks, the work buffer (lexls_lse_solve_rhs's: scratch of either call), the launch
    int run_residual_rhs(lexls_lse_t h, const char *who, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x, double *d_v, double *d_cost)
    {
        if (int rc = need_residual_rhs(h, who, d_rhs, d_x || d_v || d_cost, nrhs)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->srhs_work.reserve(residual_rhs_work_bytes(h->args(), nrhs)));
        HIP_TRY(launch_residual_rhs(h->args(), d_rhs, d_fixed, nrhs, d_x, d_v, d_cost, h->srhs_work.ptr, h->stream, &h->last_consumer));
        return LEXLS_OK;
    }
} // namespace

extern "C"
{
    int lexls_lse_set_adjoint_regularized(lexls_lse_t h, int on)
    {
        CHECK_HANDLE(h);
        h->adj_regularized = on != 0;
        return LEXLS_OK;
    }

    int lexls_lse_set_adjoint_regularized_multi(lexls_lse_t h, int on)
    {
        CHECK_HANDLE(h);
        h->adj_regularized_multi = on != 0;
        return LEXLS_OK;
    }

    int lexls_lse_solve_adjoint(lexls_lse_t h, const double *h_g)
    {
        const char *who = "lexls_lse_solve_adjoint";
        if (int rc = need_adjoint_factor(h, who, h_g, AdjointCall::single)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const size_t B = h->batch, n = h->nVar, cap = h->cap;
        HostResults &r = h->adj;
        HIP_TRY(r.make_room(1, {8 * B * n, 8 * B * cap, 8 * B * n}));
        if (int rc = upload_input(h, r.buf[0], h_g, 8 * B * n)) return rc;
        if (int rc = run_solve_adjoint(h, who, r.at<double>(0), r.at<double>(1), r.at<double>(2))) return rc;
        r.stamp(1, h->factor_epoch);
        return LEXLS_OK;
    }

    int lexls_lse_solve_adjoint_device(lexls_lse_t h, const double *d_g, double *d_grad_rhs, double *d_grad_fixed)
    {
        return run_solve_adjoint(h, "lexls_lse_solve_adjoint_device", d_g, d_grad_rhs, d_grad_fixed);
    }

    int lexls_lse_get_adjoint(lexls_lse_t h, double *h_grad_rhs, double *h_grad_fixed)
    {
        CHECK_HANDLE(h);
        const HostResults &r = h->adj;
        return r.fetch(h, "lexls_lse_get_adjoint", "lexls_lse_solve_adjoint",
                       {{h_grad_rhs, r.buf[1].ptr, 8 * (size_t)h->batch * h->cap}, {h_grad_fixed, r.buf[2].ptr, 8 * (size_t)h->batch * h->nVar}});
    }

    int lexls_lse_solve_adjoint_multi(lexls_lse_t h, const double *h_G, uint32_t ncot)
    {
        const char *who = "lexls_lse_solve_adjoint_multi";
        if (int rc = need_adjoint_multi(h, who, h_G, ncot)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const size_t B = h->batch, n = h->nVar, cap = h->cap;
        HostResults &r = h->adjm;
        HIP_TRY(r.make_room(ncot, {8 * B * ncot * n, 8 * B * ncot * cap, 8 * B * ncot * n}));
        if (int rc = upload_input(h, r.buf[0], h_G, 8 * B * ncot * n)) return rc;
        if (int rc = run_solve_adjoint_multi(h, who, r.at<double>(0), ncot, r.at<double>(1), r.at<double>(2))) return rc;
        r.stamp(ncot, h->factor_epoch);
        return LEXLS_OK;
    }

    int lexls_lse_solve_adjoint_multi_device(lexls_lse_t h, const double *d_G, uint32_t ncot, double *d_grad_rhs, double *d_grad_fixed)
    {
        return run_solve_adjoint_multi(h, "lexls_lse_solve_adjoint_multi_device", d_G, ncot, d_grad_rhs, d_grad_fixed);
    }

    int lexls_lse_get_adjoint_multi(lexls_lse_t h, double *h_grad_rhs, double *h_grad_fixed)
    {
        CHECK_HANDLE(h);
        const HostResults &r = h->adjm;
        const size_t rows    = (size_t)h->batch * r.count;
        return r.fetch(h, "lexls_lse_get_adjoint_multi", "lexls_lse_solve_adjoint_multi",
                       {{h_grad_rhs, r.buf[1].ptr, 8 * rows * h->cap}, {h_grad_fixed, r.buf[2].ptr, 8 * rows * h->nVar}});
    }

    int lexls_lse_solve_adjoint_matrix(lexls_lse_t h, const double *h_g)
    {
        const char *who = "lexls_lse_solve_adjoint_matrix";
        if (int rc = need_adjoint_matrix(h, who, h_g)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const size_t B = h->batch, n = h->nVar;
        HostResults &r = h->adjA;
        HIP_TRY(r.make_room(1, {8 * B * n, 8 * B * h->problem_elems(), B}));
        if (int rc = upload_input(h, r.buf[0], h_g, 8 * B * n)) return rc;
        if (int rc = run_solve_adjoint_matrix(h, who, r.at<double>(0), r.at<double>(1), r.at<uint8_t>(2), nullptr)) return rc;
        r.stamp(1, h->factor_epoch);
        return LEXLS_OK;
    }

    int lexls_lse_solve_adjoint_matrix_device(lexls_lse_t h, const double *d_g, double *d_grad_lod, uint8_t *d_differentiable)
    {
        return run_solve_adjoint_matrix(h, "lexls_lse_solve_adjoint_matrix_device", d_g, d_grad_lod, d_differentiable, nullptr);
    }

    int lexls_internal_solve_adjoint_matrix(lexls_lse_t h, const double *d_g, double *d_grad_lod, double *d_grad_fixed, uint8_t *d_differentiable)
    {
        return run_solve_adjoint_matrix(h, "lexls_internal_solve_adjoint_matrix", d_g, d_grad_lod, d_differentiable, d_grad_fixed);
    }

    int lexls_lse_get_adjoint_matrix(lexls_lse_t h, double *h_grad_lod, uint8_t *h_differentiable)
    {
        CHECK_HANDLE(h);
        const HostResults &r = h->adjA;
        return r.fetch(h, "lexls_lse_get_adjoint_matrix", "lexls_lse_solve_adjoint_matrix",
                       {{h_grad_lod, r.buf[1].ptr, 8 * (size_t)h->batch * h->problem_elems()}, {h_differentiable, r.buf[2].ptr, (size_t)h->batch}});
    }

    int lexls_lse_solve_tangent(lexls_lse_t h, const double *h_dlod, const double *h_dfixed, uint32_t ntan)
    {
        const char *who = "lexls_lse_solve_tangent";
        if (int rc = need_tangent(h, who, h_dlod, ntan)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const size_t B = h->batch, n = h->nVar;
        HostResults &r = h->tan;
        HIP_TRY(r.make_room(ntan, {8 * B * ntan * h->problem_elems(), 8 * B * ntan * n, 8 * B * ntan * n}));
        HIP_TRY(h->tan_flag.reserve(B));
        if (h_dfixed) HIP_TRY(hipMemcpyAsync(r.buf[1].ptr, h_dfixed, 8 * B * ntan * n, hipMemcpyHostToDevice, h->stream));
        if (int rc = upload_input(h, r.buf[0], h_dlod, 8 * B * ntan * h->problem_elems())) return rc;
        if (int rc = run_solve_tangent(h, who, r.at<double>(0), h_dfixed ? r.at<double>(1) : nullptr, ntan, r.at<double>(2), h->tan_flag.as<uint8_t>())) return rc;
        r.stamp(ntan, h->factor_epoch);
        return LEXLS_OK;
    }

    int lexls_lse_solve_tangent_device(lexls_lse_t h, const double *d_dlod, const double *d_dfixed, uint32_t ntan, double *d_dx, uint8_t *d_differentiable)
    {
        return run_solve_tangent(h, "lexls_lse_solve_tangent_device", d_dlod, d_dfixed, ntan, d_dx, d_differentiable);
    }

    int lexls_lse_get_tangent(lexls_lse_t h, double *h_dx, uint8_t *h_differentiable)
    {
        CHECK_HANDLE(h);
        const HostResults &r = h->tan;
        return r.fetch(h, "lexls_lse_get_tangent", "lexls_lse_solve_tangent",
                       {{h_dx, r.buf[2].ptr, 8 * (size_t)h->batch * r.count * h->nVar}, {h_differentiable, h->tan_flag.ptr, (size_t)h->batch}});
    }

    int lexls_lse_solve_rhs(lexls_lse_t h, const double *h_rhs, const double *h_fixed, uint32_t nrhs)
    {
        const char *who = "lexls_lse_solve_rhs";
        if (int rc = need_solve_rhs(h, who, h_rhs, nrhs)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const size_t B = h->batch, n = h->nVar, cap = h->cap;
        HostResults &r = h->srhs;
        HIP_TRY(r.make_room(nrhs, {8 * B * nrhs * cap, 8 * B * nrhs * n, 8 * B * nrhs * n}));
        if (h_fixed) HIP_TRY(hipMemcpyAsync(r.buf[1].ptr, h_fixed, 8 * B * nrhs * n, hipMemcpyHostToDevice, h->stream));
        if (int rc = upload_input(h, r.buf[0], h_rhs, 8 * B * nrhs * cap)) return rc;
        if (int rc = run_solve_rhs(h, who, r.at<double>(0), h_fixed ? r.at<double>(1) : nullptr, nrhs, r.at<double>(2))) return rc;
        r.stamp(nrhs, h->factor_epoch);
        return LEXLS_OK;
    }

    int lexls_lse_solve_rhs_device(lexls_lse_t h, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x)
    {
        return run_solve_rhs(h, "lexls_lse_solve_rhs_device", d_rhs, d_fixed, nrhs, d_x);
    }

    int lexls_lse_get_solve_rhs(lexls_lse_t h, double *h_x)
    {
        CHECK_HANDLE(h);
        const HostResults &r = h->srhs;
        return r.fetch(h, "lexls_lse_get_solve_rhs", "lexls_lse_solve_rhs", {{h_x, r.buf[2].ptr, 8 * (size_t)h->batch * r.count * h->nVar}});
    }

    int lexls_lse_residual_rhs(lexls_lse_t h, const double *h_rhs, const double *h_fixed, uint32_t nrhs)
    {
        const char *who = "lexls_lse_residual_rhs";
        if (int rc = need_residual_rhs(h, who, h_rhs, true, nrhs)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const size_t B = h->batch, n = h->nVar, cap = h->cap, nObj = h->nObj;
        HostResults &r = h->rres;
        HIP_TRY(r.make_room(nrhs, {8 * B * nrhs * cap, 8 * B * nrhs * n, 8 * B * nrhs * (cap + nObj)}));
        if (h_fixed) HIP_TRY(hipMemcpyAsync(r.buf[1].ptr, h_fixed, 8 * B * nrhs * n, hipMemcpyHostToDevice, h->stream));
        if (int rc = upload_input(h, r.buf[0], h_rhs, 8 * B * nrhs * cap)) return rc;
        if (int rc = run_residual_rhs(h, who, r.at<double>(0), h_fixed ? r.at<double>(1) : nullptr, nrhs, nullptr, r.at<double>(2), r.at<double>(2) + B * nrhs * cap)) return rc;
        r.stamp(nrhs, h->factor_epoch);
        return LEXLS_OK;
    }

    int lexls_lse_residual_rhs_device(lexls_lse_t h, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x, double *d_v, double *d_cost)
    {
        return run_residual_rhs(h, "lexls_lse_residual_rhs_device", d_rhs, d_fixed, nrhs, d_x, d_v, d_cost);
    }

    int lexls_lse_get_residual_rhs(lexls_lse_t h, double *h_v, double *h_cost)
    {
        CHECK_HANDLE(h);
        if (!h_v && !h_cost) return fail(LEXLS_ERR_INVALID, "lexls_lse_get_residual_rhs: null h_v and h_cost");
        const HostResults &r = h->rres;
        const size_t rows    = (size_t)h->batch * r.count;
        return r.fetch(h, "lexls_lse_get_residual_rhs", "lexls_lse_residual_rhs",
                       {{h_v, r.buf[2].ptr, 8 * rows * h->cap}, {h_cost, r.at<double>(2) + rows * h->cap, 8 * rows * h->nObj}});
    }

    int lexls_internal_apply_solve_map(lexls_lse_t h, const double *d_rhs, double *d_out)
    {
        if (int rc = need_adjoint_factor(h, "lexls_internal_apply_solve_map", d_rhs)) return rc;
        if (!d_out) return fail(LEXLS_ERR_INVALID, "lexls_internal_apply_solve_map: null d_out");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(launch_apply_solve_map(h->args(), d_rhs, nullptr, d_out, h->stream));
        return LEXLS_OK;
    }
}
