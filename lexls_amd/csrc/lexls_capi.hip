// C ABI of liblexls_hip (include/lexls_hip.h): handle management, H2D/D2H plumbing and kernel
// dispatch.  There is deliberately NO CPU fallback: without a usable HIP device every entry point
// that needs one fails with LEXLS_ERR_NO_DEVICE / LEXLS_ERR_HIP.
#include "../../include/lexls_hip.h"
#include "lexls_internal.h"
#include "lexls_kernels.h"
#include "lexls_launch.h"
#include "lexls_regularize.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace lexls;

namespace
{
    thread_local std::string g_err;

    int fail(int code, const std::string &msg)
    {
        g_err = msg;
        return code;
    }

#define HIP_TRY(expr)                                                                                                   \
    do                                                                                                                  \
    {                                                                                                                   \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return fail(LEXLS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

#define CHECK_HANDLE(h) \
    if (!(h)) return fail(LEXLS_ERR_INVALID, "null handle")

    /// a device buffer that only grows: what the kept-factor calls (lse_kept_capi.h) keep in the handle between calls
    struct DeviceBuffer
    {
        void *ptr    = nullptr;
        size_t bytes = 0;
        /// room for `need` bytes: a buffer that holds fewer is freed (which waits for whatever still reads it) and made anew, its contents lost
        hipError_t reserve(size_t need)
        {
            if (need <= bytes) return hipSuccess;
            release();
            hipError_t e = hipMalloc(&ptr, need);
            if (e != hipSuccess) ptr = nullptr;
            else bytes = need;
            return e;
        }
        void release()
        {
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr, bytes = 0;
        }
        template <class T> T *as() const { return static_cast<T *>(ptr); }
    };

    /// what the host form of a kept-factor call leaves in the handle for its getter: three device buffers (the call's input, then its results) with
    /// room for `room` items, the `count` items of the last call, and the factor_epoch they belong to
    struct HostResults
    {
        DeviceBuffer buf[3];
        uint32_t room = 0, count = 0;
        bool valid     = false;
        uint64_t epoch = 0;
        struct Copy { void *dst; const void *src; size_t bytes; };
        /// room for n items, bytes[i] in buffer i: more than the buffers hold drops the results, frees all three and makes all three
        hipError_t make_room(uint32_t n, const size_t (&bytes)[3])
        {
            if (n <= room) return hipSuccess;
            valid = false, room = 0;
            release();
            for (int i = 0; i < 3; i++)
                if (hipError_t e = buf[i].reserve(bytes[i])) return e;
            room = n;
            return hipSuccess;
        }
        /// after a successful run on the buffers
        void stamp(uint32_t n, uint64_t factor_epoch) { valid = true, count = n, epoch = factor_epoch; }
        /// `getter`: the results of the last `call`, while they belong to the factor, to the host (a null dst is skipped)
        int fetch(lexls_lse_s *h, const char *getter, const char *call, std::initializer_list<Copy> copies) const;
        void release()
        {
            for (DeviceBuffer &b : buf) b.release();
        }
        template <class T> T *at(int i) const { return buf[i].as<T>(); }
    };
} // namespace

struct lexls_lse_s
{
    int device;
    hipStream_t stream;
    uint32_t batch, nVar, nObj, cap, max_rows, max_level_dim, min_level_dim;
    KernelPolicy policy; // lexls_lse_set_kernel_policy
    std::vector<uint32_t> maxdim, level_max;
    void *d_large_state;
    void *d_large_ws; // work space of the fast large path
    size_t large_ws_bytes;
    double *d_norms;
    double tol;
    bool dims_set, has_fixed, factor_valid, factor_in_hbm;
    uint64_t x_epoch, factor_epoch; // x_epoch == factor_epoch: d_x holds the basic solution of the current factor (lexls_lse_solve has nothing to do)
    const char *last_kernel;
    bool solve_reciprocal = false; // the plan of the last factorization: a later lexls_lse_solve may use the reciprocal diagonal
    const char *last_consumer = ""; // lexls_lse_last_consumer_kernel: the variant the last post-factorization launcher took
    uint32_t large_levels[2] = {0, 0}; // lexls_lse_last_large_levels: levels of the last factorization the one-launch form committed / gave up
    uint32_t reg_cfg = 0; // lexls_lse_last_reg_placement: what the regularized wave kernel of the last factorization was launched with (0: another kernel)

    double *d_in_owned;
    bool deferred_sync;       // lexls_lse_set_deferred_sync: copies are enqueued, not waited for
    uint32_t *h_dims_pinned;
    hipEvent_t dims_event;
    bool dims_event_pending;
    double *d_cdata;          // resident constraint data of the batch (lexls_lse_set_constraint_data)
    uint64_t cdata_per_problem;
    uint32_t *d_row_src, *d_row_ld;
    const double *d_in;
    double *d_fac, *d_x, *d_hh, *d_v, *d_lambda, *d_maxabs, *d_scratch, *d_fixed_val;
    uint32_t *d_perm, *d_rank, *d_fcol, *d_totalrank, *d_dims, *d_nfixed, *d_fixed_idx;
    uint8_t *d_fixed_type, *d_ctr_type, *d_skip;
    bool has_skip;
    bool fused_gather = false; // this round's rows are read by reference inside lqr_wave_kernel (lexls_internal_round_resident)
    // prefix reuse (lexls_lse_set_prefix_reuse): the register-resident wave kernel leaves what a later factorization needs to read levels back
    int32_t *d_resume_level = nullptr; // batch
    uint8_t *d_resume_state = nullptr; // batch x resume_state_bytes(nObj)
    bool resume_enabled = false;
    bool resume_valid   = false; // the LAST factorization of this handle left that state (same kernel, factor kept, no regularization)
    bool resume_armed   = false; // d_resume_level holds the levels for the NEXT factorization
    int32_t *d_sens, *d_objidx;
    uint32_t reg_type;    // LexLS::RegularizationType, 0 = none
    uint32_t reg_cg_iters;
    double reg_variable;
    double *d_reg_factor, *d_reg_scratch, *d_reg_mu;
    std::vector<double> reg_stage; // host copy behind the enqueued upload of the regularization factors (set_regularization)
    bool sens_scan; // lexls_lse_set_sensitivity_scan
    uint8_t *d_wrong_sign = nullptr; // batch x (nVar + cap): the set of lexls_lse_sensitivity_collect (allocated at its first call / LEXLS_ARRAY_WRONG_SIGN)
    // lexls_lse_multipliers: every objective's multipliers (batch x nObj x (nVar + cap)) and the scratch of its per-objective fallback
    double *d_mult        = nullptr;
    void *d_mult_scratch  = nullptr;
    bool mult_valid       = false;
    uint64_t mult_epoch   = 0;      // factor_epoch the multipliers belong to
    bool mult_swept       = false;
    // the kept-factor calls (lse_kept_capi.h).  A HostResults per family holds what its host form uploads and leaves for its getter, buffers in this order:
    //   adj   lexls_lse_solve_adjoint         g (batch x nVar) | grad_rhs (batch x cap) | grad_fixed (batch x nVar)
    //   adjm  lexls_lse_solve_adjoint_multi   G (batch x ncot x nVar) | grad_rhs (batch x ncot x cap) | grad_fixed (batch x ncot x nVar)
    //   adjA  lexls_lse_solve_adjoint_matrix  g (batch x nVar) | the gradient (batch x (nVar + 1) x cap) | the flags (batch)
    //   tan   lexls_lse_solve_tangent         the directions (ntan x batch x (nVar + 1) x cap | ntan x batch x nVar) | dx (ntan x batch x nVar); tan_flag: its flags (batch)
    //   srhs  lexls_lse_solve_rhs             the right-hand sides (nrhs x batch x cap) | fixed values | solutions (nrhs x batch x nVar)
    //   rres  lexls_lse_residual_rhs          the right-hand sides (nrhs x batch x cap) | fixed values | v (nrhs x batch x cap), then the costs (nrhs x batch x nObj)
    // made for the largest count so far (adj, adjA: one).  The work buffers both forms of a call run on, each made when a call first needs it:
    //   adj_work    the matrices of the regularized adjoint where they do not fit in LDS (adjoint_reg_work_bytes)
    //   adjm_work   the buffers of the per-cotangent form (adjoint_multi_work_bytes); the tangents' M^T w runs on them too
    //   adjrm_work  the matrices of the regularized multi kernel where they do not fit in LDS (adjoint_reg_multi_work_bytes): grows with the tiles of 64 cotangents
    //   adjA_work   the chain of launch_solve_adjoint_matrix (adjoint_matrix_work_bytes)
    //   tan_work, srhs_work  the chains of launch_solve_tangent and launch_solve_rhs: grow with the count, and with the placement (srhs_work: launch_residual_rhs too)
    HostResults adj, adjm, adjA, tan, srhs, rres;
    DeviceBuffer adj_work, adjm_work, adjrm_work, adjA_work, tan_flag, tan_work, srhs_work;
    bool adj_regularized       = false; // lexls_lse_set_adjoint_regularized: the single-cotangent calls serve damped factorizations (off: UNSUPPORTED, as before)
    bool adj_regularized_multi = false; // lexls_lse_set_adjoint_regularized_multi: the multi-cotangent calls serve damped factorizations (off: UNSUPPORTED, as before)
    // accuracy guard (lexls_lse_set_accuracy_guard): mode 0 off, 1 report, 2 report + re-solve; arrays allocated when first switched on
    int guard_mode           = 0;
    double guard_threshold   = 0.0;
    double *d_guard_est      = nullptr; // batch
    uint8_t *d_guard_status  = nullptr; // batch
    uint32_t *d_guard_ind    = nullptr; // 1 + batch: [count, flagged problems]
    bool guard_last          = false;   // the last factorization ran with the guard on (the arrays describe it)
    char *d_round_in, *d_round_out; // the per-round arrays live in two slabs (lexls_lse_round_layout): one copy each way per round
    lexls_round_layout lay;

    LseArgs args() const
    {
        LseArgs a;
        a.batch = batch;
        a.nVar  = nVar;
        a.nObj  = nObj;
        a.cap   = cap;
        a.ldp   = odd_ld(max_rows);
        a.tol   = tol;
        a.in    = d_in;
        a.fac   = d_fac;
        a.x     = d_x;
        a.hh    = d_hh;
        a.perm  = d_perm;
        a.rank  = d_rank;
        a.fcol  = d_fcol;
        a.totalrank  = d_totalrank;
        a.dims       = d_dims;
        a.uniform_dim = (dims_set && min_level_dim == max_level_dim) ? max_level_dim : 0u;
        a.nfixed     = has_fixed ? d_nfixed : nullptr;
        a.fixed_idx  = d_fixed_idx;
        a.fixed_val  = d_fixed_val;
        a.fixed_type = d_fixed_type;
        a.ctr_type   = d_ctr_type;
        a.v          = d_v;
        a.lambda     = d_lambda;
        a.sens       = d_sens;
        a.maxabs     = d_maxabs;
        a.scratch    = d_scratch;
        a.skip       = has_skip ? d_skip : nullptr;
        a.reg_type     = reg_type;
        a.reg_cg_iters = reg_cg_iters;
        a.reg_variable = reg_variable;
        a.reg_factor   = d_reg_factor;
        a.reg_scratch  = d_reg_scratch;
        a.reg_mu       = d_reg_mu;
        a.g_cdata      = fused_gather ? d_cdata : nullptr;
        a.g_per        = cdata_per_problem;
        a.g_row_src    = d_row_src;
        a.g_row_ld     = d_row_ld;
        a.resume_state = resume_enabled ? d_resume_state : nullptr;
        a.resume_level = (resume_enabled && resume_armed && resume_valid) ? d_resume_level : nullptr;
        a.wrong_sign   = d_wrong_sign;
        return a;
    }
    size_t problem_elems() const { return (size_t)cap * (nVar + 1); }
};

extern "C"
{
    const char *lexls_last_error(void) { return g_err.c_str(); }
    void lexls_internal_set_error(const char *msg) { g_err = msg ? msg : ""; }
    int lexls_version(void) { return 100; }

    int lexls_device_count(int *count)
    {
        int n        = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (count) *count = (e == hipSuccess) ? n : 0;
        if (e != hipSuccess || n == 0) return fail(LEXLS_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
        return LEXLS_OK;
    }

    int lexls_lse_create(lexls_lse_t *out, int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_maxObjDim)
    {
        if (!out || !h_maxObjDim || batch == 0 || nVar == 0 || nObj == 0) return fail(LEXLS_ERR_INVALID, "lexls_lse_create: bad argument");
        int ndev = 0;
        if (lexls_device_count(&ndev) != LEXLS_OK) return LEXLS_ERR_NO_DEVICE;
        if (device < 0 || device >= ndev) return fail(LEXLS_ERR_INVALID, "lexls_lse_create: device index out of range");
        HIP_TRY(hipSetDevice(device));

        lexls_lse_s *h = new (std::nothrow) lexls_lse_s();
        if (!h) return fail(LEXLS_ERR_INVALID, "out of host memory");
        h->device = device;
        h->stream = nullptr;
        h->batch  = batch;
        h->nVar   = nVar;
        h->nObj   = nObj;
        h->maxdim.assign(h_maxObjDim, h_maxObjDim + nObj);
        h->cap = 0;
        for (uint32_t k = 0; k < nObj; k++) h->cap += h_maxObjDim[k];
        if (h->cap == 0)
        {
            delete h;
            return fail(LEXLS_ERR_INVALID, "lexls_lse_create: zero capacity");
        }
        h->max_rows    = h->cap;
        h->max_level_dim = 0;
        h->min_level_dim = 0;
        h->policy = KernelPolicy::automatic;
        if (const char *e = std::getenv("LEXLS_KERNEL_POLICY")) h->policy = static_cast<KernelPolicy>(std::atoi(e)); // diagnostic default of lexls_lse_set_kernel_policy
        h->tol         = 1e-12; // typedefs.h:120
        h->dims_set    = false;
        h->has_fixed   = false;
        h->factor_valid = h->factor_in_hbm = false;
        h->last_kernel = "";
        h->d_in_owned  = nullptr;
        h->d_cdata     = nullptr;
        h->reg_type    = 0;
        h->reg_cg_iters = 10; // typedefs.h:170
        h->reg_variable = 0.0;
        h->d_reg_factor = h->d_reg_scratch = h->d_reg_mu = nullptr;
        h->deferred_sync = false;
        h->h_dims_pinned = nullptr;
        h->dims_event = nullptr;
        h->dims_event_pending = false;
        h->cdata_per_problem = 0;
        h->d_round_in = h->d_round_out = nullptr;
        h->d_in        = nullptr;
        h->d_scratch   = nullptr;

        const size_t B = batch, n = nVar, cap = h->cap;
        hipError_t e   = hipSuccess;
        auto alloc     = [&](void **p, size_t bytes) {
            if (e == hipSuccess) e = hipMalloc(p, bytes ? bytes : 8);
        };
        // the small per-round arrays are carved out of two slabs so that a lock-step driver moves each with ONE copy
        {
            auto up = [](uint64_t v) { return (v + 255) & ~uint64_t(255); };
            lexls_round_layout &L = h->lay;
            uint64_t o   = 0;
            L.dims       = o, o = up(o + 4 * B * nObj);
            L.nfixed     = o, o = up(o + 4 * B);
            L.fixed_idx  = o, o = up(o + 4 * B * n);
            L.fixed_val  = o, o = up(o + 8 * B * n);
            L.skip       = o, o = up(o + B);
            L.obj_index  = o, o = up(o + 4 * B);
            L.row_src    = o, o = up(o + 4 * B * cap);
            L.row_ld     = o, o = up(o + 4 * B * cap);
            L.fixed_type = o, o = up(o + B * n);
            L.ctr_type   = o, o = up(o + B * cap);
            L.in_bytes   = o;
            o            = 0;
            L.x          = o, o = up(o + 8 * B * n);
            L.total_rank = o, o = up(o + 4 * B);
            L.found      = o, o = up(o + 4 * B * 3);
            L.max_abs    = o, o = up(o + 8 * B);
            L.out_bytes  = o;
            alloc((void **)&h->d_round_in, L.in_bytes);
            alloc((void **)&h->d_round_out, L.out_bytes);
            if (e == hipSuccess) e = hipMemset(h->d_round_in, 0, L.in_bytes);
            if (e == hipSuccess) e = hipMemset(h->d_round_out, 0, L.out_bytes);
            if (e == hipSuccess)
            {
                char *in = h->d_round_in, *out_ = h->d_round_out;
                h->d_dims       = (uint32_t *)(in + L.dims);
                h->d_nfixed     = (uint32_t *)(in + L.nfixed);
                h->d_fixed_idx  = (uint32_t *)(in + L.fixed_idx);
                h->d_fixed_val  = (double *)(in + L.fixed_val);
                h->d_skip       = (uint8_t *)(in + L.skip);
                h->d_objidx     = (int32_t *)(in + L.obj_index);
                h->d_row_src    = (uint32_t *)(in + L.row_src);
                h->d_row_ld     = (uint32_t *)(in + L.row_ld);
                h->d_fixed_type = (uint8_t *)(in + L.fixed_type);
                h->d_ctr_type   = (uint8_t *)(in + L.ctr_type);
                h->d_x          = (double *)(out_ + L.x);
                h->d_totalrank  = (uint32_t *)(out_ + L.total_rank);
                h->d_sens       = (int32_t *)(out_ + L.found);
                h->d_maxabs     = (double *)(out_ + L.max_abs);
            }
        }
        alloc((void **)&h->d_fac, 8 * B * h->problem_elems());
        alloc((void **)&h->d_hh, 8 * B * cap);
        alloc((void **)&h->d_v, 8 * B * cap);
        alloc((void **)&h->d_lambda, 8 * B * (n + cap));
        alloc((void **)&h->d_perm, 4 * B * n);
        alloc((void **)&h->d_rank, 4 * B * nObj);
        alloc((void **)&h->d_fcol, 4 * B * nObj);
        if (e != hipSuccess)
        {
            lexls_lse_destroy(h);
            return fail(LEXLS_ERR_HIP, std::string("lexls_lse_create: ") + hipGetErrorString(e));
        }
        // default dims = capacities (LexLSE(nVar,nObj,ObjDim) constructor semantics, lexlse.h:50-54)
        *out = h;
        return lexls_lse_set_obj_dim(h, h_maxObjDim, 0);
    }

    int lexls_lse_destroy(lexls_lse_t h)
    {
        if (!h) return LEXLS_OK;
        (void)hipSetDevice(h->device);
        void *ptrs[] = {h->d_in_owned, h->d_fac, h->d_hh, h->d_v, h->d_lambda, h->d_scratch, h->d_perm, h->d_rank, h->d_fcol, h->d_round_in, h->d_round_out,
                        h->d_large_state, h->d_large_ws, h->d_norms, h->d_cdata, h->d_reg_factor, h->d_reg_scratch, h->d_reg_mu, h->d_resume_level, h->d_resume_state,
                        h->d_guard_est, h->d_guard_status, h->d_guard_ind, h->d_mult, h->d_mult_scratch, h->d_wrong_sign};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
        h->adj.release(), h->adj_work.release(), h->adjm.release(), h->adjm_work.release(), h->adjrm_work.release(), h->adjA.release(), h->adjA_work.release();
        h->tan.release(), h->tan_flag.release(), h->tan_work.release(), h->srhs.release(), h->srhs_work.release(), h->rres.release();
        if (h->h_dims_pinned) (void)hipHostFree(h->h_dims_pinned);
        if (h->dims_event) (void)hipEventDestroy(h->dims_event);
        delete h;
        return LEXLS_OK;
    }

    int lexls_lse_set_stream(lexls_lse_t h, void *hip_stream)
    {
        CHECK_HANDLE(h);
        h->stream = static_cast<hipStream_t>(hip_stream);
        return LEXLS_OK;
    }

    int lexls_lse_synchronize(lexls_lse_t h)
    {
        CHECK_HANDLE(h);
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }

    /// What plan_lqr (lexls_dispatch.h) reads, from the handle as it stands; the environment and device facts are looked up here
    /// (LEXLS_QTOL at every call, so that a caller may change it between solves)
    static DispatchQuery query_of(const lexls_lse_s *h, bool write_factor, bool do_solve, bool opportunistic_solve = false)
    {
        DispatchQuery q;
        q.batch = h->batch, q.nVar = h->nVar, q.nObj = h->nObj, q.cap = h->cap;
        q.uniform_dim   = (h->dims_set && h->min_level_dim == h->max_level_dim) ? h->max_level_dim : 0u;
        q.max_rows = h->max_rows, q.max_level_dim = h->max_level_dim;
        q.has_fixed = h->has_fixed, q.reg_type = h->reg_type, q.has_dims = h->d_dims != nullptr;
        const uintptr_t in    = reinterpret_cast<uintptr_t>(h->d_in);
        q.align               = (in & 15u) == 0 ? 16u : ((in & 7u) == 0 ? 8u : 0u);
        q.gather_by_reference = h->fused_gather;
        q.write_factor = write_factor, q.do_solve = do_solve, q.opportunistic_solve = opportunistic_solve;
        q.policy = h->policy, q.guard = h->guard_mode != 0;
        const char *e   = std::getenv("LEXLS_QTOL");
        q.qtol_off      = e && std::atoi(e) == 0;
        q.wave_capacity = resident_wave_capacity();
        q.reg_lds_share = wave_reg_lds_share();
        return q;
    }

    /// ... of a resident LexLSI round, factor kept: the capacities given at creation stand for the dimensions (this round's are known to the
    /// device only).  Shape, policy and LDS share only — no device is asked (callers that plan a launch add wave_capacity); the handle is not touched
    static DispatchQuery resident_query_of(const lexls_lse_s *h, bool has_fixed, uint32_t reg_type)
    {
        DispatchQuery q;
        q.batch = h->batch, q.nVar = h->nVar, q.nObj = h->nObj, q.cap = h->cap;
        q.max_rows = h->cap ? h->cap : 1;
        for (uint32_t v : h->maxdim) q.max_level_dim = v > q.max_level_dim ? v : q.max_level_dim;
        q.has_fixed = has_fixed, q.reg_type = reg_type, q.policy = h->policy, q.reg_lds_share = wave_reg_lds_share();
        return q;
    }

    /// the fields lexls_internal_round_resident and lexls_internal_resident_fused both set for such a round
    static void enter_resident_round(lexls_lse_t h, const DispatchQuery &q, bool gather_by_reference)
    {
        h->level_max.assign(h->maxdim.begin(), h->maxdim.end());
        h->max_rows      = q.max_rows;
        h->max_level_dim = q.max_level_dim;
        h->min_level_dim = 0; // this round's dimensions are known to the device only
        h->dims_set      = true;
        h->has_fixed     = q.has_fixed;
        h->has_skip      = true;
        h->fused_gather  = gather_by_reference;
        h->d_in          = h->d_in_owned;
    }

    /// A round whose rows are read by reference inside the register-resident wave kernel (fused_gather) leaves `in` unassembled.  Anything that
    /// can send the next factorization to ANOTHER kernel (kernel policy, regularization type) assembles the rows first.
    static hipError_t materialize_fused_gather(lexls_lse_t h)
    {
        if (!h->fused_gather) return hipSuccess;
        hipError_t e = hipSetDevice(h->device);
        if (e != hipSuccess) return e;
        h->fused_gather = false;
        LseArgs a       = h->args();
        e = launch_gather_rows(a, h->d_cdata, h->cdata_per_problem, h->d_row_src, h->d_row_ld, h->d_in_owned, h->stream);
        h->d_in = h->d_in_owned;
        return e;
    }

    /// what every way of setting a regularization shares: type and variable factor into the handle, the kept factor dropped, the device arrays
    /// the regularized kernels read made (type != 0) — nothing is written into d_reg_factor
    static int prepare_regularization(lexls_lse_t h, int type, double variable_factor)
    {
        if ((uint32_t)type != h->reg_type) HIP_TRY(materialize_fused_gather(h));
        HIP_TRY(hipSetDevice(h->device));
        h->factor_valid = false;
        h->reg_type     = (uint32_t)type;
        h->reg_variable = variable_factor;
        if (type == 0) return LEXLS_OK;
        const size_t B = h->batch, nObj = h->nObj;
        if (!h->d_reg_factor) HIP_TRY(hipMalloc((void **)&h->d_reg_factor, 8 * B * nObj));
        if (!h->d_reg_scratch)
        {
            const size_t bytes = 8 * B * reg_scratch_doubles(h->nVar);
            HIP_TRY(hipMalloc((void **)&h->d_reg_scratch, bytes));
            HIP_TRY(hipMemsetAsync(h->d_reg_scratch, 0, bytes, h->stream));
        }
        if (type == 7 && !h->d_reg_mu) // X_mu, X_mu_rhs, residual_mu of the reference's experimental type (lexlse.h:96-99)
        {
            const size_t bytes = 8 * B * reg_mu_doubles(h->nVar, h->nObj, h->cap);
            HIP_TRY(hipMalloc((void **)&h->d_reg_mu, bytes));
            HIP_TRY(hipMemsetAsync(h->d_reg_mu, 0, bytes, h->stream));
        }
        return LEXLS_OK;
    }

    /// lexls_lse_set_regularization / lexls_internal_set_regularization_block(_per_problem): the factors are staged in the handle (reg_stage) and
    /// enqueued in its stream; wait: the stream is synchronised before returning
    static int set_regularization(lexls_lse_t h, int type, const double *h_factors, int per_problem, double variable_factor, bool wait)
    {
        const int rc = prepare_regularization(h, type, variable_factor);
        if (rc != LEXLS_OK || type == 0) return rc;
        const size_t B = h->batch, nObj = h->nObj;
        h->reg_stage.assign(B * nObj, 0.0);
        if (h_factors)
            for (size_t b = 0; b < B; b++)
                for (size_t k = 0; k < nObj; k++) h->reg_stage[b * nObj + k] = per_problem ? h_factors[b * nObj + k] : h_factors[k];
        HIP_TRY(hipMemcpyAsync(h->d_reg_factor, h->reg_stage.data(), 8 * B * nObj, hipMemcpyHostToDevice, h->stream));
        if (wait) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }

    int lexls_lse_set_regularization(lexls_lse_t h, int type, const double *h_factors, int per_problem, double variable_factor)
    {
        CHECK_HANDLE(h);
        if (type < 0 || type > 9) return fail(LEXLS_ERR_INVALID, "set_regularization: unknown regularization type");
        return set_regularization(h, type, h_factors, per_problem, variable_factor, true);
    }

    /* internal (the lock-step LexLSI driver): the regularization of ONE run as a block that stays on the device for its length — the type, the
     * variable factor and the CG iteration bound (they travel in every launch's argument block) and one factor per LexLSE level, the same for
     * every problem of the batch, in the array the kernels read (batch x nObj).  What lexls_lse_set_regularization + lexls_lse_set_cg_iterations
     * set, but only ENQUEUED in the handle's stream: nothing is waited for (the staging copy lives in the handle; the caller synchronises the
     * stream before the next call, as every run of the driver does when it downloads its results).  Also drops what prefix reuse kept: a
     * regularized factorization reads nothing back and leaves nothing to read back. */
    int lexls_internal_set_regularization_block(lexls_lse_t h, int type, const double *h_level_factors, double variable_factor, uint32_t cg_iterations)
    {
        CHECK_HANDLE(h);
        if (type < 1 || type > 9) return fail(LEXLS_ERR_INVALID, "set_regularization_block: regularization type outside 1 .. 9");
        h->resume_valid = false;
        h->resume_armed = false;
        h->reg_cg_iters = cg_iterations;
        return set_regularization(h, type, h_level_factors, 0, variable_factor, false);
    }

    /* internal: lexls_internal_set_regularization_block with factors of its own for every problem — h_factors is batch x nObj, problem-major, the
     * array the kernels read (they index it by problem already).  Enqueued only, like the shared form. */
    int lexls_internal_set_regularization_block_per_problem(lexls_lse_t h, int type, const double *h_factors, double variable_factor, uint32_t cg_iterations)
    {
        CHECK_HANDLE(h);
        if (type < 1 || type > 9) return fail(LEXLS_ERR_INVALID, "set_regularization_block: regularization type outside 1 .. 9");
        if (!h_factors) return fail(LEXLS_ERR_INVALID, "set_regularization_block: null factors");
        h->resume_valid = false;
        h->resume_armed = false;
        h->reg_cg_iters = cg_iterations;
        return set_regularization(h, type, h_factors, 1, variable_factor, false);
    }

    /* internal: the regularization block of a run whose factors the CALLER writes on the device — type, variable factor and CG bound are set and
     * the kept factor dropped as lexls_internal_set_regularization_block does, the arrays exist, and *d_factors is the batch x nObj array the
     * kernels read: the caller fills it in the handle's stream before the first factorization.  No host staging: nothing of the handle's own
     * staging copy is enqueued over what the caller writes. */
    int lexls_internal_set_regularization_block_device(lexls_lse_t h, int type, double variable_factor, uint32_t cg_iterations, double **d_factors)
    {
        CHECK_HANDLE(h);
        if (type < 1 || type > 9) return fail(LEXLS_ERR_INVALID, "set_regularization_block: regularization type outside 1 .. 9");
        if (!d_factors) return fail(LEXLS_ERR_INVALID, "set_regularization_block: null output");
        h->resume_valid = false;
        h->resume_armed = false;
        h->reg_cg_iters = cg_iterations;
        const int rc = prepare_regularization(h, type, variable_factor);
        if (rc == LEXLS_OK) *d_factors = h->d_reg_factor;
        return rc;
    }

    /* internal (the lock-step LexLSI driver): can the resident iterations of this handle's batch run under regularization `type`?  Every type
     * the REG instantiations of the register-resident wave kernel serve (all but the experimental type 7) on the shapes that kernel takes, as
     * long as the l-QR image plus the regularization routines' vectors fit a workgroup's LDS (their work matrix and the null-space basis are
     * optional there).  Decided from the capacities given at creation: nothing is launched, nothing changes. */
    int lexls_internal_resident_reg_serves(lexls_lse_t h, int type)
    {
        if (!h || type < 1 || type > 9 || h->policy == KernelPolicy::generic_only) return 0;
        const DispatchQuery q = resident_query_of(h, true, (uint32_t)type);
        return (dispatch::wave_family_supports(q) && wave_reg_kernel_fits(q)) ? 1 : 0;
    }

    int lexls_lse_set_cg_iterations(lexls_lse_t h, uint32_t max_iterations)
    {
        CHECK_HANDLE(h);
        h->reg_cg_iters = max_iterations;
        h->factor_valid = false;
        return LEXLS_OK;
    }

    int lexls_lse_set_deferred_sync(lexls_lse_t h, int on)
    {
        CHECK_HANDLE(h);
        if (!on && h->deferred_sync) // leaving the mode: everything enqueued so far completes first
        {
            HIP_TRY(hipSetDevice(h->device));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        h->deferred_sync = on != 0;
        return LEXLS_OK;
    }

    int lexls_lse_set_tolerance(lexls_lse_t h, double tol)
    {
        CHECK_HANDLE(h);
        if (tol != h->tol)
        {
            h->factor_valid = false; // a factor / solution computed with the old tolerance must not be served any more
            // ... nor read back by prefix reuse: the levels of the previous factorization carry the ranks of the old tolerance (the kernel
            // replays them, it does not repeat the rank test).  Resume levels armed before this call are dropped with the state
            h->resume_valid = false;
            h->resume_armed = false;
        }
        h->tol = tol;
        return LEXLS_OK;
    }

    int lexls_lse_set_obj_dim(lexls_lse_t h, const uint32_t *h_dims, int per_problem)
    {
        CHECK_HANDLE(h);
        if (!h_dims) return fail(LEXLS_ERR_INVALID, "set_obj_dim: null dims");
        const size_t nd = (size_t)h->batch * h->nObj;
        std::vector<uint32_t> d_tmp;
        uint32_t *d = nullptr;
        if (h->deferred_sync) // the copy below is not waited for: its source must outlive this call and be DMA-able
        {
            HIP_TRY(hipSetDevice(h->device));
            if (!h->h_dims_pinned) HIP_TRY(hipHostMalloc((void **)&h->h_dims_pinned, 4 * nd, hipHostMallocDefault));
            else if (h->dims_event_pending) HIP_TRY(hipEventSynchronize(h->dims_event)); // the previous copy out of this buffer is done
            d = h->h_dims_pinned;
        }
        else
        {
            d_tmp.resize(nd);
            d = d_tmp.data();
        }
        uint32_t max_rows = 0, max_level = 0, min_level = 0xffffffffu;
        h->level_max.assign(h->nObj, 0);
        for (uint32_t b = 0; b < h->batch; b++)
        {
            uint32_t m = 0;
            for (uint32_t k = 0; k < h->nObj; k++)
            {
                const uint32_t v = per_problem ? h_dims[(size_t)b * h->nObj + k] : h_dims[k];
                if (v > h->maxdim[k]) return fail(LEXLS_ERR_INVALID, "set_obj_dim: dimension exceeds the capacity given at creation");
                d[(size_t)b * h->nObj + k] = v;
                m += v;
                if (v > max_level) max_level = v;
                if (v < min_level) min_level = v;
                if (v > h->level_max[k]) h->level_max[k] = v;
            }
            if (m > max_rows) max_rows = m;
        }
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(h->d_dims, d, 4 * nd, hipMemcpyHostToDevice, h->stream));
        if (h->deferred_sync)
        {
            if (!h->dims_event) HIP_TRY(hipEventCreateWithFlags(&h->dims_event, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(h->dims_event, h->stream));
            h->dims_event_pending = true;
        }
        else
            HIP_TRY(hipStreamSynchronize(h->stream)); // d is a temporary
        h->max_rows      = max_rows ? max_rows : 1;
        h->max_level_dim = max_level;
        h->min_level_dim = min_level;
        h->dims_set     = true;
        h->factor_valid = false;
        return LEXLS_OK;
    }

    int lexls_lse_set_fixed(lexls_lse_t h, const uint32_t *h_nfixed, const uint32_t *h_index, const double *h_value, const uint8_t *h_type)
    {
        CHECK_HANDLE(h);
        HIP_TRY(hipSetDevice(h->device));
        h->factor_valid = false;
        if (!h_nfixed)
        {
            h->has_fixed = false;
            return LEXLS_OK;
        }
        if (!h_index || !h_value) return fail(LEXLS_ERR_INVALID, "set_fixed: null index/value");
        bool any = false;
        for (uint32_t b = 0; b < h->batch; b++)
        {
            if (h_nfixed[b] > h->nVar) return fail(LEXLS_ERR_INVALID, "Cannot fix more than nVar variables"); // lexlse.h:1453
            for (uint32_t k = 0; k < h_nfixed[b]; k++)
                if (h_index[(size_t)b * h->nVar + k] >= h->nVar) return fail(LEXLS_ERR_INVALID, "set_fixed: variable index out of range");
            any = any || h_nfixed[b] > 0;
        }
        const size_t B = h->batch, n = h->nVar;
        HIP_TRY(hipMemcpyAsync(h->d_nfixed, h_nfixed, 4 * B, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->d_fixed_idx, h_index, 4 * B * n, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->d_fixed_val, h_value, 8 * B * n, hipMemcpyHostToDevice, h->stream));
        if (h_type)
            HIP_TRY(hipMemcpyAsync(h->d_fixed_type, h_type, B * n, hipMemcpyHostToDevice, h->stream));
        else
            HIP_TRY(hipMemsetAsync(h->d_fixed_type, CTR_ACTIVE_UB, B * n, h->stream)); // default of fixVariable, lexlse.h:1381
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        h->has_fixed = any;
        return LEXLS_OK;
    }

    int lexls_lse_set_fixed_type(lexls_lse_t h, const uint8_t *h_type)
    {
        CHECK_HANDLE(h);
        if (!h_type) return fail(LEXLS_ERR_INVALID, "set_fixed_type: null");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(h->d_fixed_type, h_type, (size_t)h->batch * h->nVar, hipMemcpyHostToDevice, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK; // activation types only matter to the dual solve: the factorization stays valid
    }

    int lexls_lse_set_ctr_type(lexls_lse_t h, const uint8_t *h_types)
    {
        CHECK_HANDLE(h);
        if (!h_types) return fail(LEXLS_ERR_INVALID, "set_ctr_type: null");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(h->d_ctr_type, h_types, (size_t)h->batch * h->cap, hipMemcpyHostToDevice, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }

    int lexls_lse_set_skip(lexls_lse_t h, const uint8_t *h_skip)
    {
        CHECK_HANDLE(h);
        if (!h_skip)
        {
            h->has_skip = false;
            return LEXLS_OK;
        }
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(h->d_skip, h_skip, (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        h->has_skip = false; // as upload_round: kernels look at the mask only when some problem is masked (an all-zero mask is no mask)
        for (uint32_t b = 0; b < h->batch && !h->has_skip; b++) h->has_skip = h_skip[b] != 0;
        return LEXLS_OK;
    }

    int lexls_lse_set_problem_host(lexls_lse_t h, const double *h_lod)
    {
        CHECK_HANDLE(h);
        if (!h_lod) return fail(LEXLS_ERR_INVALID, "set_problem_host: null");
        HIP_TRY(hipSetDevice(h->device));
        const size_t bytes = 8 * (size_t)h->batch * h->problem_elems();
        if (!h->d_in_owned) HIP_TRY(hipMalloc((void **)&h->d_in_owned, bytes));
        HIP_TRY(hipMemcpyAsync(h->d_in_owned, h_lod, bytes, hipMemcpyHostToDevice, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        h->d_in         = h->d_in_owned;
        h->fused_gather = false;
        h->factor_valid = false;
        return LEXLS_OK;
    }

    /// the batch's resident constraint data from host memory (waited for) or device memory (enqueued)
    static int set_constraint_data(lexls_lse_t h, const char *who, const double *data, uint64_t per_problem, hipMemcpyKind kind)
    {
        CHECK_HANDLE(h);
        if (!data || per_problem == 0) return fail(LEXLS_ERR_INVALID, std::string(who) + ": null / empty");
        HIP_TRY(hipSetDevice(h->device));
        const size_t bytes = 8 * (size_t)h->batch * per_problem;
        if (h->d_cdata && h->cdata_per_problem != per_problem)
        {
            HIP_TRY(hipFree(h->d_cdata));
            h->d_cdata = nullptr;
        }
        if (!h->d_cdata) HIP_TRY(hipMalloc((void **)&h->d_cdata, bytes));
        h->cdata_per_problem = per_problem;
        HIP_TRY(hipMemcpyAsync(h->d_cdata, data, bytes, kind, h->stream));
        if (kind == hipMemcpyHostToDevice) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }
    int lexls_lse_set_constraint_data(lexls_lse_t h, const double *h_data, uint64_t per_problem) { return set_constraint_data(h, "set_constraint_data", h_data, per_problem, hipMemcpyHostToDevice); }
    int lexls_internal_set_constraint_data_device(lexls_lse_t h, const double *d_data, uint64_t per_problem) { return set_constraint_data(h, "set_constraint_data_device", d_data, per_problem, hipMemcpyDeviceToDevice); }

    int lexls_internal_ensure_gather_buffer(lexls_lse_t h)
    {
        CHECK_HANDLE(h);
        if (h->d_in_owned) return LEXLS_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMalloc((void **)&h->d_in_owned, 8 * (size_t)h->batch * h->problem_elems()));
        HIP_TRY(hipMemsetAsync(h->d_in_owned, 0, 8 * (size_t)h->batch * h->problem_elems(), h->stream));
        return LEXLS_OK;
    }

    int lexls_lse_gather_problem(lexls_lse_t h, const uint32_t *h_row_src, const uint32_t *h_row_ld)
    {
        CHECK_HANDLE(h);
        if (!h_row_src || !h_row_ld) return fail(LEXLS_ERR_INVALID, "gather_problem: null");
        if (!h->d_cdata) return fail(LEXLS_ERR_INVALID, "gather_problem: call lexls_lse_set_constraint_data first");
        const size_t B = h->batch, cap = h->cap;
        // every element a row refers to must lie inside the problem's resident block (the kernel does not check)
        for (size_t i = 0; i < B * cap; i++)
        {
            const uint64_t ld = h_row_ld[i] & 0x7fffffffu;
            if (ld && (uint64_t)h_row_src[i] + (uint64_t)(h->nVar + 1) * ld >= h->cdata_per_problem)
                return fail(LEXLS_ERR_INVALID, "gather_problem: row reference outside the constraint data");
        }
        if (int rc = lexls_internal_ensure_gather_buffer(h)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(h->d_row_src, h_row_src, 4 * B * cap, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->d_row_ld, h_row_ld, 4 * B * cap, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(launch_gather_rows(h->args(), h->d_cdata, h->cdata_per_problem, h->d_row_src, h->d_row_ld, h->d_in_owned, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream)); // the host arrays may be reused by the caller
        h->d_in         = h->d_in_owned;
        h->fused_gather = false;
        h->factor_valid = false;
        return LEXLS_OK;
    }

    int lexls_lse_round_layout(lexls_lse_t h, lexls_round_layout *out)
    {
        CHECK_HANDLE(h);
        if (!out) return fail(LEXLS_ERR_INVALID, "round_layout: null");
        *out = h->lay;
        return LEXLS_OK;
    }

    const double *lexls_internal_cdata(lexls_lse_t h) { return h ? h->d_cdata : nullptr; }
    double *lexls_internal_cdata_writable(lexls_lse_t h) { return h ? h->d_cdata : nullptr; }

    char *lexls_internal_round_in(lexls_lse_t h) { return h ? h->d_round_in : nullptr; }
    int lexls_internal_round_resident(lexls_lse_t h, int has_fixed)
    {
        CHECK_HANDLE(h);
        if (!h->d_cdata || !h->d_in_owned) return fail(LEXLS_ERR_INVALID, "round_resident: needs resident constraint data and one uploaded round");
        HIP_TRY(hipSetDevice(h->device));
        // the register-resident wave kernel reads the rows by reference itself where the plan says so (plan_round_gathers_by_reference)
        DispatchQuery q = resident_query_of(h, has_fixed != 0, h->reg_type);
        q.wave_capacity   = resident_wave_capacity();
        const bool by_ref = plan_round_gathers_by_reference(q);
        enter_resident_round(h, q, by_ref);
        h->factor_valid = false;
        if (!by_ref) HIP_TRY(launch_gather_rows(h->args(), h->d_cdata, h->cdata_per_problem, h->d_row_src, h->d_row_ld, h->d_in_owned, h->stream));
        return LEXLS_OK;
    }

    /// The plan of the persistent LexLSI launch for a run of regularization `reg_type` on this handle's batch, from the capacities given at creation
    /// and the environment's switch (none: not taken); q: the query it was made from.  lexls_internal_resident_fused launches by it and
    /// lexls_internal_resident_fused_serves answers from it: one decision
    static KernelId plan_resident_fused(const lexls_lse_s *h, bool has_fixed, uint32_t reg_type, DispatchQuery &q)
    {
        q               = resident_query_of(h, has_fixed, reg_type);
        q.wave_capacity = resident_wave_capacity();
        LseArgs a       = h->args(); // (the sweep's test reads the shape and the regularization type)
        a.reg_type      = reg_type;
        q.sweep_serves  = sensitivity_sweep_serves(a, q.max_level_dim);
        return std::getenv("LEXLS_LSI_NO_FUSED") ? KernelId::none : plan_lsi_fused(q);
    }

    /* internal (the lock-step LexLSI driver): ALL remaining resident iterations in one persistent launch — per instance l-QR (rows gathered by
     * reference, levels above the changed one read back) -> removal sweep -> lsi_iterate_body, until the instance stops (at most `count`
     * iterations).  Same preparation and the same bookkeeping as lexls_internal_round_resident + lexls_internal_arm_resume +
     * lexls_lse_factorize_solve(h, 1) + lexls_lse_sensitivity_resident per stage.  Returns 1 (nothing done, nothing changed) when the shape has no
     * persistent instantiation: the driver then enqueues the stage's three kernels as before. */
    int lexls_internal_resident_fused(lexls_lse_t h, int has_fixed, int count, double tolW, double tolC, const void *resident_args, size_t resident_args_bytes)
    {
        CHECK_HANDLE(h);
        if (!h->d_cdata || !h->d_in_owned) return fail(LEXLS_ERR_INVALID, "resident_fused: needs resident constraint data and one uploaded round");
        const bool reg = h->reg_type != 0; // the launch with the regularized l-QR: no prefix reuse (lqr_small_impl.h), so no resume levels either way
        HIP_TRY(hipSetDevice(h->device));
        DispatchQuery q;
        const KernelId id = plan_resident_fused(h, has_fixed != 0, h->reg_type, q);
        if (id == KernelId::none) return 1;
        // the arguments lexls_internal_round_resident + lexls_internal_arm_resume would leave — on a copy: nothing changes when the launch is not taken
        LseArgs pa      = h->args();
        pa.ldp          = odd_ld(q.max_rows);
        pa.in           = h->d_in_owned;
        pa.uniform_dim  = 0;
        pa.nfixed       = q.has_fixed ? h->d_nfixed : nullptr;
        pa.skip         = h->d_skip;
        pa.g_cdata      = h->d_cdata;
        pa.resume_level = (h->resume_enabled && !reg && h->resume_valid) ? h->d_resume_level : nullptr;
        const FusedCall call{q.max_level_dim, h->d_objidx, tolW, tolC, h->sens_scan, resident_args, resident_args_bytes, count};
        LaunchExtras x;
        x.fused            = &call;
        const hipError_t e = launch_kernel(id, pa, h->stream, x);
        if (e == hipErrorNotSupported) return 1;
        HIP_TRY(e);
        h->last_kernel      = kernel_name(id);
        h->solve_reciprocal = false;
        enter_resident_round(h, q, true);
        h->resume_armed  = false;
        h->resume_valid  = h->resume_enabled && h->d_resume_state != nullptr && !reg;
        h->factor_valid  = true;
        h->factor_epoch++;
        h->x_epoch       = h->factor_epoch;
        h->factor_in_hbm = true;
        return LEXLS_OK;
    }

    /* internal (the lock-step LexLSI driver): would lexls_internal_resident_fused take the launch for a run of regularization `type` (0: none) on this
     * handle's batch?  The launch's own plan (plan_resident_fused) and the launcher's own LDS sum (lsi_fused_lds_bytes of the planned instantiation;
     * resident_lds: the driver's share, resident_lds_per_wave): nothing is launched, nothing changes. */
    int lexls_internal_resident_fused_serves(lexls_lse_t h, int has_fixed, int type, size_t resident_lds)
    {
        if (!h || type < 0 || type > 9 || hipSetDevice(h->device) != hipSuccess) return 0;
        DispatchQuery q;
        const KernelId id = plan_resident_fused(h, has_fixed != 0, (uint32_t)type, q);
        if (id == KernelId::none) return 0;
        uint32_t reg_cfg = 0;
        const size_t share = type != 0 ? wave_reg_lds_share() : 0;
        const size_t lds   = !lsi_fused_is_64x16(id) ? lsi_fused_lds_bytes<41, 12>(h->nVar, h->nObj, h->cap, (uint32_t)type, share, resident_lds, reg_cfg)
                                                          : lsi_fused_lds_bytes<64, 16>(h->nVar, h->nObj, h->cap, (uint32_t)type, share, resident_lds, reg_cfg);
        return lds <= kLsiFusedMaxLdsBytes ? 1 : 0;
    }

    static int upload_round(lexls_lse_t h, const void *h_in, int gather, bool trusted);
    int lexls_lse_upload_round(lexls_lse_t h, const void *h_in, int gather) { return upload_round(h, h_in, gather, false); }
    int lexls_internal_upload_round_trusted(lexls_lse_t h, const void *h_in, int gather) { return upload_round(h, h_in, gather, true); }

    static int upload_round(lexls_lse_t h, const void *h_in, int gather, bool trusted)
    {
        CHECK_HANDLE(h);
        if (!h_in) return fail(LEXLS_ERR_INVALID, "upload_round: null");
        const lexls_round_layout &L = h->lay;
        const char *in           = static_cast<const char *>(h_in);
        const uint32_t *dims     = reinterpret_cast<const uint32_t *>(in + L.dims);
        const uint32_t *nfixed   = reinterpret_cast<const uint32_t *>(in + L.nfixed);
        const uint32_t *fixedidx = reinterpret_cast<const uint32_t *>(in + L.fixed_idx);
        const uint8_t *skip      = reinterpret_cast<const uint8_t *>(in + L.skip);
        const uint32_t *row_src  = reinterpret_cast<const uint32_t *>(in + L.row_src);
        const uint32_t *row_ld   = reinterpret_cast<const uint32_t *>(in + L.row_ld);
        // the host-side checks and bookkeeping of set_obj_dim / set_fixed / gather_problem (skipped problems included: a later
        // sensitivity call may still serve them, and the kernels' LDS budget follows the largest problem of the batch)
        uint32_t max_rows = 0, max_level = 0, min_level = 0xffffffffu;
        bool any_fixed = false;
        h->level_max.assign(h->nObj, 0);
        if (gather && !h->d_cdata) return fail(LEXLS_ERR_INVALID, "upload_round: call lexls_lse_set_constraint_data first");
        for (uint32_t b = 0; b < h->batch; b++)
        {
            uint32_t m = 0;
            for (uint32_t k = 0; k < h->nObj; k++)
            {
                const uint32_t v = dims[(size_t)b * h->nObj + k];
                if (v > h->maxdim[k]) return fail(LEXLS_ERR_INVALID, "upload_round: dimension exceeds the capacity given at creation");
                m += v;
                if (v > max_level) max_level = v;
                if (v < min_level) min_level = v;
                if (v > h->level_max[k]) h->level_max[k] = v;
            }
            if (m > max_rows) max_rows = m;
            if (nfixed[b] > h->nVar) return fail(LEXLS_ERR_INVALID, "Cannot fix more than nVar variables"); // lexlse.h:1453
            any_fixed = any_fixed || nfixed[b] > 0;
            if (trusted) continue;
            for (uint32_t k = 0; k < nfixed[b]; k++)
                if (fixedidx[(size_t)b * h->nVar + k] >= h->nVar) return fail(LEXLS_ERR_INVALID, "upload_round: variable index out of range");
            if (gather && !skip[b])
                for (size_t i = (size_t)b * h->cap; i < (size_t)(b + 1) * h->cap; i++)
                {
                    const uint64_t ld = row_ld[i] & 0x7fffffffu;
                    if (ld && (uint64_t)row_src[i] + (uint64_t)(h->nVar + 1) * ld >= h->cdata_per_problem)
                        return fail(LEXLS_ERR_INVALID, "upload_round: row reference outside the constraint data");
                }
        }
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(h->d_round_in, h_in, L.in_bytes, hipMemcpyHostToDevice, h->stream));
        h->fused_gather  = false;
        h->max_rows      = max_rows ? max_rows : 1;
        h->max_level_dim = max_level;
        h->min_level_dim = min_level;
        h->dims_set      = true;
        h->has_fixed     = any_fixed;
        h->has_skip      = false; // kernels look at the mask only when some problem is masked (the one-launch-per-level large kernel needs "none")
        for (uint32_t b = 0; b < h->batch && !h->has_skip; b++) h->has_skip = skip[b] != 0;
        h->factor_valid  = false;
        if (gather)
        {
            if (int rc = lexls_internal_ensure_gather_buffer(h)) return rc;
            HIP_TRY(launch_gather_rows(h->args(), h->d_cdata, h->cdata_per_problem, h->d_row_src, h->d_row_ld, h->d_in_owned, h->stream));
            h->d_in = h->d_in_owned;
        }
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }

    int lexls_lse_download_round(lexls_lse_t h, void *h_out, void *h_types)
    {
        CHECK_HANDLE(h);
        HIP_TRY(hipSetDevice(h->device));
        const lexls_round_layout &L = h->lay;
        if (h_out) HIP_TRY(hipMemcpyAsync(h_out, h->d_round_out, L.out_bytes, hipMemcpyDeviceToHost, h->stream));
        if (h_types) HIP_TRY(hipMemcpyAsync(h_types, h->d_round_in + L.fixed_type, L.in_bytes - L.fixed_type, hipMemcpyDeviceToHost, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }

    int lexls_lse_set_problem_device(lexls_lse_t h, const double *d_lod)
    {
        CHECK_HANDLE(h);
        if (!d_lod) return fail(LEXLS_ERR_INVALID, "set_problem_device: null");
        // the kernels read doubles: no launch on a pointer that is not one's (the handle keeps what it had bound, and its factor)
        if (reinterpret_cast<uintptr_t>(d_lod) & 7u) return fail(LEXLS_ERR_INVALID, "set_problem_device: the pointer must be a multiple of 8 bytes");
        h->d_in         = d_lod;
        h->fused_gather = false;
        h->factor_valid = false;
        return LEXLS_OK;
    }

    /// Default threshold of the accuracy guard's estimate (max over pivots of |raw pivot column| / |R_jj|), calibrated by
    /// scripts/calibrate_guard.py ("Accuracy guard"): the largest estimate of 4096 well-conditioned IK problems is 13.1, the
    /// smallest of a problem whose x moves by more than 1e-11 under one-ulp changes of its data 421 — about five times either way
    static constexpr double kGuardDefaultThreshold = 64.0;

    /// opportunistic_solve: the caller only asked for the factor; kernels that produce x on the way at no extra launch do (the wave kernels
    /// always, the generic kernel on request), so that a later lexls_lse_solve of the same factor has nothing left to do
    static int run_lqr(lexls_lse_t h, bool write_factor, bool do_solve, bool opportunistic_solve = false)
    {
        CHECK_HANDLE(h);
        if (!h->d_in) return fail(LEXLS_ERR_INVALID, "no problem data: call lexls_lse_set_problem_host/device first");
        HIP_TRY(hipSetDevice(h->device));
        const LseArgs a       = h->args();
        const DispatchQuery q = query_of(h, write_factor, do_solve, opportunistic_solve);
        const KernelPlan plan = plan_lqr(q);
        const char *consumer  = "";
        LaunchExtras x;
        x.est = h->d_guard_est, x.ind = h->d_guard_ind;
        h->large_levels[0] = h->large_levels[1] = 0u;
        h->reg_cfg = 0u;
        x.reg_cfg  = &h->reg_cfg;
        if (plan.id == KernelId::large_multi)
        {
            if (!h->d_large_state) HIP_TRY(hipMalloc(&h->d_large_state, large_state_bytes(h->batch)));
            if (!h->d_norms) HIP_TRY(hipMalloc((void **)&h->d_norms, 8 * (size_t)h->batch * h->nVar));
            HIP_TRY(launch_lqr_large(a, h->level_max.data(), h->max_rows, h->d_large_state, h->d_norms, h->stream));
        }
        else if (plan.id == KernelId::large_fast)
        {
            const size_t need = large_fast_workspace_bytes(h->batch, h->nVar, h->cap, large::max_level_dim(h->level_max.data(), h->nObj));
            if (need > h->large_ws_bytes)
            {
                if (h->d_large_ws) HIP_TRY(hipFree(h->d_large_ws));
                h->d_large_ws = nullptr;
                HIP_TRY(hipMalloc(&h->d_large_ws, need));
                h->large_ws_bytes = need;
            }
            HIP_TRY(launch_lqr_large_fast(a, h->level_max.data(), h->max_rows, h->d_large_ws, h->stream, h->large_levels));
        }
        else if (plan.id == KernelId::none || plan.id >= KernelId::generic_64_lds)
            HIP_TRY(launch_lqr_generic(a, h->max_rows, plan.id, write_factor, plan.solves_x, h->stream));
        else
            HIP_TRY(launch_kernel(plan.id, a, h->stream, x));
        if (plan.needs_solve_launch) HIP_TRY(launch_solve_generic(a, h->stream, plan.reciprocal_solve, &consumer));
        h->guard_last = q.guard;
        if (q.guard)
        {
            if (plan.estimating) // flags -> status (and the list), then the bit-exact re-solve of the flagged problems: all in the stream
            {
                HIP_TRY(launch_guard_compact(h->d_guard_est, h->d_guard_status, h->d_guard_ind, h->batch, h->guard_threshold, h->guard_mode, h->stream));
                if (h->guard_mode == 2) HIP_TRY(launch_kernel(plan_guard_resolve(q), a, h->stream, x));
            }
            else if (a.skip) // a bit-exact kernel solved the problems the mask leaves: status 0, no estimate; a skipped problem keeps its report
                HIP_TRY(launch_guard_clear(h->d_guard_est, h->d_guard_status, a.skip, h->batch, h->stream));
            else // a bit-exact kernel solved: status 0, no estimate
            {
                HIP_TRY(hipMemsetAsync(h->d_guard_est, 0, 8 * (size_t)h->batch, h->stream));
                HIP_TRY(hipMemsetAsync(h->d_guard_status, 0, (size_t)h->batch, h->stream));
            }
        }
        // prefix reuse: the levels handed over are consumed; the state is there for the next factorization iff this one was the register-resident
        // wave kernel keeping its factor (every other kernel ignores both pointers and factorizes everything)
        h->resume_armed     = false;
        h->resume_valid     = a.resume_state != nullptr && write_factor && h->reg_type == 0 && plan.register_resident;
        h->last_kernel      = plan.name;
        h->solve_reciprocal = plan.reciprocal_solve;
        h->last_consumer    = consumer; // (what ran on the previous factor says nothing about this one)
        h->factor_valid     = true;
        h->factor_epoch++;
        if (plan.solves_x) h->x_epoch = h->factor_epoch;
        h->factor_in_hbm = plan.factor_in_hbm;
        return LEXLS_OK;
    }

    int lexls_lse_factorize(lexls_lse_t h) { return run_lqr(h, true, false, true); }
    int lexls_lse_factorize_solve(lexls_lse_t h, int keep_factor) { return run_lqr(h, keep_factor != 0, true); }

    static int need_factor(lexls_lse_t h, const char *who)
    {
        CHECK_HANDLE(h);
        if (!h->factor_valid || !h->factor_in_hbm) return fail(LEXLS_ERR_INVALID, std::string(who) + ": needs a factorization whose factor was kept");
        return LEXLS_OK;
    }

    int lexls_lse_solve(lexls_lse_t h)
    {
        if (int rc = need_factor(h, "lexls_lse_solve")) return rc;
        if (h->x_epoch == h->factor_epoch) return LEXLS_OK; // the factorization kernel left the basic solution in place
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(launch_solve_generic(h->args(), h->stream, h->solve_reciprocal, &h->last_consumer)); // (same x as that path's factorize_solve)
        h->x_epoch = h->factor_epoch;
        return LEXLS_OK;
    }

    /// the three least-norm solves: same preparation, one launcher each; d_x then holds a least-norm solution
    static int solve_least_norm(lexls_lse_t h, const char *who, hipError_t (*launch)(const LseArgs &, hipStream_t, const char **))
    {
        if (int rc = need_factor(h, who)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        if (!h->d_scratch) HIP_TRY(hipMalloc((void **)&h->d_scratch, 8 * (size_t)h->batch * 2 * h->nVar * h->nVar));
        HIP_TRY(launch(h->args(), h->stream, &h->last_consumer));
        h->x_epoch = 0;
        return LEXLS_OK;
    }
    int lexls_lse_solve_least_norm(lexls_lse_t h) { return solve_least_norm(h, "lexls_lse_solve_least_norm", launch_leastnorm); }
    int lexls_lse_solve_least_norm_2(lexls_lse_t h) { return solve_least_norm(h, "lexls_lse_solve_least_norm_2", launch_leastnorm2); }
    int lexls_lse_solve_least_norm_3(lexls_lse_t h)
    {
        if (h && h->factor_valid && h->factor_in_hbm && h->reg_type != 1 && h->reg_type != 2 && h->reg_type != 8 && h->reg_type != 3 && h->reg_type != 7)
            return fail(LEXLS_ERR_INVALID, "lexls_lse_solve_least_norm_3: needs a factorization with a regularization type that accumulates the null-space basis (lexlse.h:1217-1221)");
        return solve_least_norm(h, "lexls_lse_solve_least_norm_3", launch_leastnorm3);
    }

    int lexls_lse_residual(lexls_lse_t h)
    {
        if (int rc = need_factor(h, "lexls_lse_residual")) return rc;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(launch_residual(h->args(), h->stream, &h->last_consumer));
        return LEXLS_OK;
    }

    static int need_wrong_sign(lexls_lse_t h)
    {
        if (h->d_wrong_sign) return LEXLS_OK;
        const size_t bytes = (size_t)h->batch * (h->nVar + h->cap);
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMalloc((void **)&h->d_wrong_sign, bytes));
        HIP_TRY(hipMemsetAsync(h->d_wrong_sign, 0, bytes, h->stream));
        return LEXLS_OK;
    }

    /// the removal search / the wrong-sign set (collect); the objective of each problem from the host (h_obj_index), one for all
    /// (obj_index_all), or the indices already on the device (resident)
    static int sensitivity(lexls_lse_t h, const char *who, const int32_t *h_obj_index, int32_t obj_index_all, bool resident, double tolW, double tolC, bool collect)
    {
        if (int rc = need_factor(h, who)) return rc;
        if (collect)
            if (int rc = need_wrong_sign(h)) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const int32_t *d_obj = resident ? h->d_objidx : nullptr;
        if (!resident && h_obj_index)
        {
            HIP_TRY(hipMemcpyAsync(h->d_objidx, h_obj_index, 4 * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
            if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
            d_obj = h->d_objidx;
        }
        else if (!resident && (obj_index_all < 0 || (uint32_t)obj_index_all >= h->nObj))
            return fail(LEXLS_ERR_INVALID, "ObjIndex >= nObj");
        HIP_TRY(launch_sensitivity(h->args(), d_obj, obj_index_all, tolW, tolC, h->stream, h->sens_scan, h->max_level_dim, collect, &h->last_consumer));
        return LEXLS_OK;
    }
    int lexls_lse_sensitivity(lexls_lse_t h, const int32_t *h_obj_index, int32_t obj_index_all, double tolW, double tolC) { return sensitivity(h, "lexls_lse_sensitivity", h_obj_index, obj_index_all, false, tolW, tolC, false); }
    int lexls_lse_sensitivity_resident(lexls_lse_t h, double tolW, double tolC) { return sensitivity(h, "lexls_lse_sensitivity_resident", nullptr, 0, true, tolW, tolC, false); }
    int lexls_lse_sensitivity_collect(lexls_lse_t h, const int32_t *h_obj_index, int32_t obj_index_all, double tolW, double tolC) { return sensitivity(h, "lexls_lse_sensitivity_collect", h_obj_index, obj_index_all, false, tolW, tolC, true); }
    int lexls_lse_sensitivity_collect_resident(lexls_lse_t h, double tolW, double tolC) { return sensitivity(h, "lexls_lse_sensitivity_collect_resident", nullptr, 0, true, tolW, tolC, true); }

    int lexls_lse_set_sensitivity_scan(lexls_lse_t h, int on)
    {
        CHECK_HANDLE(h);
        h->sens_scan = on != 0;
        return LEXLS_OK;
    }

    int lexls_lse_multipliers(lexls_lse_t h)
    {
        if (int rc = need_factor(h, "lexls_lse_multipliers")) return rc;
        HIP_TRY(hipSetDevice(h->device));
        const LseArgs a = h->args();
        if (!h->d_mult) HIP_TRY(hipMalloc((void **)&h->d_mult, 8 * (size_t)h->batch * h->nObj * (h->nVar + h->cap)));
        if (!multipliers_sweep_serves(a, h->max_level_dim) && !h->d_mult_scratch) HIP_TRY(hipMalloc(&h->d_mult_scratch, multipliers_scratch_bytes(a)));
        HIP_TRY(launch_multipliers(a, h->d_mult, h->max_level_dim, h->stream, h->d_mult_scratch, &h->mult_swept, &h->last_consumer));
        h->mult_valid = true;
        h->mult_epoch = h->factor_epoch;
        return LEXLS_OK;
    }

    int lexls_internal_kernel_policy(lexls_lse_t h) { return h ? (int)h->policy : 0; }

    const double *lexls_internal_multipliers(lexls_lse_t h, int *swept)
    {
        if (swept) *swept = (h && h->mult_swept) ? 1 : 0;
        return (h && h->mult_valid) ? h->d_mult : nullptr;
    }

    static int download(lexls_lse_t h, void *dst, const void *src, size_t bytes)
    {
        CHECK_HANDLE(h);
        if (!dst) return fail(LEXLS_ERR_INVALID, "null output pointer");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }

    int lexls_lse_get_x(lexls_lse_t h, double *h_x) { return h ? download(h, h_x, h->d_x, 8 * (size_t)h->batch * h->nVar) : fail(LEXLS_ERR_INVALID, "null handle"); }
    int lexls_lse_get_factor(lexls_lse_t h, double *h_lod)
    {
        if (int rc = need_factor(h, "lexls_lse_get_factor")) return rc;
        return download(h, h_lod, h->d_fac, 8 * (size_t)h->batch * h->problem_elems());
    }
    int lexls_lse_get_hh_scalars(lexls_lse_t h, double *h_hh) { return h ? download(h, h_hh, h->d_hh, 8 * (size_t)h->batch * h->cap) : fail(LEXLS_ERR_INVALID, "null handle"); }
    int lexls_lse_get_permutation(lexls_lse_t h, uint32_t *h_perm)
    {
        return h ? download(h, h_perm, h->d_perm, 4 * (size_t)h->batch * h->nVar) : fail(LEXLS_ERR_INVALID, "null handle");
    }
    int lexls_lse_get_ranks(lexls_lse_t h, uint32_t *h_rank, uint32_t *h_first_col, uint32_t *h_total_rank)
    {
        CHECK_HANDLE(h);
        int rc = LEXLS_OK;
        if (h_rank) rc = download(h, h_rank, h->d_rank, 4 * (size_t)h->batch * h->nObj);
        if (!rc && h_first_col) rc = download(h, h_first_col, h->d_fcol, 4 * (size_t)h->batch * h->nObj);
        if (!rc && h_total_rank) rc = download(h, h_total_rank, h->d_totalrank, 4 * (size_t)h->batch);
        return rc;
    }
    int lexls_lse_get_mu(lexls_lse_t h, double *h_x_mu, double *h_x_mu_rhs, double *h_residual_mu)
    {
        CHECK_HANDLE(h);
        if (h->reg_type != 7 || !h->d_reg_mu) return fail(LEXLS_ERR_INVALID, "lexls_lse_get_mu: X_mu / X_mu_rhs / residual_mu exist with REGULARIZATION_TIKHONOV_1 (7) only");
        HIP_TRY(hipSetDevice(h->device));
        const size_t n = h->nVar, nObj = h->nObj, cap = h->cap, per = reg_mu_doubles(h->nVar, h->nObj, h->cap);
        if (h_x_mu) HIP_TRY(hipMemcpy2DAsync(h_x_mu, 8 * nObj * n, h->d_reg_mu, 8 * per, 8 * nObj * n, h->batch, hipMemcpyDeviceToHost, h->stream));
        if (h_x_mu_rhs) HIP_TRY(hipMemcpy2DAsync(h_x_mu_rhs, 8 * nObj * n, h->d_reg_mu + nObj * n, 8 * per, 8 * nObj * n, h->batch, hipMemcpyDeviceToHost, h->stream));
        if (h_residual_mu) HIP_TRY(hipMemcpy2DAsync(h_residual_mu, 8 * cap, h->d_reg_mu + 2 * nObj * n, 8 * per, 8 * cap, h->batch, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return LEXLS_OK;
    }
    int lexls_lse_get_v(lexls_lse_t h, double *h_v) { return h ? download(h, h_v, h->d_v, 8 * (size_t)h->batch * h->cap) : fail(LEXLS_ERR_INVALID, "null handle"); }
    int lexls_lse_get_lambda(lexls_lse_t h, double *h_lambda)
    {
        return h ? download(h, h_lambda, h->d_lambda, 8 * (size_t)h->batch * (h->nVar + h->cap)) : fail(LEXLS_ERR_INVALID, "null handle");
    }
    int lexls_lse_get_multipliers(lexls_lse_t h, double *h_L)
    {
        CHECK_HANDLE(h);
        if (!h->mult_valid) return fail(LEXLS_ERR_INVALID, "lexls_lse_get_multipliers: call lexls_lse_multipliers first");
        if (!h->factor_valid || h->mult_epoch != h->factor_epoch)
            return fail(LEXLS_ERR_INVALID, "lexls_lse_get_multipliers: the problem or its factorization changed since lexls_lse_multipliers (call it again)");
        return download(h, h_L, h->d_mult, 8 * (size_t)h->batch * h->nObj * (h->nVar + h->cap));
    }
    int lexls_lse_get_sensitivity(lexls_lse_t h, int32_t *h_found_ctr_obj, double *h_max_abs)
    {
        CHECK_HANDLE(h);
        int rc = LEXLS_OK;
        if (h_found_ctr_obj) rc = download(h, h_found_ctr_obj, h->d_sens, 4 * (size_t)h->batch * 3);
        if (!rc && h_max_abs) rc = download(h, h_max_abs, h->d_maxabs, 8 * (size_t)h->batch);
        return rc;
    }
    int lexls_lse_get_wrong_sign(lexls_lse_t h, uint8_t *h_mask)
    {
        CHECK_HANDLE(h);
        if (!h->d_wrong_sign) return fail(LEXLS_ERR_INVALID, "lexls_lse_get_wrong_sign: call lexls_lse_sensitivity_collect first");
        return download(h, h_mask, h->d_wrong_sign, (size_t)h->batch * (h->nVar + h->cap));
    }
    int lexls_lse_get_fixed_type(lexls_lse_t h, uint8_t *h_types) { return h ? download(h, h_types, h->d_fixed_type, (size_t)h->batch * h->nVar) : fail(LEXLS_ERR_INVALID, "null handle"); }
    int lexls_lse_get_ctr_type(lexls_lse_t h, uint8_t *h_types) { return h ? download(h, h_types, h->d_ctr_type, (size_t)h->batch * h->cap) : fail(LEXLS_ERR_INVALID, "null handle"); }

    int lexls_lse_device_ptr(lexls_lse_t h, int which, void **d_ptr)
    {
        CHECK_HANDLE(h);
        if (!d_ptr) return fail(LEXLS_ERR_INVALID, "null output pointer");
        switch (which)
        {
        case LEXLS_ARRAY_X: *d_ptr = h->d_x; break;
        case LEXLS_ARRAY_FACTOR: *d_ptr = h->d_fac; break;
        case LEXLS_ARRAY_HH: *d_ptr = h->d_hh; break;
        case LEXLS_ARRAY_PERM: *d_ptr = h->d_perm; break;
        case LEXLS_ARRAY_RANK: *d_ptr = h->d_rank; break;
        case LEXLS_ARRAY_FIRST_COL: *d_ptr = h->d_fcol; break;
        case LEXLS_ARRAY_TOTAL_RANK: *d_ptr = h->d_totalrank; break;
        case LEXLS_ARRAY_V: *d_ptr = h->d_v; break;
        case LEXLS_ARRAY_LAMBDA: *d_ptr = h->d_lambda; break;
        case LEXLS_ARRAY_GUARD_ESTIMATE:
        case LEXLS_ARRAY_GUARD_STATUS:
            if (!h->d_guard_est) return fail(LEXLS_ERR_INVALID, "lexls_lse_device_ptr: the accuracy guard has not been switched on (lexls_lse_set_accuracy_guard)");
            *d_ptr = which == LEXLS_ARRAY_GUARD_ESTIMATE ? (void *)h->d_guard_est : (void *)h->d_guard_status;
            break;
        case LEXLS_ARRAY_MULTIPLIERS:
            if (!h->d_mult)
            {
                HIP_TRY(hipSetDevice(h->device));
                HIP_TRY(hipMalloc((void **)&h->d_mult, 8 * (size_t)h->batch * h->nObj * (h->nVar + h->cap)));
            }
            *d_ptr = h->d_mult;
            break;
        case LEXLS_ARRAY_WRONG_SIGN:
            if (int rc = need_wrong_sign(h)) return rc;
            *d_ptr = h->d_wrong_sign;
            break;
        case LEXLS_ARRAY_INPUT:
            if (!h->d_in_owned)
            {
                HIP_TRY(hipSetDevice(h->device));
                HIP_TRY(hipMalloc((void **)&h->d_in_owned, 8 * (size_t)h->batch * h->problem_elems()));
            }
            *d_ptr  = h->d_in_owned;
            h->d_in = h->d_in_owned;
            h->fused_gather = false;
            break;
        default: return fail(LEXLS_ERR_INVALID, "unknown array id");
        }
        return LEXLS_OK;
    }

    const char *lexls_lse_last_kernel(lexls_lse_t h) { return h ? h->last_kernel : ""; }

    int lexls_lse_last_consumer_kernel(lexls_lse_t h, char *buf, size_t len)
    {
        CHECK_HANDLE(h);
        if (!buf || len == 0) return fail(LEXLS_ERR_INVALID, "lexls_lse_last_consumer_kernel: no buffer");
        std::snprintf(buf, len, "%s", h->last_consumer);
        return LEXLS_OK;
    }

    int lexls_lse_last_reg_placement(lexls_lse_t h, uint32_t *window_order, uint32_t *basis_in_lds)
    {
        CHECK_HANDLE(h);
        if (!window_order || !basis_in_lds) return fail(LEXLS_ERR_INVALID, "lexls_lse_last_reg_placement: no output");
        *window_order = h->reg_cfg & 0xffu;
        *basis_in_lds = (h->reg_cfg >> 8) & 1u;
        return LEXLS_OK;
    }

    int lexls_lse_last_large_levels(lexls_lse_t h, uint32_t *in_launch, uint32_t *redone)
    {
        CHECK_HANDLE(h);
        if (!in_launch || !redone) return fail(LEXLS_ERR_INVALID, "lexls_lse_last_large_levels: no output");
        *in_launch = h->large_levels[0];
        *redone    = h->large_levels[1];
        return LEXLS_OK;
    }

    int lexls_lse_set_accuracy_guard(lexls_lse_t h, int mode, double threshold)
    {
        CHECK_HANDLE(h);
        if (mode < 0 || mode > 2) return fail(LEXLS_ERR_INVALID, "lexls_lse_set_accuracy_guard: mode must be 0, 1 or 2");
        if (mode != 0 && !h->d_guard_est)
        {
            HIP_TRY(hipSetDevice(h->device));
            HIP_TRY(hipMalloc((void **)&h->d_guard_est, 8 * (size_t)h->batch));
            HIP_TRY(hipMalloc((void **)&h->d_guard_status, (size_t)h->batch));
            HIP_TRY(hipMalloc((void **)&h->d_guard_ind, 4 * (1 + (size_t)h->batch)));
            HIP_TRY(hipMemsetAsync(h->d_guard_est, 0, 8 * (size_t)h->batch, h->stream));
            HIP_TRY(hipMemsetAsync(h->d_guard_status, 0, (size_t)h->batch, h->stream));
            HIP_TRY(hipMemsetAsync(h->d_guard_ind, 0, 4 * (1 + (size_t)h->batch), h->stream));
            if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        }
        h->guard_mode      = mode;
        h->guard_threshold = threshold > 0.0 ? threshold : kGuardDefaultThreshold; // (NaN: the default as well)
        return LEXLS_OK;
    }

    int lexls_lse_get_accuracy(lexls_lse_t h, double *h_estimate, uint8_t *h_status, uint32_t *h_flagged)
    {
        CHECK_HANDLE(h);
        const size_t B = h->batch;
        if (!h->d_guard_est || !h->guard_last) // the last solve ran without the guard: nothing to report
        {
            if (h_estimate) std::memset(h_estimate, 0, 8 * B);
            if (h_status) std::memset(h_status, 0, B);
            if (h_flagged) *h_flagged = 0;
            return LEXLS_OK;
        }
        HIP_TRY(hipSetDevice(h->device));
        std::vector<uint8_t> own;
        uint8_t *st = h_status;
        if (!st && h_flagged)
        {
            own.resize(B);
            st = own.data();
        }
        if (h_estimate) HIP_TRY(hipMemcpyAsync(h_estimate, h->d_guard_est, 8 * B, hipMemcpyDeviceToHost, h->stream));
        if (st) HIP_TRY(hipMemcpyAsync(st, h->d_guard_status, B, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream)); // (also under deferred sync: the count is made on the host)
        if (h_flagged)
        {
            uint32_t c = 0;
            for (size_t b = 0; b < B; b++) c += st[b] >= 2 ? 1u : 0u;
            *h_flagged = c;
        }
        return LEXLS_OK;
    }

    int lexls_lse_set_prefix_reuse(lexls_lse_t h, int enable)
    {
        CHECK_HANDLE(h);
        HIP_TRY(hipSetDevice(h->device));
        if (enable && !h->d_resume_state)
        {
            HIP_TRY(hipMalloc((void **)&h->d_resume_state, (size_t)h->batch * resume_state_bytes(h->nObj)));
            HIP_TRY(hipMalloc((void **)&h->d_resume_level, 4 * (size_t)h->batch));
            HIP_TRY(hipMemsetAsync(h->d_resume_level, 0, 4 * (size_t)h->batch, h->stream));
        }
        h->resume_enabled = enable != 0;
        h->resume_valid   = false;
        h->resume_armed   = false;
        return LEXLS_OK;
    }
    int lexls_lse_prefix_reuse_ready(lexls_lse_t h) { return (h && h->resume_enabled && h->resume_valid) ? 1 : 0; }
    int lexls_lse_set_resume_levels(lexls_lse_t h, const int32_t *h_levels)
    {
        CHECK_HANDLE(h);
        if (!h->resume_enabled) return fail(LEXLS_ERR_INVALID, "set_resume_levels: lexls_lse_set_prefix_reuse(h, 1) first");
        if (!h_levels) return fail(LEXLS_ERR_INVALID, "set_resume_levels: levels is NULL");
        if (!h->resume_valid) return fail(LEXLS_ERR_INVALID, "set_resume_levels: the last factorization left nothing to resume from (another kernel, no factor kept, or none yet)");
        for (uint32_t b = 0; b < h->batch; b++)
            if (h_levels[b] < 0 || (uint32_t)h_levels[b] > h->nObj) return fail(LEXLS_ERR_INVALID, "set_resume_levels: a level is outside 0 .. nObj");
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpyAsync(h->d_resume_level, h_levels, 4 * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
        if (!h->deferred_sync) HIP_TRY(hipStreamSynchronize(h->stream));
        h->resume_armed = true;
        return LEXLS_OK;
    }
    int32_t *lexls_internal_resume_levels(lexls_lse_t h) { return (h && h->resume_enabled && h->reg_type == 0) ? h->d_resume_level : nullptr; }
    void lexls_internal_arm_resume(lexls_lse_t h)
    {
        if (h && h->resume_enabled) h->resume_armed = true;
    }

    int lexls_lse_set_kernel_policy(lexls_lse_t h, int policy)
    {
        CHECK_HANDLE(h);
        if (policy != (int)h->policy) HIP_TRY(materialize_fused_gather(h)); // another kernel may read `in`: the rows named by the round must be there
        h->policy = static_cast<KernelPolicy>(policy);
        return LEXLS_OK;
    }
}

#include "lse_kept_capi.h" // the calls that work on a kept factor beyond the solves above: the adjoints, the tangents, new right-hand sides
