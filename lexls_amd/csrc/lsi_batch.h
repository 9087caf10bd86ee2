// The lock-step LexLSI batch object: B host driver instances (include/lexls/lexlsi.h) over the equality-solver handles of a few groups (lsi_batch_ctx.h).
#pragma once
#include <lexls/lsi_runner.h>
#include <memory>
#include <thread>
#include "lsi_slot.h"
#include "lsi_final.h"

namespace
{
    /// One problem through the single-problem driver (every equality problem on the device, the removal search of an iteration in one
    /// device call); `lsi` is left solved for what the caller reads next.
    runner::LsiInfo solve_one(internal::LexLSI &lsi, int device, const runner::LsiProblem &p, const ParametersLexLSI &par, double *h_x, int32_t *h_info6, uint8_t *h_active, double *h_v)
    {
        lsi.getLexLSE().setDevice(device);
        lsi.getLexLSE().setSensitivityScan(true);
        lsi.setSensitivityScansAllLevels(true);
        runner::setup(lsi, p, par);
        lsi.solve();
        runner::LsiInfo info;
        runner::collect(lsi, p, h_x, &info, h_active, h_v);
        if (h_info6) std::memcpy(h_info6, &info, sizeof(info));
        return info;
    }

    /// lexls_lsi_batch_set_instance_regularization with the factors in device memory, for one group: row i of the group's handle array (B x nObjL,
    /// what the regularized kernels read) takes the factors of the caller's row i (B x nObj, the group's first instance in front): LexLSE level k
    /// = objective off + k.  One thread per (instance, level).
    __global__ __launch_bounds__(256) void lsi_instance_factors_kernel(const double *__restrict__ factors, uint32_t B, uint32_t nObj, uint32_t nObjL, uint32_t off,
                                                                      double *__restrict__ out)
    {
        const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= B * nObjL) return;
        const uint32_t i = t / nObjL, k = t - i * nObjL;
        out[t] = factors[(size_t)i * nObj + off + k];
    }

    /// lexls_lsi_batch_enqueue_device with h_reg_factors: the factors of the LexLSE levels travel in the launch itself (nothing of the host is read
    /// after the call returns; a captured launch keeps the capturing call's), every row of the group's handle array (B x nObjL) takes them
    struct LevelFactors
    {
        double f[STEP_MAX_OBJ];
    };
    __global__ __launch_bounds__(256) void lsi_level_factors_kernel(LevelFactors lf, uint32_t B, uint32_t nObjL, double *__restrict__ out)
    {
        const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= B * nObjL) return;
        out[t] = lf.f[t % nObjL];
    }
} // namespace

/// A lock-step batch that outlives one solve (the reference constructs a LexLSI once and feeds it successive problems, lexlsi.h:56-112):
/// device buffers, pinned blocks, streams and the worker pool are made once; every run() re-reads the problem data.
struct lexls_lsi_batch_s : LsiBatchShape
{
    LsiFinal fin{*this}; // what follows a run: its working sets, get_lambda and the gradient calls (lsi_final.h)
    bool resident_ok = false;
    bool resident_shape = false; // resident_ok but for the environment's switches: the structure has resident iterations at all
    // ---- lexls_lsi_batch_set_instance_regularization: batch x nObj factors that stand for h_reg_factors in every regularized run while set ----
    enum : int { INST_NONE = 0, INST_HOST = 1, INST_DEVICE = 2 };
    int inst_mode = INST_NONE;
    std::vector<double> inst_factors;     // INST_HOST: the copy taken at the call
    const double *d_inst_factors = NULL;  // INST_DEVICE: the caller's array, read in the groups' streams at the start of every run
    // ---- lexls_lsi_batch_set_instance_max_factorizations: batch int32 in device memory, the caller's; read by the setup kernel of every device run while set ----
    const int32_t *d_limits = NULL;
    const int32_t *group_limits(uint32_t g) const { return d_limits ? d_limits + lo[g] : NULL; }
    // ---- lexls_lsi_batch_set_instance_obj_dims: batch x nObj uint32 in device memory, the caller's; read by the setup kernel of every device run while set ----
    const uint32_t *d_obj_dims = NULL;
    const uint32_t *group_obj_dims(uint32_t g) const { return d_obj_dims ? d_obj_dims + (size_t)lo[g] * nObj : NULL; }
    double t_create = 0.0;
    int32_t last_stats[4] = {0, 0, 0, 0}; // of the last run: factorize+solve stages, sensitivity stages, stages with the step on the device, groups
    const char *last_kernel = ""; // lexls_lsi_batch_last_kernel: what served the resident iterations of the last run ("host": nothing did)
    std::vector<uint32_t> cycling_count; // batch: LexLSI::getCyclingCounter() of every instance of the last run (lexls_lsi_batch_get_cycling_counters)
    // ---- the working-set log of the last run (lexls_lsi_batch_set_working_set_log; LexLSI::getWorkingSetLog, lexlsi.h:739) ----
    // One slab for the batch, on the device and as a pinned staging copy: batch x cap records, batch x cap values, batch counters; group g works on
    // the rows from lo[g] on (BatchCtx::bind_working_set_log), so the caller of lexls_lsi_batch_working_set_log_device sees one array per part.
    // The device copy is the log: resident iterations write it where they happen, what host objects logged is uploaded into it.
    struct WlogBufs
    {
        uint32_t cap = 0;
        int32_t *d_log    = NULL;
        double *d_alpha   = NULL;
        uint32_t *d_count = NULL;
        Pinned<int32_t> log;
        Pinned<double> alpha;
        Pinned<uint32_t> count;
        ~WlogBufs()
        {
            if (d_log) (void)hipFree(d_log);
            if (d_alpha) (void)hipFree(d_alpha);
            if (d_count) (void)hipFree(d_count);
        }
    };
    std::unique_ptr<WlogBufs> wlog;      // NULL: logging is off
    bool wlog_valid = false;             // the slab describes the last run (which ran with logging on and did not fail)
    std::vector<uint8_t> wlog_from_host; // batch: this run's entries of the instance are all its host object's (it never became resident)

    // ---- lexls_lsi_batch_enqueue_device / lexls_lsi_batch_finish: what the stream-ordered run keeps between the two calls ----
    struct Async
    {
        uint32_t *d_fault = NULL;      // the fault word of the run (every group's setup kernel takes its minimum into it)
        Pinned<uint32_t> fault_host;
        hipEvent_t ev_fork = NULL;     // the caller's stream at the start of the run: the groups' streams wait for it
        double *d_inst = NULL;         // INST_HOST factors on the device (batch x nObj) ...
        Pinned<double> inst_stage;     // ... and the pinned copy they are uploaded from, when they have changed (inst_uploaded != inst_gen)
        uint64_t inst_uploaded = 0;
        bool pending = false;          // an enqueue without its finish
        bool enqueued = false;         // there has been an enqueue (finish may be called again behind every replay of a captured one)
        hipStream_t stream = NULL;     // of the last enqueue
        ParametersLexLSI par;          // of the last enqueue
        ~Async()
        {
            if (d_fault) (void)hipFree(d_fault);
            if (d_inst) (void)hipFree(d_inst);
            if (ev_fork) (void)hipEventDestroy(ev_fork);
        }
    };
    std::unique_ptr<Async> async;
    uint64_t inst_gen = 1; // counts the calls of lexls_lsi_batch_set_instance_regularization with host factors
    bool pending() const { return async && async->pending; }
    /// what every synchronous entry point and host getter answers between an enqueue and its finish
    void refuse_pending(const char *who) const
    {
        if (pending()) throw Exception(std::string(who) + ": a lexls_lsi_batch_enqueue_device run of this batch is waiting for lexls_lsi_batch_finish");
    }

    /// what a group's next stage must serve (Run::wants): somebody alive, a factorize+solve, a sensitivity, a device-side step, a solve whose x the host needs
    enum : uint32_t { WANT_ALIVE = 1u, WANT_FS = 2u, WANT_SENS = 4u, WANT_STEP = 8u, WANT_X = 16u };

    /// What the phases of ONE run() share.  It lives on run()'s stack: between two runs the batch object keeps the statistics of the last
    /// one and the working sets get_lambda needs, nothing else.
    struct Run
    {
        const double *h_data, *h_x0, *h_v0, *h_reg_factors;
        const uint32_t *h_var_index;
        const uint8_t *h_active_guess;
        const ParametersLexLSI &par;
        double *h_x, *h_v;
        int32_t *h_info6, *h_rounds2;
        uint8_t *h_active;
        const RunSwitches sw;
        bool gather = false, resident = false, step = false; // of this run: rows gathered on the device, resident iterations, device-side step
        std::vector<SlotStep> hooks; // (before the instances that point to them)
        std::vector<std::unique_ptr<SlotLSI>> lsi;
        std::vector<runner::LsiProblem> prob;
        std::vector<std::atomic<uint32_t>> wants; // per group: WANT_* of the next stage
        double t_begin = 0.0, t_ctx = 0.0, t_setup = 0.0, t_host = 0.0;
        const double *inst_rows = NULL, *d_inst_rows = NULL; // per-instance factors of this run (batch x nObj; host copy / caller's device array) or NULL
    };

    lexls_lsi_batch_s(int device_, uint32_t batch_, uint32_t nVar_, uint32_t nObj_, const uint32_t *h_dims, const int32_t *h_types)
    : LsiBatchShape(device_, batch_, nVar_, nObj_)
    {
        if (batch == 0 || nObj == 0) throw Exception("lexls_lsi_batch_solve: empty batch");
        dims.assign(h_dims, h_dims + nObj);
        types.assign(h_types, h_types + nObj);
        off = (h_types[0] == 1) ? 1 : 0;
        if (nObj - off == 0) throw Exception("Problems consisting of one level of simple bounds are not supported."); // lexlsi.cpp:417
        for (uint32_t k = 0; k < nObj; k++)
        {
            per_data += objective_elems(h_dims[k], h_types[k], nVar);
            total += h_dims[k];
        }
        cycling_count.assign(batch, 0u);
        const double t_begin = BatchCtx::now();
        const CreateSwitches sw;
        // The instances can be split into groups that take turns: while one group's stage runs on the GPU (its own stream), the host
        // advances the active-set logic of the other one.  Every stage carries fixed costs (one copy each way, launches, one
        // synchronisation) that a split multiplies, so it pays for large batches only.  Measured on MI355X, cold
        // solve of n = 40, 5 x 12, seconds with 1 / 2 / 3 groups: 512 instances 0.034 / 0.030 / 0.040; 1024: 0.039 / 0.034 / 0.045
        // (256 instances, an earlier state of the driver: 0.044 / 0.047).  LEXLS_LSI_GROUPS overrides the number.
        // (With resident iterations — the default, see below — there is no host work per stage left to overlap: one group.)
        nGroups = ((!sw.resident || sw.device_step) && batch >= 512) ? 2u : 1u;
        if (sw.groups) nGroups = std::max(1, std::atoi(sw.groups));
        nGroups = std::min(nGroups, batch);
        gather = per_data < 0x7fffffffull && !sw.host_staging; // (LEXLS_LSI_HOST_STAGING, a diagnostic switch: assemble on the host, stage over PCIe)
        grp.resize(nGroups);
        fin.create();
        lo.assign(nGroups + 1, 0);
        for (uint32_t g = 0; g < nGroups; g++) lo[g + 1] = lo[g] + batch / nGroups + (g < batch % nGroups ? 1u : 0u);
        for (uint32_t g = 0; g < nGroups; g++)
        {
            grp[g].reset(new BatchCtx());
            BatchCtx &ctx = *grp[g];
            ctx.create(device, lo[g + 1] - lo[g], nVar, nObj - off, h_dims + off, gather, sw.prefix_reuse);
            hip_check(lexls_lse_set_deferred_sync(ctx.h, 1)); // every per-round array of BatchCtx is pinned and only touched between stages
            hip_check(lexls_lse_set_sensitivity_scan(ctx.h, 1)); // the removal search of an iteration in ONE sensitivity stage (all its levels)
            // The removal search runs speculatively behind every factorization (a third fewer stages: one synchronisation per active-set
            // iteration instead of two).  With round 1's 83-us level-by-level search it lost (1024 instances cold 0.040 s vs 0.036 s); since the
            // search is one 36-us sweep (sensitivity_sweep_kernel) it wins: warm-started ~30 iterations 0.027-0.028 s vs 0.029-0.034 s.
            // LEXLS_LSI_SPECULATIVE_SENS=0 restores the two-stage form.
            ctx.spec_sens = sw.spec_sens;
        }
        // the step of an iteration can run on the device when the constraint data is resident
        StepShape sh;
        std::memset(&sh, 0, sizeof(sh));
        sh.n = nVar, sh.nObj = nObj, sh.total = (uint32_t)total, sh.SD = nVar + 2 * (uint32_t)total, sh.per_data = per_data, sh.dim0 = off ? h_dims[0] : 0;
        const uint64_t elems = nObj <= STEP_MAX_OBJ ? fill_shape(sh, h_dims, h_types, nVar) : 0;
        // Off by default: measured on MI355X (scripts/lsi_ab.sh; 1024 / 4096 instances of n = 40, 5 x 12) it is a wash — cold 0.052 s
        // vs 0.049 s at 1024, 0.117 s vs 0.120 s at 4096: the host's share of a stage is parallel and small, the extra copy + kernel +
        // copy of a stage is not free.  LEXLS_LSI_DEVICE_STEP=1 turns it on.
        bool step_ok = sw.device_step && gather && nObj <= STEP_MAX_OBJ && 8 * (size_t)sh.SD * 4 <= 48 * 1024;
        for (uint32_t k = 0; k < nObj && step_ok; k++) step_ok = h_dims[k] <= 65535;
        if (step_ok)
            for (uint32_t g = 0; g < nGroups; g++) grp[g]->create_step(sh);
        // Resident iterations (lsi_iterate_kernel), the default where the structure allows it: after phase 1 the instances leave the host —
        // a stage is row gather + l-QR + removal sweep + step / working-set change / next problem, all enqueued, and the host only polls
        // how many instances have stopped.  LEXLS_LSI_RESIDENT=0 keeps the active-set logic on the host (one synchronisation per stage).
        resident_ok = sw.resident && !step_ok && gather && nObj <= STEP_MAX_OBJ && 4 * resident_lds_per_wave(sh.SD, (uint32_t)total) <= 48 * 1024 && total <= 65535 && elems <= 0xffffffffull;
        for (uint32_t k = 1; k < nObj && resident_ok; k++) resident_ok = h_types[k] != 1; // (the driver itself only takes a simple-bounds objective first, lexlsi.h:402-405)
        resident_shape = per_data < 0x7fffffffull && nObj <= STEP_MAX_OBJ && 4 * resident_lds_per_wave(sh.SD, (uint32_t)total) <= 48 * 1024 && total <= 65535 && elems <= 0xffffffffull;
        for (uint32_t k = 1; k < nObj && resident_shape; k++) resident_shape = h_types[k] != 1;
        if (resident_ok)
            for (uint32_t g = 0; g < nGroups; g++) grp[g]->create_resident(sh, off);
        group_of.resize(batch);
        for (uint32_t g = 0; g < nGroups; g++)
            for (uint32_t b = lo[g]; b < lo[g + 1]; b++) group_of[b] = g;
        pool.reset(new WorkerPool(WorkerPool::default_workers(batch), sw.pool_spin_seconds));
        t_create = BatchCtx::now() - t_begin;
    }

    /// LexLSI::getCyclingCounter() of every instance of the last run, whichever path served it
    int get_cycling_counters(uint32_t *h_counts) const
    {
        if (!fin.ran()) throw Exception("lexls_lsi_batch_get_cycling_counters: no completed lexls_lsi_batch_run on this batch");
        if (!h_counts) throw Exception("lexls_lsi_batch_get_cycling_counters: null output");
        std::copy(cycling_count.begin(), cycling_count.end(), h_counts);
        return LEXLS_OK;
    }

    /// lexls_lsi_batch_set_working_set_log: max_entries records per instance for every later run; 0: off, the slab is freed
    int set_working_set_log(uint32_t max_entries)
    {
        wlog_valid = false;
        for (uint32_t g = 0; g < nGroups; g++) grp[g]->bind_working_set_log(0, NULL, NULL, NULL, NULL, NULL, NULL);
        wlog.reset();
        if (max_entries == 0) return LEXLS_OK;
        std::unique_ptr<WlogBufs> w(new WlogBufs());
        w->cap            = max_entries;
        const size_t rows = (size_t)batch * max_entries;
        if (hipSetDevice(device) != hipSuccess || hipMalloc((void **)&w->d_log, 4 * rows * RESIDENT_WLOG_FIELDS) != hipSuccess || hipMalloc((void **)&w->d_alpha, 8 * rows) != hipSuccess ||
            hipMalloc((void **)&w->d_count, 4 * (size_t)batch) != hipSuccess)
            throw Exception("hipMalloc failed (lexls_lsi_batch_set_working_set_log)");
        w->log.assign(rows * RESIDENT_WLOG_FIELDS, 0);
        w->alpha.assign(rows, 0.0);
        w->count.assign(batch, 0u);
        wlog_from_host.assign(batch, 0);
        wlog = std::move(w);
        for (uint32_t g = 0; g < nGroups; g++)
        {
            const size_t r0 = (size_t)lo[g] * max_entries;
            grp[g]->bind_working_set_log(max_entries, wlog->d_log + r0 * RESIDENT_WLOG_FIELDS, wlog->d_alpha + r0, wlog->d_count + lo[g], wlog->log.data() + r0 * RESIDENT_WLOG_FIELDS,
                                         wlog->alpha.data() + r0, wlog->count.data() + lo[g]);
        }
        return LEXLS_OK;
    }
    /// a run starts: the staging copy is empty (the groups clear their device rows in their streams, prepare_groups)
    void begin_working_set_log()
    {
        wlog_valid = false;
        if (!wlog) return;
        std::fill(wlog->log.begin(), wlog->log.end(), 0);
        std::fill(wlog->alpha.begin(), wlog->alpha.end(), 0.0);
        std::fill(wlog->count.begin(), wlog->count.end(), 0u);
        std::fill(wlog_from_host.begin(), wlog_from_host.end(), 0);
    }
    /// instance b never left the host (host path, one-by-one path, or it stopped before the hand-over): its rows are its host object's log
    template <class LSI>
    void keep_host_log(uint32_t b, const LSI &inst)
    {
        if (!wlog) return;
        put_working_set_log(inst.getWorkingSetLog(), wlog->cap, b, wlog->log.data(), wlog->alpha.data(), wlog->count.data());
        wlog_from_host[b] = 1;
    }
    /// the run is over (every stream is idle): rows that host objects made are merged into the device copy, which is then complete
    void finish_working_set_log()
    {
        if (!wlog) return;
        size_t from_host = 0;
        for (uint32_t b = 0; b < batch; b++) from_host += wlog_from_host[b];
        if (from_host)
        {
            const size_t cap = wlog->cap, rows = (size_t)batch * cap;
            if (hipSetDevice(device) != hipSuccess) throw Exception("hipSetDevice failed (working-set log)");
            if (from_host < batch) // the resident instances' rows as the device left them
            {
                std::vector<int32_t> log(rows * RESIDENT_WLOG_FIELDS);
                std::vector<double> alpha(rows);
                std::vector<uint32_t> count(batch);
                if (hipMemcpy(log.data(), wlog->d_log, 4 * log.size(), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(alpha.data(), wlog->d_alpha, 8 * rows, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(count.data(), wlog->d_count, 4 * (size_t)batch, hipMemcpyDeviceToHost) != hipSuccess)
                    throw Exception("download of the working-set log failed");
                for (uint32_t b = 0; b < batch; b++)
                    if (!wlog_from_host[b])
                    {
                        std::copy(log.begin() + (size_t)b * cap * RESIDENT_WLOG_FIELDS, log.begin() + (size_t)(b + 1) * cap * RESIDENT_WLOG_FIELDS, wlog->log.begin() + (size_t)b * cap * RESIDENT_WLOG_FIELDS);
                        std::copy(alpha.begin() + (size_t)b * cap, alpha.begin() + (size_t)(b + 1) * cap, wlog->alpha.begin() + (size_t)b * cap);
                        wlog->count[b] = count[b];
                    }
            }
            if (hipMemcpy(wlog->d_log, wlog->log.data(), 4 * rows * RESIDENT_WLOG_FIELDS, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(wlog->d_alpha, wlog->alpha.data(), 8 * rows, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(wlog->d_count, wlog->count.data(), 4 * (size_t)batch, hipMemcpyHostToDevice) != hipSuccess)
                throw Exception("upload of the merged working-set log failed");
        }
        wlog_valid = true;
    }
    /// lexls_lsi_batch_get_working_set_log: the last run's log from the device copy (any pointer may be NULL)
    int get_working_set_log(int32_t *h_log, double *h_alpha, uint32_t *h_counts) const
    {
        if (!wlog) throw Exception("lexls_lsi_batch_get_working_set_log: the working-set log is off (lexls_lsi_batch_set_working_set_log)");
        if (!wlog_valid) throw Exception("lexls_lsi_batch_get_working_set_log: no completed run with the working-set log on");
        const size_t rows = (size_t)batch * wlog->cap;
        if (hipSetDevice(device) != hipSuccess || (h_log && hipMemcpy(h_log, wlog->d_log, 4 * rows * RESIDENT_WLOG_FIELDS, hipMemcpyDeviceToHost) != hipSuccess) ||
            (h_alpha && hipMemcpy(h_alpha, wlog->d_alpha, 8 * rows, hipMemcpyDeviceToHost) != hipSuccess) ||
            (h_counts && hipMemcpy(h_counts, wlog->d_count, 4 * (size_t)batch, hipMemcpyDeviceToHost) != hipSuccess))
            throw Exception("lexls_lsi_batch_get_working_set_log: download failed");
        return LEXLS_OK;
    }
    /// the parameters of a run as its host objects get them: with logging on they keep their working-set log (ParametersLexLSI::log_working_set_enabled)
    ParametersLexLSI with_log_switch(ParametersLexLSI par) const
    {
        if (wlog) par.log_working_set_enabled = true;
        return par;
    }

    runner::LsiProblem problem(const Run &r, uint32_t b) const
    {
        return {nVar, nObj, dims.data(), types.data(), r.h_data + (size_t)b * per_data, r.h_var_index ? r.h_var_index + (size_t)b * dims[0] : NULL,
                r.h_active_guess ? r.h_active_guess + (size_t)b * total : NULL, r.h_x0 ? r.h_x0 + (size_t)b * nVar : NULL, r.h_v0 ? r.h_v0 + (size_t)b * total : NULL,
                r.inst_rows ? r.inst_rows + (size_t)b * nObj : r.h_reg_factors};
    }

    /// lexls_lsi_batch_set_instance_regularization
    int set_instance_regularization(const double *factors, int in_device_memory)
    {
        if (!factors)
        {
            inst_mode      = INST_NONE;
            d_inst_factors = NULL;
            inst_factors.clear();
            return LEXLS_OK;
        }
        if (in_device_memory)
        {
            bool served = false; // some regularization type has a register-resident kernel on this shape
            for (int t = 1; t <= 9 && resident_shape && !served; t++) served = lexls_internal_resident_reg_serves(grp[0]->h, t) != 0;
            if (!served)
            {
                lexls_internal_set_error("lexls_lsi_batch_set_instance_regularization: factors in device memory need a batch whose regularized runs can be resident "
                                         "(no register-resident kernel for this shape): there is no detour over the host");
                return LEXLS_ERR_UNSUPPORTED;
            }
            inst_factors.clear();
            d_inst_factors = factors;
            inst_mode      = INST_DEVICE;
            return LEXLS_OK;
        }
        inst_factors.assign(factors, factors + (size_t)batch * nObj);
        inst_gen++;
        d_inst_factors = NULL;
        inst_mode      = INST_HOST;
        return LEXLS_OK;
    }
    /// lexls_lsi_batch_set_instance_mask: the pointer is kept (NULL: no mask); nothing is read or copied here
    int set_instance_mask(const uint8_t *d_mask_)
    {
        d_mask = d_mask_;
        return LEXLS_OK;
    }
    /// lexls_lsi_batch_set_instance_max_factorizations: the pointer is kept (NULL: no limits); nothing is read or copied here
    int set_instance_max_factorizations(const int32_t *d_limits_)
    {
        d_limits = d_limits_;
        return LEXLS_OK;
    }
    /// lexls_lsi_batch_set_instance_obj_dims: the pointer is kept (NULL: every instance has the batch's dims); nothing is read or copied here
    int set_instance_obj_dims(const uint32_t *d_dims_)
    {
        d_obj_dims = d_dims_;
        return LEXLS_OK;
    }
    /// lexls_lsi_batch_run while row counts are set: the mask's rule (refuse_masked_run)
    int refuse_ragged_run(const char *who) const
    {
        if (!d_obj_dims) return LEXLS_OK;
        lexls_internal_set_error((std::string(who) + ": not served while lexls_lsi_batch_set_instance_obj_dims holds per-instance objective row counts for this batch (they are device "
                                                     "memory, read by the kernels of lexls_lsi_batch_run_device / lexls_lsi_batch_enqueue_device only): clear them with a NULL pointer first").c_str());
        return LEXLS_ERR_UNSUPPORTED;
    }
    /// lexls_lsi_batch_run while limits are set: the mask's rule (refuse_masked_run) — its phase 1 is host work and reads no device memory
    int refuse_limited_run(const char *who) const
    {
        if (!d_limits) return LEXLS_OK;
        lexls_internal_set_error((std::string(who) + ": not served while lexls_lsi_batch_set_instance_max_factorizations holds per-instance limits for this batch (they are device "
                                                     "memory, read by the kernels of lexls_lsi_batch_run_device / lexls_lsi_batch_enqueue_device only): clear them with a NULL pointer first").c_str());
        return LEXLS_ERR_UNSUPPORTED;
    }
    /// lexls_lsi_batch_run while a mask is set: its phase 1 builds host objects from host data and cannot read a device mask — refused before any work
    int refuse_masked_run(const char *who) const
    {
        if (!d_mask) return LEXLS_OK;
        lexls_internal_set_error((std::string(who) + ": not served while lexls_lsi_batch_set_instance_mask holds an instance mask for this batch (the mask is device memory, read by "
                                                     "the kernels of lexls_lsi_batch_run_device / lexls_lsi_batch_enqueue_device only): clear it with a NULL mask first").c_str());
        return LEXLS_ERR_UNSUPPORTED;
    }
    /// the setting as a run with these parameters sees it (a run with regularization_type 0 ignores it, as it ignores h_reg_factors)
    void take_instance_regularization(Run &r) const
    {
        if (r.par.regularization_type == REGULARIZATION_NONE) return;
        r.inst_rows   = inst_mode == INST_HOST ? inst_factors.data() : NULL;
        r.d_inst_rows = inst_mode == INST_DEVICE ? d_inst_factors : NULL;
    }
    /// what the entry points refuse before any work: 0, or the code with lexls_last_error() set.  `who`: the entry point; with_v0: lexls_lsi_batch_run got h_v0
    int refuse_run(const char *who, const double *h_reg_factors, const ParametersLexLSI &par, bool with_v0) const
    {
        if (inst_mode == INST_NONE) return LEXLS_OK;
        if (h_reg_factors)
        {
            lexls_internal_set_error((std::string(who) + ": h_reg_factors must be NULL while lexls_lsi_batch_set_instance_regularization holds factors for this batch").c_str());
            return LEXLS_ERR_INVALID;
        }
        if (inst_mode != INST_DEVICE || par.regularization_type == REGULARIZATION_NONE) return LEXLS_OK;
        if (!would_be_resident(par))
        {
            lexls_internal_set_error((std::string(who) + ": per-instance regularization factors in device memory are served on resident runs only (not: LEXLS_LSI_RESIDENT=0, "
                                                         "regularization type 7, cycling handling of a regularized run); they are never copied to the host").c_str());
            return LEXLS_ERR_UNSUPPORTED;
        }
        if (with_v0)
        {
            lexls_internal_set_error((std::string(who) + ": per-instance regularization factors in device memory make phase 1 device work, which does not take h_v0").c_str());
            return LEXLS_ERR_UNSUPPORTED;
        }
        return LEXLS_OK;
    }
    BatchCtx &group_of_instance(uint32_t b, uint32_t &k)
    {
        k = b - lo[group_of[b]];
        return *grp[group_of[b]];
    }

    void run(const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0, const double *h_v0,
             const double *h_reg_factors, const ParametersLexLSI &par_, double *h_x, int32_t *h_info6, uint8_t *h_active, double *h_v, int32_t *h_rounds2)
    {
        if (!h_data || !h_x) throw Exception("lexls_lsi_batch_run: null data / x");
        if (par_.use_phase1_v0 && !h_x0) throw Exception("when use_phase1_v0 = true, x_guess has to be specified"); // (lexlsi.h:882, before any work)
        const ParametersLexLSI par = with_log_switch(par_);
        begin_working_set_log();
        fin.begin_run(par);
        last_kernel = "host";
        std::fill(cycling_count.begin(), cycling_count.end(), 0u);
        // getLambda of this run needs the rows gathered from resident constraint data, unrelaxed bounds and unregularized factorizations
        const int lam_after = (par.cycling_handling_enabled || par.regularization_type != REGULARIZATION_NONE || !gather || total > 65535) ? LEXLS_ERR_UNSUPPORTED : LEXLS_OK;
        const char *lam_why = par.cycling_handling_enabled ? "lexls_lsi_batch_get_lambda: not available after a run with cycling handling enabled (it may have relaxed bounds: in the instances' host copies, or in the resident constraint data of a resident run)"
                              : par.regularization_type != REGULARIZATION_NONE ? "lexls_lsi_batch_get_lambda: not available after a regularized run"
                                                                                : "lexls_lsi_batch_get_lambda: not available when the constraint data is not resident on the device (or beyond 65535 constraints)";
        Run r{h_data, h_x0, h_v0, h_reg_factors, h_var_index, h_active_guess, par, h_x, h_v, h_info6, h_rounds2, h_active};
        take_instance_regularization(r);
        // deactivate_first_wrong_sign is a removal rule the resident iterations know (collecting removal search + activation stamps, lexls_lsi_device.h);
        // the host-driven lock-step stages of a whole run do not: where the run would not be resident its instances go one by one
        if (par.deactivate_first_wrong_sign && !would_be_resident(par))
        {
            run_one_by_one(r, lam_after == LEXLS_OK);
            finish_working_set_log();
            const bool no_indices = off && !h_var_index;
            fin.set_rule(no_indices ? LEXLS_ERR_INVALID : lam_after, no_indices ? "lexls_lsi_batch_get_lambda: the run had no variable indices" : lam_why, par, false);
            return;
        }
        // LEXLS_LSI_DEVICE_PHASE1=1: no host objects, phase 1 is device work; so it is with per-instance factors in device memory, which no host
        // object may read (refuse_run has turned away the runs this cannot serve)
        if ((r.sw.device_phase1 || r.d_inst_rows) && !h_v0 && would_be_resident(par))
        {
            run_phase1_on_device(r, NULL);
            finish_working_set_log();
            const bool no_indices = off && !h_var_index;
            fin.set_rule(no_indices ? LEXLS_ERR_INVALID : lam_after, no_indices ? "lexls_lsi_batch_get_lambda: the run had no variable indices" : lam_why, par, true);
            return;
        }
        r.t_begin = BatchCtx::now();
        pool->prewake(); // (the workers went to sleep between two solves; they are needed in ~0.1 ms)
        prepare_groups(r);
        upload_regularization_block(r); // (before the constraint data's upload starts on another thread: this call may touch the handles)
        build_instances(r);
        host_rounds(r);
        if (r.resident) resident_rounds(r);
        collect(r);
        finish_working_set_log();
        report(r);
        fin.set_rule(lam_after, lam_why, par, r.resident);
        bool any_left = false;
        for (uint32_t b = 0; b < batch && !any_left; b++) any_left = r.lsi[b] != nullptr;
        if (any_left) pool->run(batch, [&](uint32_t b) { r.lsi[b].reset(); }); // a thousand LexLSI objects (dozens of vectors each): freed in parallel, not serially on return
    }

    /// A deactivate_first_wrong_sign run (lexlsi.h:1089-1103) that cannot be resident (LEXLS_LSI_RESIDENT=0, cycling handling of a regularized run, regularization type 7,
    /// no register-resident kernel, data not gathered): its instances go one after the other through the single-problem driver — same results as
    /// lexls_lsi_solve_ex on each, every equality problem on the GPU, the wrong-sign multipliers read back per iteration.
    void run_one_by_one(Run &r, bool lambda_possible)
    {
        int32_t fs = 0;
        for (uint32_t b = 0; b < batch; b++)
        {
            const runner::LsiProblem p = problem(r, b);
            internal::LexLSI lsi;
            fs += solve_one(lsi, device, p, r.par, r.h_x + (size_t)b * nVar, r.h_info6 ? r.h_info6 + (size_t)b * 6 : NULL, r.h_active ? r.h_active + (size_t)b * total : NULL,
                            r.h_v ? r.h_v + (size_t)b * total : NULL).factorizations;
            fin.keep_working_set(b, lsi, p.data, p.var_index);
            keep_host_log(b, lsi);
            cycling_count[b] = static_cast<uint32_t>(lsi.getCyclingCounter());
        }
        last_stats[0] = fs, last_stats[1] = last_stats[2] = 0, last_stats[3] = 1;
        if (r.h_rounds2) r.h_rounds2[0] = fs, r.h_rounds2[1] = 0;
        // (these instances never used the group handles: the constraint data getLambda gathers from goes there now — one copy of the batch's
        // data per run, asked for or not: the caller's array is gone when get_lambda comes, and this path solves its instances one by one,
        // milliseconds each, against ~1 ms per 16 MB for the copy)
        if (lambda_possible && (!off || r.h_var_index))
            for (uint32_t g = 0; g < nGroups; g++) hip_check(lexls_lse_set_constraint_data(grp[g]->h, r.h_data + (size_t)lo[g] * per_data, per_data));
    }

    /// the variable indices of a simple-bounds objective 0 (dim0 per instance) of group g, for the step kernels
    void upload_variable_indices(const Run &r, uint32_t g, uint32_t *d_var, uint32_t dim0)
    {
        if (!dim0) return;
        BatchCtx &ctx = *grp[g];
        if (!r.h_var_index) throw Exception("lexls_lsi_batch_run: a simple-bounds objective needs variable indices");
        if (hipMemcpyAsync(d_var, r.h_var_index + (size_t)lo[g] * dim0, 4 * (size_t)ctx.B * dim0, hipMemcpyHostToDevice, ctx.stream) != hipSuccess || hipStreamSynchronize(ctx.stream) != hipSuccess)
            throw Exception("upload of the variable indices failed");
    }

    /// whole iterations on the device: plain runs and the regularized ones the register-resident kernel's REG instantiations serve (every
    /// type but the experimental 7).  Cycling handling is part of the resident iteration of an unregularized run (the handler's state travels with the
    /// instance, a relaxed bound is written into the resident constraint data: lexls_lsi_device.h); a regularized run with cycling handling keeps
    /// the host path, as every other case
    bool would_be_resident(const ParametersLexLSI &par) const
    {
        const int reg_type = static_cast<int>(par.regularization_type);
        return gather && (!par.cycling_handling_enabled || reg_type == 0) && resident_ok && grp[0]->resident && (reg_type == 0 || lexls_internal_resident_reg_serves(grp[0]->h, reg_type)) &&
               par.max_number_of_factorizations < 0x7fffffff;
    }

    /// every group back to what a fresh one holds, with this run's parameters; decides what kind of run it is
    void prepare_groups(Run &r)
    {
        // Cycling handling on the host relaxes bounds in the instances' host copies of the constraint data (cycling.h:32-65, objective.h:774-790):
        // such a run assembles its problems on the host from those copies instead of gathering rows of the resident (unrelaxed) device copy.
        // A resident run relaxes the device copy itself; what the host does of it before the hand-over (at most one working-set change per
        // instance) relaxes nothing, so its stages gather from the device copy like any other run's
        r.resident = would_be_resident(r.par);
        r.gather   = gather && (!r.par.cycling_handling_enabled || r.resident);
        for (uint32_t g = 0; g < nGroups; g++)
        {
            BatchCtx &ctx = *grp[g];
            ctx.gather    = r.gather;
            if (!r.gather) ctx.need_staging();
            ctx.reset();
            ctx.clear_working_set_log();
            ctx.set_first_wrong_sign(r.par.deactivate_first_wrong_sign);
            ctx.set_cycling(r.par.cycling_handling_enabled && r.resident, r.par.cycling_relax_step, static_cast<uint32_t>(r.par.cycling_max_counter));
            hip_check(lexls_lse_set_tolerance(ctx.h, r.par.tol_linear_dependence));
            ctx.reg_type = static_cast<int>(r.par.regularization_type), ctx.reg_variable = r.par.variable_regularization_factor, ctx.reg_cg_iters = r.par.max_number_of_CG_iterations;
            ctx.reg_dirty.store(ctx.reg_type != 0);
            if (ctx.reg_type == 0) hip_check(lexls_lse_set_regularization(ctx.h, 0, NULL, 0, 0.0));
            if (r.gather && ctx.device_step)
            {
                ctx.shape.tol_feasibility = r.par.tol_feasibility;
                upload_variable_indices(r, g, ctx.d_var, ctx.shape.dim0);
            }
        }
        r.step     = r.gather && grp[0]->device_step;
    }

    /// A regularized resident run: its regularization goes to the device ONCE, as a block in every group's stream — LexLSE level k takes the
    /// factor of objective k + off (a simple-bounds objective 0 becomes fixed variables and has none: lexlsi.h formLexLSE), whatever the level
    /// holds in the working set of the moment.  The host copy the instances post into (SlotLSE::setRegularizationFactor) starts from the
    /// same values, so phase 1 finds nothing to upload again.
    /// Per-instance factors (lexls_lsi_batch_set_instance_regularization): row lo[g] + i of the caller's array fills row i of group g's block, from the
    /// host copy through the same staging, from a device array by lsi_instance_factors_kernel in the group's stream.  A run on a device array
    /// has no host objects (phase 1 is device work), so nobody reads the host copy ctx.reg_factor, which does not hold its factors.
    void upload_regularization_block(Run &r)
    {
        const int reg_type = static_cast<int>(r.par.regularization_type);
        if (!r.resident || reg_type == 0) return;
        const uint32_t nObjL = nObj - off;
        std::vector<double> level_factor(nObjL, 0.0);
        if (r.h_reg_factors)
            for (uint32_t k = 0; k + off < nObj; k++) level_factor[k] = r.h_reg_factors[k + off];
        for (uint32_t g = 0; g < nGroups; g++)
        {
            BatchCtx &ctx = *grp[g];
            if (r.d_inst_rows)
            {
                double *d_block = NULL;
                hip_check(lexls_internal_set_regularization_block_device(ctx.h, reg_type, ctx.reg_variable, ctx.reg_cg_iters, &d_block));
                const uint32_t cells = ctx.B * nObjL;
                hipLaunchKernelGGL(lsi_instance_factors_kernel, dim3((cells + 255) / 256), dim3(256), 0, ctx.stream, r.d_inst_rows + (size_t)lo[g] * nObj, ctx.B, nObj, nObjL, off, d_block);
                if (hipGetLastError() != hipSuccess) throw Exception("lsi_instance_factors_kernel launch failed");
            }
            else if (r.inst_rows)
            {
                for (uint32_t i = 0; i < ctx.B; i++)
                    std::copy(r.inst_rows + (size_t)(lo[g] + i) * nObj + off, r.inst_rows + (size_t)(lo[g] + i + 1) * nObj, ctx.reg_factor.begin() + (size_t)i * nObjL);
                hip_check(lexls_internal_set_regularization_block_per_problem(ctx.h, reg_type, ctx.reg_factor.data(), ctx.reg_variable, ctx.reg_cg_iters));
            }
            else
            {
                hip_check(lexls_internal_set_regularization_block(ctx.h, reg_type, level_factor.data(), ctx.reg_variable, ctx.reg_cg_iters));
                for (uint32_t b = 0; b < ctx.B; b++) std::copy(level_factor.begin(), level_factor.end(), ctx.reg_factor.begin() + (size_t)b * ctx.nObjL);
            }
            ctx.reg_dirty.store(false);
        }
    }

    /// The constraint data goes to the device (16 MB for 1024 IK instances: ~0.4 ms) while the worker pool builds the instances' host
    /// objects and runs their phase 1: nothing of that touches the handles; joined before the first stage.
    void build_instances(Run &r)
    {
        int upload_rc = LEXLS_OK;
        std::string upload_err;
        std::thread uploader;
        if (r.gather)
            uploader = std::thread([&]() {
                for (uint32_t g = 0; g < nGroups && upload_rc == LEXLS_OK; g++)
                {
                    upload_rc = lexls_lse_set_constraint_data(grp[g]->h, r.h_data + (size_t)lo[g] * per_data, per_data);
                    if (upload_rc != LEXLS_OK) upload_err = lexls_last_error();
                }
            });
        struct Joiner // (the setup below may throw)
        {
            std::thread &t;
            ~Joiner()
            {
                if (t.joinable()) t.join();
            }
        } joiner{uploader};
        if (r.resident)
            for (uint32_t g = 0; g < nGroups; g++)
            {
                grp[g]->rshape.tol_feasibility = r.par.tol_feasibility;
                upload_variable_indices(r, g, grp[g]->d_rvar, grp[g]->rshape.dim0);
            }
        r.hooks = std::vector<SlotStep>(r.step ? batch : 0);
        r.t_ctx = BatchCtx::now() - r.t_begin;
        r.lsi   = std::vector<std::unique_ptr<SlotLSI>>(batch);
        r.prob.resize(batch);
        pool->run(batch, [&](uint32_t b) {
            uint32_t k;
            BatchCtx &ctx = group_of_instance(b, k);
            r.lsi[b].reset(new SlotLSI());
            r.lsi[b]->getLexLSE().bind(&ctx, k);
            r.prob[b] = problem(r, b);
            runner::setup(*r.lsi[b], r.prob[b], r.par);
            r.lsi[b]->setSensitivityScansAllLevels(true);
            if (r.step)
            {
                r.hooks[b].c = &ctx;
                r.hooks[b].b = k;
                r.lsi[b]->setStepHook(&r.hooks[b]);
            }
            r.lsi[b]->begin();
        });
        if (uploader.joinable()) uploader.join();
        if (upload_rc != LEXLS_OK) throw Exception(std::string("liblexls_hip: ") + upload_err);
        r.t_setup = BatchCtx::now() - r.t_begin;
    }

    /// The job of instance k of group g between two stages: take over the results of the stage that just finished (if it was served), advance
    /// its active-set logic, and post what it needs next into the group's round block and into r.wants[g].
    void advance_instance(Run &r, uint32_t g, uint32_t k)
    {
        BatchCtx &ctx = *grp[g];
        SlotLSI &inst = *r.lsi[lo[g] + k];
        if (r.resident && ctx.is_resident[k]) return; // waits for the others to leave phase 1
        const bool served_fs = ctx.stage_fs && !ctx.skip[k], served_sens = ctx.stage_sens && ctx.skip[k] && ctx.objidx[k] >= 0;
        const bool has_spec  = served_fs && ctx.stage_sens && ctx.objidx[k] == 0; // its removal search ran right behind its l-QR
        if (r.step) ctx.mode()[k] = 0; // (the hook raises it again when the instance posts an iteration's equality problem)
        if (served_fs) ctx.take_solution(k);
        if (served_fs || served_sens) inst.advance();
        if (has_spec && !inst.finished() && inst.need() == SlotLSI::NEED_SENSITIVITY && inst.needLevel() == 0) inst.advance(); // step not blocked: use it
        const bool alive = !inst.finished();
        if (r.resident && alive && inst.atIterationSolve())
        {
            // phase 1 is over and the equality problem of a regular iteration is staged: from here on the instance iterates on the
            // device (its staged problem is served by the first resident stage)
            ctx.hand_over(k, inst);
            ctx.skip[k]   = 1;
            ctx.objidx[k] = -1;
            return;
        }
        const bool fs    = alive && inst.need() == SlotLSI::NEED_FACTORIZE_SOLVE;
        const bool se    = alive && inst.need() == SlotLSI::NEED_SENSITIVITY;
        const bool spec  = fs && ctx.spec_sens;
        ctx.skip[k]      = fs ? 0 : 1;
        ctx.objidx[k]    = se ? static_cast<int32_t>(inst.needLevel()) : (spec ? 0 : -1);
        const bool dstep = r.step && fs && ctx.mode()[k] != 0;
        const uint32_t w = (alive ? WANT_ALIVE : 0u) | (fs ? WANT_FS : 0u) | ((se || spec) ? WANT_SENS : 0u) | (dstep ? WANT_STEP : 0u) | ((fs && !dstep) ? WANT_X : 0u);
        if (w & ~r.wants[g].load(std::memory_order_relaxed)) r.wants[g].fetch_or(w, std::memory_order_relaxed);
    }
    void turn(Run &r, uint32_t g)
    {
        r.wants[g].store(0);
        const double t0 = BatchCtx::now();
        pool->run(lo[g + 1] - lo[g], [&](uint32_t k) { advance_instance(r, g, k); });
        r.t_host += BatchCtx::now() - t0;
    }
    /// one stage of group g for what its instances asked for; false when no instance of the group is alive any more
    bool enqueue(Run &r, uint32_t g)
    {
        BatchCtx &ctx    = *grp[g];
        const uint32_t w = r.wants[g].load();
        ctx.stage_fs = ctx.stage_sens = false;
        if (!(w & WANT_ALIVE)) return false;
        if (!(w & (WANT_FS | WANT_SENS))) throw Exception("lexls_lsi_batch_solve: an instance is alive but requests nothing");
        ctx.enqueue_stage((w & WANT_FS) != 0, (w & WANT_SENS) != 0, (w & WANT_STEP) != 0, (w & WANT_X) != 0, r.par.tol_wrong_sign_lambda, r.par.tol_correct_sign_lambda);
        return true;
    }

    /// The stages the host's active-set logic drives.  One stage of group g serves every pending factorize+solve of the group in one call and
    /// every pending ObjectiveSensitivity in one call (different instances), both only enqueued.  Between two stages every instance of the
    /// group runs ONE job on the worker pool (advance_instance).
    void host_rounds(Run &r)
    {
        r.wants = std::vector<std::atomic<uint32_t>>(nGroups);
        std::vector<char> alive(nGroups, 0);
        bool any = false;
        for (uint32_t g = 0; g < nGroups; g++)
        {
            turn(r, g); // nothing served yet: only posts the first requests
            any = (alive[g] = enqueue(r, g)) || any;
        }
        while (any)
        {
            any = false;
            for (uint32_t g = 0; g < nGroups; g++)
                if (alive[g])
                {
                    grp[g]->finish_stage(); // the other groups' stages keep the GPU busy meanwhile
                    turn(r, g);
                    alive[g] = enqueue(r, g);
                    any      = any || alive[g];
                }
        }
    }

    /// the iterations of the handed-over instances, on the device until every one has stopped; their slabs come back at the end
    void resident_rounds(Run &r)
    {
        std::vector<char> going(nGroups, 0);
        bool more = false;
        for (uint32_t g = 0; g < nGroups; g++)
        {
            BatchCtx &ctx  = *grp[g];
            ctx.n_resident = 0;
            for (uint32_t k = 0; k < ctx.B; k++)
            {
                const bool res = ctx.is_resident[k] != 0;
                ctx.skip[k]    = res ? 0 : 1;
                ctx.objidx[k]  = res ? 0 : -1;
                ctx.n_resident += res ? 1u : 0u;
            }
            if (ctx.n_resident)
            {
                ctx.begin_resident();
                going[g] = 1;
                more     = true;
            }
        }
        resident_chunks(r, going, more);
        for (uint32_t g = 0; g < nGroups; g++)
            if (grp[g]->n_resident)
            {
                grp[g]->download_resident(r.sw.stamps_dump);
                last_kernel = grp[g]->resident_kernel; // (every group takes the same path: same shape, same regularization)
            }
    }

    /// stages of the groups in `going` until every one of their instances has stopped
    void resident_chunks(Run &r, std::vector<char> &going, bool more)
    {
        // stages are enqueued in chunks; after each chunk ONE word comes back (instances that have stopped).  Stages past an
        // instance's end skip it in every kernel; a chunk that turns out not to be needed costs a few launches of early-exit kernels
        const int chunk = 8;
        bool freed = r.lsi.empty(); // (phase 1 on the device: there are no host objects)
        while (more)
        {
            more = false;
            for (uint32_t g = 0; g < nGroups; g++)
                if (going[g]) grp[g]->enqueue_resident(chunk, r.par.tol_wrong_sign_lambda, r.par.tol_correct_sign_lambda, static_cast<int32_t>(r.par.max_number_of_factorizations));
            if (!freed) // the handed-over instances' host objects (a thousand LexLSI instances, dozens of vectors each) are not needed any
            {           // more: they are freed now, while the GPU works on the first chunk, instead of on the caller's time at the end
                freed = true;
                pool->run(batch, [&](uint32_t b) {
                    uint32_t k;
                    if (group_of_instance(b, k).is_resident[k]) r.lsi[b].reset();
                });
            }
            for (uint32_t g = 0; g < nGroups; g++)
                if (going[g])
                {
                    if (grp[g]->resident_done()) going[g] = 0;
                    more = more || going[g];
                }
        }
    }

    /// the arrays of lexls_lsi_batch_run_device: memory of the batch's device
    struct DeviceArrays
    {
        const double *data;
        const uint32_t *var_index;
        const uint8_t *active_guess;
        const double *x0;
        double *x;
        int32_t *info6;
        uint8_t *active;
        double *v;
        const double *v0 = NULL;        // lexls_lsi_batch_run_device_ex: initial residuals (used with x0 only)
        uint32_t *cycling_counts = NULL; // ... and where the scatter kernel leaves the cycling handlers' relaxation counts
    };

    /// A resident run (would_be_resident) without host LexLSI objects: the constraint data goes into every group's resident copy, the setup kernel
    /// writes the slabs and the first equality problem where they live, iteration 0 follows the first stage on the device (lsi_phase1_device.h),
    /// and the run goes on as the resident run it is.  dev == NULL: the arrays of r are host memory (lexls_lsi_batch_run under
    /// LEXLS_LSI_DEVICE_PHASE1=1) — uploaded, results taken from the downloaded slabs; otherwise everything stays on the device
    void run_phase1_on_device(Run &r, const DeviceArrays *dev)
    {
        r.t_begin = BatchCtx::now();
        prepare_groups(r);
        if (!r.resident) throw Exception("lexls_lsi_batch_run: phase 1 on the device needs a resident run");
        upload_regularization_block(r);
        const double *data     = dev ? dev->data : r.h_data;
        const uint32_t *var    = dev ? dev->var_index : r.h_var_index;
        const uint8_t *guess   = dev ? dev->active_guess : r.h_active_guess;
        const double *x0       = dev ? dev->x0 : r.h_x0;
        const double *v0       = dev ? dev->v0 : NULL; // (only lexls_lsi_batch_run_device_ex gives one, and only together with x0)
        const uint32_t dim0    = off ? dims[0] : 0u;
        const int32_t max_fact = static_cast<int32_t>(r.par.max_number_of_factorizations);
        if (dim0 && !var) throw Exception("lexls_lsi_batch_run: a simple-bounds objective needs variable indices");
        if (r.par.use_phase1_v0 && !x0) throw Exception("when use_phase1_v0 = true, x_guess has to be specified"); // (the entry points have said so already)
        for (uint32_t g = 0; g < nGroups; g++)
        {
            BatchCtx &ctx              = *grp[g];
            ctx.rshape.tol_feasibility = r.par.tol_feasibility;
            hip_check(dev ? lexls_internal_set_constraint_data_device(ctx.h, data + (size_t)lo[g] * per_data, per_data) : lexls_lse_set_constraint_data(ctx.h, data + (size_t)lo[g] * per_data, per_data));
            if (dim0 && hipMemcpyAsync(ctx.d_rvar, var + (size_t)lo[g] * dim0, 4 * (size_t)ctx.B * dim0, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx.stream) != hipSuccess)
                throw Exception("copy of the variable indices failed");
            const uint8_t *gg = guess ? guess + (size_t)lo[g] * total : NULL;
            const double *xg  = x0 ? x0 + (size_t)lo[g] * nVar : NULL;
            ctx.enqueue_phase1_setup(dev ? xg : ctx.stage_x0(xg), dev ? gg : ctx.stage_guess(gg), lo[g], max_fact, v0 ? v0 + (size_t)lo[g] * total : NULL, NULL,
                                     dev ? group_mask(g) : NULL, dev ? group_limits(g) : NULL, dev ? group_obj_dims(g) : NULL, p1_hot_word(r.par)); // (mask, limits and row counts are the device entries' alone: lexls_lsi_batch_run is refused while one is set)
        }
        r.t_ctx = BatchCtx::now() - r.t_begin;
        uint32_t fault = 0xffffffffu;
        for (uint32_t g = 0; g < nGroups; g++)
        {
            grp[g]->finish_stage();
            fault = std::min(fault, grp[g]->p1_fault_host[0]);
        }
        if (fault != 0xffffffffu) // nothing else is launched for this run
            throw Exception("lexls_lsi_batch_run: instance " + std::to_string(fault >> 3) + ": " + p1_fault_text(fault & 7u));
        for (uint32_t g = 0; g < nGroups; g++)
            if (r.par.use_phase1_v0)
                grp[g]->enqueue_phase1_v0(max_fact);
            else
                grp[g]->enqueue_phase1_stage(x0 != NULL, r.par.tol_wrong_sign_lambda, r.par.tol_correct_sign_lambda, max_fact, true, p1_hot_word(r.par));
        r.t_setup = BatchCtx::now() - r.t_begin;
        std::vector<char> going(nGroups, 0), went(nGroups, 0);
        bool more = false;
        for (uint32_t g = 0; g < nGroups; g++)
        {
            went[g] = going[g] = grp[g]->resident_done() ? 0 : 1; // (an instance that stopped in iteration 0 never reaches a resident stage)
            more               = more || going[g];
        }
        resident_chunks(r, going, more);
        const bool keep_fixed_bounds = fin.needs_final_problem(r.par);
        for (uint32_t g = 0; g < nGroups; g++)
        {
            BatchCtx &ctx = *grp[g];
            if (dev)
                ctx.scatter_results(dev->x + (size_t)lo[g] * nVar, dev->info6 ? dev->info6 + (size_t)lo[g] * 6 : NULL, dev->active ? dev->active + (size_t)lo[g] * total : NULL,
                                    dev->v ? dev->v + (size_t)lo[g] * total : NULL, keep_fixed_bounds, dev->cycling_counts ? dev->cycling_counts + lo[g] : NULL, NULL, NULL, group_mask(g));
            ctx.download_resident(r.sw.stamps_dump, dev == NULL);
            if (went[g]) last_kernel = ctx.resident_kernel;
        }
        if (dev) // the working sets for get_lambda, the relaxations done; x / v / info / active are in the caller's arrays already
            for (uint32_t b = 0; b < batch; b++)
            {
                uint32_t k;
                BatchCtx &ctx = group_of_instance(b, k);
                if (ctx.cycling) cycling_count[b] = ctx.rl.cyc(ctx.rws_host.data(), k)[CYC_COUNT];
                fin.keep_working_set_resident(b, ctx, k, NULL, NULL);
            }
        else
        {
            r.prob.resize(batch);
            for (uint32_t b = 0; b < batch; b++) r.prob[b] = problem(r, b);
            collect(r);
        }
        report(r);
    }

    /// ... and why not, after a run_device / enqueue_device run
    static const char *lam_msg_after_device_run(const ParametersLexLSI &par)
    {
        return par.cycling_handling_enabled ? "lexls_lsi_batch_get_lambda: not available after a run with cycling handling enabled (it may have relaxed bounds in the resident constraint data)"
                                               : "lexls_lsi_batch_get_lambda: not available after a regularized run";
    }
    /// lexls_lsi_batch_run_device(_ex): the caller has checked would_be_resident(par)
    void run_device(const DeviceArrays &dev, const double *h_reg_factors, const ParametersLexLSI &par)
    {
        begin_working_set_log(); // (no host objects: every entry is written on the device)
        fin.begin_run(par);
        last_kernel = "host";
        std::fill(cycling_count.begin(), cycling_count.end(), 0u);
        Run r{NULL, NULL, NULL, h_reg_factors, NULL, NULL, par, NULL, NULL, NULL, NULL, NULL};
        take_instance_regularization(r);
        run_phase1_on_device(r, &dev);
        finish_working_set_log();
        fin.set_rule(fin.lam_rc_after(par), lam_msg_after_device_run(par), par, true, d_obj_dims != NULL);
    }

    /// the runs lexls_lsi_batch_enqueue_device serves: those of run_device that the persistent launch takes, decided on numbers (every group's handle:
    /// their batch sizes differ by one)
    bool would_be_fused(const ParametersLexLSI &par) const
    {
        if (nGroups != 1 || !would_be_resident(par)) return false; // (several groups: only under LEXLS_LSI_GROUPS where runs are resident; not served)
        for (uint32_t g = 0; g < nGroups; g++)
            if (!lexls_internal_resident_fused_serves(grp[g]->h, off ? 1 : 0, static_cast<int>(par.regularization_type), resident_lds_per_wave(grp[g]->rshape.SD, grp[g]->rshape.total))) return false;
        return true;
    }

    /// lexls_lsi_batch_enqueue_device (the caller has checked would_be_fused(par): one group): run_phase1_on_device with device arrays, without its waits.
    /// The run forks from `s` into the group's stream and joins it again; the fault word stays on the device (lsi_phase1_gate_kernel acts on it); nothing
    /// comes back to the host before finish().  No HIP call here waits for the device, and none allocates once a run with these options has been enqueued
    void enqueue_device(hipStream_t s, const DeviceArrays &dev, const double *h_reg_factors, const ParametersLexLSI &par, uint32_t *d_status, double *d_lambda)
    {
        if (hipSetDevice(device) != hipSuccess) throw Exception("hipSetDevice failed (lexls_lsi_batch_enqueue_device)");
        if (d_lambda) fin.ensure_lambda_bufs();
        if (!async)
        {
            std::unique_ptr<Async> a(new Async());
            if (hipMalloc((void **)&a->d_fault, 16) != hipSuccess || hipEventCreateWithFlags(&a->ev_fork, hipEventDisableTiming) != hipSuccess)
                throw Exception("hipMalloc / hipEventCreate failed (lexls_lsi_batch_enqueue_device)");
            a->fault_host.assign(4, 0xffffffffu);
            for (uint32_t g = 0; g < nGroups; g++)
                if (hipEventCreateWithFlags(&grp[g]->ev_joined, hipEventDisableTiming) != hipSuccess)
                    throw Exception("hipEventCreate failed (lexls_lsi_batch_enqueue_device)");
            async = std::move(a);
        }
        Async &as = *async;
        Run r{NULL, NULL, NULL, h_reg_factors, NULL, NULL, par, NULL, NULL, NULL, NULL, NULL};
        take_instance_regularization(r);
        const int reg_type     = static_cast<int>(par.regularization_type);
        const uint32_t nObjL   = nObj - off, dim0 = off ? dims[0] : 0u;
        const int32_t max_fact = static_cast<int32_t>(par.max_number_of_factorizations);
        const double *d_rows   = r.d_inst_rows;
        if (r.inst_rows) // host factors of every instance: one pinned copy, uploaded when they have changed
        {
            if (as.inst_uploaded != inst_gen)
            {
                if (as.pending) throw Exception("lexls_lsi_batch_enqueue_device: the host factors of lexls_lsi_batch_set_instance_regularization have changed while an enqueued run "
                                                "may still read the previous ones: call lexls_lsi_batch_finish first");
                if (!as.d_inst)
                {
                    if (hipMalloc((void **)&as.d_inst, 8 * (size_t)batch * nObj) != hipSuccess) throw Exception("hipMalloc failed (lexls_lsi_batch_enqueue_device)");
                    as.inst_stage.assign((size_t)batch * nObj, 0.0);
                }
                std::copy(inst_factors.begin(), inst_factors.end(), as.inst_stage.begin());
                if (hipMemcpyAsync(as.d_inst, as.inst_stage.data(), 8 * (size_t)batch * nObj, hipMemcpyHostToDevice, s) != hipSuccess)
                    throw Exception("hipMemcpyAsync failed (per-instance regularization factors)");
                as.inst_uploaded = inst_gen;
            }
            d_rows = as.d_inst;
        }
        // the host's record of the last run: nothing of it is valid until finish()
        wlog_valid  = false;
        fin.begin_run(par);
        last_kernel = "host";
        std::fill(cycling_count.begin(), cycling_count.end(), 0u);
        as.pending = as.enqueued = true;
        as.stream  = s;
        as.par     = par;
        hipLaunchKernelGGL(lsi_fault_reset_kernel, dim3(1), dim3(64), 0, s, as.d_fault);
        if (hipGetLastError() != hipSuccess || hipEventRecord(as.ev_fork, s) != hipSuccess) throw Exception("lsi_fault_reset_kernel launch / hipEventRecord failed (lexls_lsi_batch_enqueue_device)");
        for (uint32_t g = 0; g < nGroups; g++)
        {
            BatchCtx &ctx = *grp[g];
            if (hipStreamWaitEvent(ctx.stream, as.ev_fork, 0) != hipSuccess) throw Exception("hipStreamWaitEvent failed (lexls_lsi_batch_enqueue_device)");
            // prepare_groups, without BatchCtx::reset(): the pinned blocks it clears belong to the host-driven stages, which this run has none of
            ctx.gather = true;
            ctx.clear_working_set_log_by_kernel();
            ctx.set_first_wrong_sign(par.deactivate_first_wrong_sign);
            ctx.set_cycling(par.cycling_handling_enabled, par.cycling_relax_step, static_cast<uint32_t>(par.cycling_max_counter));
            hip_check(lexls_lse_set_tolerance(ctx.h, par.tol_linear_dependence));
            ctx.reg_type = reg_type, ctx.reg_variable = par.variable_regularization_factor, ctx.reg_cg_iters = par.max_number_of_CG_iterations;
            ctx.reg_dirty.store(false);
            ctx.rounds_fs = ctx.rounds_sens = ctx.rounds_step = 0;
            ctx.t_enqueue = ctx.t_wait = 0.0;
            ctx.stage_fs = ctx.stage_sens = false;
            if (reg_type == 0)
                hip_check(lexls_lse_set_regularization(ctx.h, 0, NULL, 0, 0.0));
            else // upload_regularization_block, every kind of factors written by a kernel in the group's stream
            {
                double *d_block = NULL;
                hip_check(lexls_internal_set_regularization_block_device(ctx.h, reg_type, ctx.reg_variable, ctx.reg_cg_iters, &d_block));
                const uint32_t cells = ctx.B * nObjL;
                if (d_rows)
                    hipLaunchKernelGGL(lsi_instance_factors_kernel, dim3((cells + 255) / 256), dim3(256), 0, ctx.stream, d_rows + (size_t)lo[g] * nObj, ctx.B, nObj, nObjL, off, d_block);
                else
                {
                    LevelFactors lf;
                    for (uint32_t k = 0; k < STEP_MAX_OBJ; k++) lf.f[k] = (h_reg_factors && k + off < nObj) ? h_reg_factors[k + off] : 0.0;
                    hipLaunchKernelGGL(lsi_level_factors_kernel, dim3((cells + 255) / 256), dim3(256), 0, ctx.stream, lf, ctx.B, nObjL, d_block);
                }
                if (hipGetLastError() != hipSuccess) throw Exception("launch of the regularization factors' kernel failed");
            }
            ctx.rshape.tol_feasibility = par.tol_feasibility;
            hip_check(lexls_internal_set_constraint_data_device(ctx.h, dev.data + (size_t)lo[g] * per_data, per_data));
            if (dim0 && hipMemcpyAsync(ctx.d_rvar, dev.var_index + (size_t)lo[g] * dim0, 4 * (size_t)ctx.B * dim0, hipMemcpyDeviceToDevice, ctx.stream) != hipSuccess)
                throw Exception("copy of the variable indices failed");
            ctx.enqueue_phase1_setup(dev.x0 ? dev.x0 + (size_t)lo[g] * nVar : NULL, dev.active_guess ? dev.active_guess + (size_t)lo[g] * total : NULL, lo[g], max_fact,
                                     dev.v0 ? dev.v0 + (size_t)lo[g] * total : NULL, as.d_fault, group_mask(g), group_limits(g), group_obj_dims(g), p1_hot_word(par));
            const bool keep_fixed_bounds = fin.needs_final_problem(par);
            ctx.enqueue_phase1_gate(as.d_fault, max_fact);
            if (par.use_phase1_v0)
                ctx.enqueue_phase1_v0(max_fact, false);
            else
                ctx.enqueue_phase1_stage(dev.x0 != NULL, par.tol_wrong_sign_lambda, par.tol_correct_sign_lambda, max_fact, false, p1_hot_word(par));
            ctx.enqueue_fused(par.tol_wrong_sign_lambda, par.tol_correct_sign_lambda, max_fact);
            ctx.scatter_results(dev.x + (size_t)lo[g] * nVar, dev.info6 ? dev.info6 + (size_t)lo[g] * 6 : NULL, dev.active ? dev.active + (size_t)lo[g] * total : NULL,
                                dev.v ? dev.v + (size_t)lo[g] * total : NULL, keep_fixed_bounds, dev.cycling_counts ? dev.cycling_counts + lo[g] : NULL, as.d_fault, g == 0 ? d_status : NULL, group_mask(g));
            if (d_lambda) fin.enqueue_lambda(g, max_fact, as.d_fault, d_lambda);
            if (hipEventRecord(ctx.ev_joined, ctx.stream) != hipSuccess || hipStreamWaitEvent(s, ctx.ev_joined, 0) != hipSuccess)
                throw Exception("hipEventRecord / hipStreamWaitEvent failed (lexls_lsi_batch_enqueue_device)");
        }
    }

    /// lexls_lsi_batch_finish: waits for the stream (NULL: the one of the last enqueue), then fetches what run_phase1_on_device downloads before it returns —
    /// the fault word, the slabs with the working sets, counters and cycling counts, the active simple bounds — and leaves the batch as run_device does
    int finish(hipStream_t s)
    {
        if (!async || !async->enqueued) throw Exception("lexls_lsi_batch_finish: no lexls_lsi_batch_enqueue_device on this batch");
        Async &as = *async;
        if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize(s ? s : as.stream) != hipSuccess) throw Exception("lexls_lsi_batch_finish: stream synchronisation failed");
        as.pending  = false;
        fin.forget();
        last_kernel = "host";
        wlog_valid  = false;
        std::fill(cycling_count.begin(), cycling_count.end(), 0u);
        if (hipMemcpyAsync(as.fault_host.data(), as.d_fault, 4, hipMemcpyDeviceToHost, grp[0]->stream) != hipSuccess || hipStreamSynchronize(grp[0]->stream) != hipSuccess)
            throw Exception("lexls_lsi_batch_finish: download of the fault word failed");
        const uint32_t fault = as.fault_host[0];
        if (fault != 0xffffffffu) throw Exception("lexls_lsi_batch_run: instance " + std::to_string(fault >> 3) + ": " + p1_fault_text(fault & 7u));
        const ParametersLexLSI &par = as.par;
        const bool keep_fixed_bounds = fin.needs_final_problem(par);
        int rounds_fs = 0, rounds_sens = 0, rounds_step = 0;
        for (uint32_t g = 0; g < nGroups; g++)
        {
            BatchCtx &ctx = *grp[g];
            if (keep_fixed_bounds) ctx.fetch_fixed_bounds();
            ctx.download_resident(false, false, true);
            bool went = false; // some instance was alive behind iteration 0 (run_phase1_on_device: the group went into the persistent launch)
            for (uint32_t k = 0; k < ctx.B && !went; k++) went = ctx.rl.info(ctx.rws_host.data(), k)[1] > 1;
            if (went) last_kernel = ctx.resident_kernel;
            rounds_fs += ctx.rounds_fs, rounds_sens += ctx.rounds_sens, rounds_step += ctx.rounds_step + ctx.rounds_resident;
        }
        for (uint32_t b = 0; b < batch; b++)
        {
            uint32_t k;
            BatchCtx &ctx = group_of_instance(b, k);
            if (ctx.cycling) cycling_count[b] = ctx.rl.cyc(ctx.rws_host.data(), k)[CYC_COUNT];
            fin.keep_working_set_resident(b, ctx, k, NULL, NULL);
        }
        last_stats[0] = rounds_fs, last_stats[1] = rounds_sens, last_stats[2] = rounds_step, last_stats[3] = (int32_t)nGroups;
        wlog_valid = wlog != nullptr;
        fin.set_rule(fin.lam_rc_after(par), lam_msg_after_device_run(par), par, true, d_obj_dims != NULL);
        return LEXLS_OK;
    }

    /// instance b's results into the caller's arrays, and its final working set for get_lambda
    void collect_instance(Run &r, uint32_t b)
    {
        uint32_t k;
        BatchCtx &ctx = group_of_instance(b, k);
        double *x = r.h_x + (size_t)b * nVar, *v = r.h_v ? r.h_v + (size_t)b * total : NULL;
        if (r.resident && ctx.is_resident[k]) // x, v, working set and counters as the device left them (its host object is gone already)
        {
            unpack_state(ctx.rstate_host.data() + (size_t)k * ctx.rshape.SD, nVar, total, x, v);
            if (r.h_active) std::copy(ctx.rl.ctr_state(ctx.rws_host.data(), k), ctx.rl.ctr_state(ctx.rws_host.data(), k) + total, r.h_active + (size_t)b * total);
            if (r.h_info6) std::memcpy(r.h_info6 + (size_t)b * 6, ctx.rl.info(ctx.rws_host.data(), k), 6 * sizeof(int32_t));
            if (ctx.cycling) cycling_count[b] = ctx.rl.cyc(ctx.rws_host.data(), k)[CYC_COUNT];
            fin.keep_working_set_resident(b, ctx, k, r.prob[b].data, r.prob[b].var_index);
            return;
        }
        runner::LsiInfo info;
        runner::collect(*r.lsi[b], r.prob[b], x, &info, r.h_active ? r.h_active + (size_t)b * total : NULL, v);
        if (r.h_info6) std::memcpy(r.h_info6 + (size_t)b * 6, &info, sizeof(info));
        fin.keep_working_set(b, *r.lsi[b], r.prob[b].data, r.prob[b].var_index);
        keep_host_log(b, *r.lsi[b]);
        cycling_count[b] = static_cast<uint32_t>(r.lsi[b]->getCyclingCounter());
        if (r.step && ctx.on_device[k]) unpack_state(ctx.state_host.data() + (size_t)k * ctx.shape.SD, nVar, total, x, v);
    }
    void collect(Run &r)
    {
        if (r.step) // x and v of the instances whose state lives on the device
            for (uint32_t g = 0; g < nGroups; g++)
            {
                BatchCtx &ctx = *grp[g];
                if (hipMemcpyAsync(ctx.state_host.data(), ctx.d_state, 8 * (size_t)ctx.B * ctx.shape.SD, hipMemcpyDeviceToHost, ctx.stream) != hipSuccess ||
                    hipStreamSynchronize(ctx.stream) != hipSuccess)
                    throw Exception("download of the final state failed");
            }
        bool every_instance_resident = r.resident; // (then the job below is four small copies per instance)
        for (uint32_t g = 0; g < nGroups && every_instance_resident; g++)
            for (uint32_t k = 0; k < grp[g]->B && every_instance_resident; k++) every_instance_resident = grp[g]->is_resident[k] != 0;
        pool->run(batch, [&](uint32_t b) { collect_instance(r, b); }, every_instance_resident);
    }

    /// statistics of the run (lexls_lsi_batch_stats, h_rounds2) and, under LEXLS_LSI_TIMING, where its time went
    void report(Run &r)
    {
        int rounds_fs = 0, rounds_sens = 0, rounds_step = 0;
        double t_enq = 0.0, t_wait = 0.0;
        for (uint32_t g = 0; g < nGroups; g++)
        {
            rounds_fs += grp[g]->rounds_fs;
            rounds_sens += grp[g]->rounds_sens;
            rounds_step += grp[g]->rounds_step + grp[g]->rounds_resident;
            t_enq += grp[g]->t_enqueue;
            t_wait += grp[g]->t_wait;
        }
        if (r.sw.timing && r.resident) // prefix reuse: what the lock-step stages could and what a per-instance loop would save
        {
            long sumK = 0, cnt = 0, worstK = 0, worstN = -1;
            for (uint32_t g = 0; g < nGroups; g++)
                for (uint32_t k = 0; k < grp[g]->B; k++)
                    if (grp[g]->is_resident[k])
                    {
                        const int32_t *inf = grp[g]->rl.info(grp[g]->rws_host.data(), k);
                        sumK += inf[6], cnt += inf[7];
                        if (inf[7] > worstN) worstN = inf[7], worstK = inf[6];
                    }
            std::fprintf(stderr, "lexls_lsi_batch_solve: prefix reuse: %ld resident factorizations behind a working-set change, %.2f levels read back on average; the instance with the most (%ld): %.2f\n",
                         cnt, cnt ? (double)sumK / cnt : 0.0, worstN, worstN > 0 ? (double)worstK / worstN : 0.0);
        }
        if (r.sw.timing)
            std::fprintf(stderr, "lexls_lsi_batch_solve: setup = %.4f s reset / constraint upload + %.4f s LexLSI objects (batch created in %.4f s)\n", r.t_ctx, r.t_setup - r.t_ctx, t_create),
            std::fprintf(stderr, "lexls_lsi_batch_solve: total %.4f s = setup %.4f + enqueue %.4f + wait for the GPU %.4f + host logic %.4f + rest %.4f (%u groups, %d+%d stages, %d with the step on the device)\n",
                         BatchCtx::now() - r.t_begin, r.t_setup, t_enq, t_wait, r.t_host, BatchCtx::now() - r.t_begin - r.t_setup - t_enq - t_wait - r.t_host, nGroups,
                         rounds_fs, rounds_sens, rounds_step);
        if (r.h_rounds2) r.h_rounds2[0] = rounds_fs, r.h_rounds2[1] = rounds_sens;
        last_stats[0] = rounds_fs, last_stats[1] = rounds_sens, last_stats[2] = rounds_step, last_stats[3] = (int32_t)nGroups;
    }
};
