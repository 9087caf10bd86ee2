// One group of a lock-step LexLSI batch: its equality-solver handle, streams, the pinned per-round blocks, the slabs of the device-side step
// and of the resident iterations, and the enqueueing of stages.  Included once, by lexls_lsi_capi.hip (it launches lsi_step_kernel / lsi_iterate_kernel).
#pragma once
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "lexls_internal.h"
#include "lexls_lsi_device.h" // StepShape / StepArgs / lsi_step_kernel, ResidentArgs / lsi_iterate_kernel (shared with the persistent iteration kernel)
#include "lsi_phase1_device.h" // lsi_phase1_setup_kernel / lsi_phase1_finish_kernel / lsi_result_scatter_kernel

namespace
{
    void hip_check(int rc)
    {
        if (rc != LEXLS_OK) throw Exception(std::string("liblexls_hip: ") + lexls_last_error());
    }

    /// The environment switches of the driver, read in two places only: these at the creation of a batch object ...
    struct CreateSwitches
    {
        static const char *env(const char *name, const char *unset)
        {
            const char *e = std::getenv(name);
            return e ? e : unset;
        }
        const bool resident = std::atoi(env("LEXLS_LSI_RESIDENT", "1")) != 0, device_step = std::atoi(env("LEXLS_LSI_DEVICE_STEP", "0")) != 0, spec_sens = std::atoi(env("LEXLS_LSI_SPECULATIVE_SENS", "1")) != 0,
                   prefix_reuse = std::atoi(env("LEXLS_LSI_PREFIX_REUSE", "1")) != 0, host_staging = std::getenv("LEXLS_LSI_HOST_STAGING") != nullptr;
        const char *const groups = std::getenv("LEXLS_LSI_GROUPS");                                   // NULL: not given
        const double pool_spin_seconds = 1e-6 * std::atof(env("LEXLS_POOL_SPIN_US", "300")); // diagnostic: 0 = the pool's workers sleep at once
    };
    /// ... and these once per lexls_lsi_batch_run / lexls_lsi_batch_get_lambda
    struct RunSwitches
    {
        const bool timing = std::getenv("LEXLS_LSI_TIMING") != nullptr;
        const bool stamps_dump = std::getenv("LEXLS_FUSED_STAMPS_DUMP") != nullptr; // (a -DLEXLS_FUSED_STAMPS build leaves its phase clocks in the multiplier buffer)
        const bool device_phase1 = std::atoi(CreateSwitches::env("LEXLS_LSI_DEVICE_PHASE1", "0")) != 0; // phase 1 of a resident run as device work (lsi_phase1_device.h)
    };

    /// typed window into a pinned block (the per-round arrays of a batch sit in blocks laid out like the handle's device slabs)
    template <class T>
    struct View
    {
        T *p     = NULL;
        size_t n = 0;
        void bind(void *base, uint64_t offset, size_t n_, T v)
        {
            p = reinterpret_cast<T *>(static_cast<char *>(base) + offset);
            n = n_;
            std::fill(p, p + n, v);
        }
        T *data() { return p; }
        T &operator[](size_t i) { return p[i]; }
        T *begin() { return p; }
        T *end() { return p + n; }
    };

    /// host array in pinned memory (hipHostMalloc): the per-round copies of a lock-step batch are enqueued, not waited for
    /// (lexls_lse_set_deferred_sync), so their sources / destinations must be DMA-able and stable until the round's synchronize
    template <class T>
    struct Pinned
    {
        T *p     = NULL;
        size_t n = 0;
        Pinned() {}
        Pinned(const Pinned &)            = delete;
        Pinned &operator=(const Pinned &) = delete;
        ~Pinned()
        {
            if (p) (void)hipHostFree(p);
        }
        void assign(size_t n_, T v)
        {
            if (p) (void)hipHostFree(p);
            p = NULL;
            if (hipHostMalloc((void **)&p, (n_ ? n_ : 1) * sizeof(T), hipHostMallocDefault) != hipSuccess) throw Exception("hipHostMalloc failed (lock-step LSI batch)");
            n = n_;
            std::fill(p, p + n, v);
        }
        T *data() { return p; }
        T &operator[](size_t i) { return p[i]; }
        T *begin() { return p; }
        T *end() { return p + n; }
    };

    /// elements of one objective's block in an instance's constraint data: [A | lb | ub], or [lb | ub] for simple bounds
    inline uint64_t objective_elems(uint32_t dim, int32_t type, uint32_t nVar) { return (uint64_t)dim * (type == 1 ? 2 : nVar + 2); }
    /// the per-objective part of a shape (nObj <= STEP_MAX_OBJ); returns the elements of one instance's constraint data
    inline uint64_t fill_shape(StepShape &sh, const uint32_t *dims, const int32_t *types, uint32_t nVar)
    {
        uint64_t o = 0;
        uint32_t f = 0;
        for (uint32_t k = 0; k < sh.nObj; k++)
        {
            sh.dim[k] = dims[k], sh.simple[k] = types[k] == 1, sh.first[k] = f, sh.off[k] = o;
            o += objective_elems(dims[k], types[k], nVar);
            f += dims[k];
        }
        return o;
    }

    /// Working-set slab of the device-side step, as lsi_step_kernel reads it (StepArgs): [mode B | ctr_state B x total | inact_pos (u16) B x total],
    /// every part 16-aligned.  base: the host mirror or the device slab.
    struct StepSlab
    {
        size_t total = 0, o_state = 0, o_pos = 0, bytes = 0;
        explicit StepSlab(size_t B = 0, size_t total_ = 0) : total(total_)
        {
            o_state = (B + 15) & ~size_t(15);
            o_pos   = (o_state + B * total + 15) & ~size_t(15);
            bytes   = o_pos + 2 * B * total;
        }
        uint8_t *mode(uint8_t *base) const { return base; }
        uint8_t *ctr_state(uint8_t *base, size_t b = 0) const { return base + o_state + b * total; }
        uint16_t *inact_pos(uint8_t *base, size_t b = 0) const { return reinterpret_cast<uint16_t *>(base + o_pos) + b * total; }
    };
    /// Slab of the resident iterations, as lsi_iterate_kernel reads it (ResidentArgs): ctr_state | alive | act | inact | inact_pos | na | info |
    /// finished | stamp | next_stamp | cyc, every part 256-aligned.  base: the host mirror or the device slab; b: the instance.  The activation stamps
    /// (deactivate_first_wrong_sign) follow the core: only a run with that rule uploads them (bytes_stamps), every other copy stops in front of them
    /// (bytes_core).  The cycling handlers' state (RESIDENT_CYC_STRIDE words per instance, laid out like info) comes last and travels, as a copy
    /// of its own each way, only in runs with cycling handling (o_cyc, bytes_cyc).
    struct ResidentSlab
    {
        size_t total = 0, o_alive = 0, o_act = 0, o_inact = 0, o_ipos = 0, o_na = 0, o_info = 0, o_fin = 0, o_stamp = 0, o_next = 0, o_cyc = 0, bytes_core = 0, bytes_stamps = 0,
               bytes_cyc = 0, bytes = 0;
        explicit ResidentSlab(size_t B = 0, size_t total_ = 0) : total(total_)
        {
            auto up  = [](size_t v) { return (v + 255) & ~size_t(255); };
            size_t o = up(B * total); // ctr_state at 0
            o_alive = o, o = up(o + B);
            o_act = o, o = up(o + 2 * B * total);
            o_inact = o, o = up(o + 2 * B * total);
            o_ipos = o, o = up(o + 2 * B * total);
            o_na = o, o = up(o + 2 * B * RESIDENT_NA_STRIDE);
            o_info = o, o = up(o + 4 * B * RESIDENT_INFO_STRIDE);
            o_fin = o, o = up(o + 16);
            bytes_core = o;
            o_stamp = o, o = up(o + 4 * B * total);
            o_next = o, o = up(o + 4 * B);
            bytes_stamps = o;
            o_cyc = o, o = up(o + 4 * B * RESIDENT_CYC_STRIDE);
            bytes_cyc = 4 * B * RESIDENT_CYC_STRIDE;
            bytes = o;
        }
        uint8_t *ctr_state(char *base, size_t b = 0) const { return reinterpret_cast<uint8_t *>(base) + b * total; }
        uint8_t *alive(char *base) const { return reinterpret_cast<uint8_t *>(base + o_alive); }
        uint16_t *act(char *base, size_t b = 0) const { return reinterpret_cast<uint16_t *>(base + o_act) + b * total; }
        uint16_t *inact(char *base, size_t b = 0) const { return reinterpret_cast<uint16_t *>(base + o_inact) + b * total; }
        uint16_t *inact_pos(char *base, size_t b = 0) const { return reinterpret_cast<uint16_t *>(base + o_ipos) + b * total; }
        uint16_t *na(char *base, size_t b = 0) const { return reinterpret_cast<uint16_t *>(base + o_na) + b * RESIDENT_NA_STRIDE; }
        int32_t *info(char *base, size_t b = 0) const { return reinterpret_cast<int32_t *>(base + o_info) + b * RESIDENT_INFO_STRIDE; }
        uint32_t *finished(char *base) const { return reinterpret_cast<uint32_t *>(base + o_fin); }
        uint32_t *stamp(char *base, size_t b = 0) const { return reinterpret_cast<uint32_t *>(base + o_stamp) + b * total; }
        uint32_t *next_stamp(char *base) const { return reinterpret_cast<uint32_t *>(base + o_next); }
        uint32_t *cyc(char *base, size_t b = 0) const { return reinterpret_cast<uint32_t *>(base + o_cyc) + b * RESIDENT_CYC_STRIDE; }
    };

    /// an instance's [x | v | A x] into its row of a state array (sh.SD doubles) ...
    inline void pack_state(double *st, const StepShape &sh, const dVectorType &x, const std::vector<internal::Objective> &obj)
    {
        for (uint32_t j = 0; j < sh.n; j++) st[j] = x(j);
        for (uint32_t k = 0; k < sh.nObj; k++)
        {
            const dVectorType &v = obj[k].get_v(), &ax = obj[k].get_Ax();
            for (uint32_t i = 0; i < sh.dim[k]; i++)
            {
                st[sh.n + sh.first[k] + i]            = v(i);
                st[sh.n + sh.total + sh.first[k] + i] = ax(i);
            }
        }
    }
    /// ... and x / v (NULL: not wanted) back out of one
    inline void unpack_state(const double *st, size_t n, size_t total, double *x, double *v)
    {
        std::copy(st, st + n, x);
        if (v) std::copy(st + n, st + n + total, v);
    }

    /// The one walk over an instance's working set (workingset.h order): active(k, a, ctr, type) for the a-th active constraint of objective k,
    /// inactive(k, i, ctr) for its i-th inactive one
    template <class A, class I>
    inline void walk_working_set(const std::vector<internal::Objective> &obj, uint32_t nObj, A &&active, I &&inactive)
    {
        for (uint32_t k = 0; k < nObj; k++)
        {
            for (Index a = 0; a < obj[k].getActiveCtrCount(); a++) active(k, a, obj[k].getActiveCtrIndex(a), obj[k].getActiveCtrType(a));
            for (Index i = 0; i < obj[k].getInactiveCtrCount(); i++) inactive(k, i, obj[k].getInactiveCtrIndex(i));
        }
    }

    /// a host driver's working-set log (getWorkingSetLog, lexlsi.h:739) into row b of log arrays of capacity `cap` per instance, in the row layout of
    /// lexls_lsi_debug::log; the count is the number of entries made, those beyond the capacity are dropped (runner::collect_debug does the same)
    inline void put_working_set_log(const std::vector<WorkingSetLogEntry> &wlog, uint32_t cap, size_t b, int32_t *log, double *alpha, uint32_t *count)
    {
        static_assert(RESIDENT_WLOG_FIELDS == LEXLS_LSI_LOG_FIELDS && LEXLS_LSI_LOG_OBJ_INDEX == 0 && LEXLS_LSI_LOG_CTR_INDEX == 1 && LEXLS_LSI_LOG_CTR_TYPE == 2 &&
                          LEXLS_LSI_LOG_CYCLING_DETECTED == 3 && LEXLS_LSI_LOG_RANK == 4,
                      "the record lsi_iterate_finish writes is the row include/lexls_hip.h declares");
        for (size_t i = 0; i < wlog.size() && i < cap; i++)
        {
            int32_t *e = log + (b * cap + i) * RESIDENT_WLOG_FIELDS;
            e[0]       = static_cast<int32_t>(wlog[i].obj_index);
            e[1]       = static_cast<int32_t>(wlog[i].ctr_index);
            e[2]       = static_cast<int32_t>(wlog[i].ctr_type);
            e[3]       = wlog[i].cycling_detected ? 1 : 0;
            e[4]       = static_cast<int32_t>(wlog[i].rank);
            alpha[b * cap + i] = wlog[i].alpha_or_lambda;
        }
        count[b] = static_cast<uint32_t>(wlog.size());
    }

    struct BatchCtx
    {
        lexls_lse_t h = NULL;
        hipStream_t stream = NULL; // every group of a lock-step batch has its own stream: group A's kernels run while group B's host logic does
        hipStream_t stream_sens = NULL; // the sensitivity kernel of a stage serves other instances than its l-QR kernel: they run side by side
        hipEvent_t ev_uploaded = NULL, ev_sens_done = NULL;
        hipEvent_t ev_joined = NULL; // lexls_lsi_batch_enqueue_device: this group's whole run is complete (made at the first such call)
        bool stage_fs = false, stage_sens = false; // what the stage in flight serves
        uint32_t B = 0, n = 0, nObjL = 0, cap = 0;
        size_t pstride = 0;
        std::vector<uint32_t> maxdim, totalrank;
        std::vector<double> x;
        lexls_round_layout lay;
        Pinned<char> in_block, out_block; // pinned mirrors of the handle's round slabs: ONE copy each per stage
        View<uint32_t> dims, nfixed, fixed_idx, row_src, row_ld, tr_dl; // row_src/row_ld: B x cap, where each LOD row comes from (device gather)
        View<double> fixed_val, maxabs, x_dl;
        double *lod = NULL; // B x cap x (n+1), PINNED: host-staging fallback, uploaded every active-set round
        View<uint8_t> fixed_type, ctr_type, skip;
        View<int32_t> sens, objidx;
        std::vector<double> reg_factor;        // B x nObjL regularization factors (host copy; uploaded when they change)
        int reg_type = 0;                      // LexLS::RegularizationType shared by the batch
        double reg_variable = 0.0;
        uint32_t reg_cg_iters = 10;
        std::atomic<bool> reg_dirty{false};
        bool gather = false;                   // constraint data resident on the device: only row references travel per round
        // ---- step of an iteration on the device (lsi_step_kernel) ----
        bool device_step = false;
        StepShape shape;
        double *d_state = NULL, *d_state_in = NULL, *d_res = NULL;
        uint32_t *d_var = NULL;
        uint8_t *d_wset = NULL;
        Pinned<double> state_host, res_host;       // B x SD (hand-over staging, final download), B x 4
        StepSlab wl;                               // layout of d_wset / wset_host
        Pinned<uint8_t> wset_host;
        std::vector<uint8_t> on_device;            // per instance: x / v / A x live on the device
        std::atomic<bool> handover{false};         // some instance put its state into state_host for the next stage
        bool spec_sens  = false; // every factorization is followed by its removal search in the same stage (results used if the step is not blocked)
        // ---- resident iterations (lsi_iterate_kernel): x / v / A x, the working sets and the counters of an instance live on the device ----
        bool resident = false; // buffers exist (the structure allows it)
        StepShape rshape;
        uint32_t r_off = 0;
        double *d_rstate = NULL;
        uint32_t *d_rvar = NULL;
        ResidentSlab rl; // layout of d_rws / rws_host
        char *d_rws = NULL;
        Pinned<char> rws_host;
        Pinned<double> rstate_host;
        Pinned<uint32_t> fin_host;
        std::vector<uint8_t> is_resident; // per instance: handed over to the device
        uint32_t n_resident  = 0;
        int rounds_resident  = 0;
        std::vector<int32_t> iterations_at_handover;
        int rounds_fs_at_handover = 0, rounds_sens_at_handover = 0;
        bool first_wrong_sign = false;     // this run removes by deactivate_first_wrong_sign: collecting removal searches, activation stamps
        uint8_t *d_wrong_sign = NULL;      // the handle's LEXLS_ARRAY_WRONG_SIGN
        Pinned<uint8_t> wrong_sign_host;   // B x (n + cap): the set of the last host-driven sensitivity stage (made at the first run with the rule)
        bool cycling = false;              // this run handles cycling on the device: handler state in the slab, relaxed bounds in the resident constraint data
        double cycling_relax_step = 0.0;
        uint32_t cycling_max_counter = 0;
        // ---- working-set log (lexls_lsi_batch_set_working_set_log): this group's rows of the batch's log slab, on the device and in the pinned
        // staging copy — laid out like the cycling state, per instance wlog_cap records / values and one counter.  NULL: logging is off ----
        uint32_t wlog_cap = 0;
        int32_t *d_wlog = NULL, *wlog_host = NULL;
        double *d_wlog_alpha = NULL, *wlog_alpha_host = NULL;
        uint32_t *d_wlog_count = NULL, *wlog_count_host = NULL;
        // ---- phase 1 on the device (lsi_phase1_device.h): no host objects, the slabs are written where they live ----
        bool phase1_on_device = false;     // this run: the first resident stage finds its problem in the device's in slab
        uint32_t *d_p1_fault = NULL;       // the setup kernel's error word
        Pinned<uint32_t> p1_fault_host;
        uint8_t *d_p1_guess = NULL;        // B x total / B x n: staging of a host caller's guess and x0 (made at the first run that needs them)
        double *d_p1_x0 = NULL;
        uint32_t *d_fix_var = NULL;        // B x dim0 each: the active simple bounds of a run whose data never was on the host (lexls_lsi_batch_get_lambda)
        double *d_fix_val = NULL;
        Pinned<uint32_t> fix_var_host;
        Pinned<double> fix_val_host;
        int32_t *d_inst_limit = NULL;      // B: every instance's factorization limit of this run (ResidentArgs::inst_max_fact), the setup kernel's copy
        bool inst_limits = false;          // this run has per-instance limits (lexls_lsi_batch_set_instance_max_factorizations): the resident kernels read d_inst_limit
        uint32_t *d_inst_dims = NULL;      // B x RESIDENT_DIMS_STRIDE: every instance's objective row counts of this run (ResidentArgs::inst_dims), the setup kernel's copy
        bool inst_dims = false;            // this run has per-instance row counts (lexls_lsi_batch_set_instance_obj_dims): the resident kernels read d_inst_dims
        bool fused_all = false, fused_refused = false; // the rest of the resident iterations is one persistent launch / the shape has none
        const char *resident_kernel = "";              // the kernel that served the resident iterations of this run (download_resident)
        int rounds_fs = 0, rounds_sens = 0, rounds_step = 0;
        double t_enqueue = 0, t_wait = 0; // seconds, reported when LEXLS_LSI_TIMING is set
        static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

        void create(int device, uint32_t B_, uint32_t n_, uint32_t nObjL_, const uint32_t *maxdim_, bool gather_, bool prefix_reuse)
        {
            gather = gather_, B = B_, n = n_, nObjL = nObjL_;
            maxdim.assign(maxdim_, maxdim_ + nObjL);
            cap = 0;
            for (uint32_t k = 0; k < nObjL; k++) cap += maxdim[k];
            pstride = (size_t)cap * (n + 1);
            hip_check(lexls_lse_create(&h, device, B, n, nObjL, maxdim.data()));
            if (prefix_reuse) hip_check(lexls_lse_set_prefix_reuse(h, 1)); // in the resident iterations; off: everything is factorized in every iteration
            if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&stream_sens, hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&ev_uploaded, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_sens_done, hipEventDisableTiming) != hipSuccess)
                throw Exception("hipStreamCreate / hipEventCreate failed (lock-step LSI batch)");
            hip_check(lexls_lse_set_stream(h, stream));
            hip_check(lexls_lse_round_layout(h, &lay));
            in_block.assign(lay.in_bytes, 0);
            out_block.assign(lay.out_bytes, 0);
            if (!gather) need_staging();
            reset();
        }

        /// host staging of whole problems (pinned, B x cap x (n+1)): only for runs without the device-side gather
        void need_staging()
        {
            if (lod) return;
            if (hipHostMalloc((void **)&lod, 8 * (size_t)B * pstride, hipHostMallocDefault) != hipSuccess) throw Exception("hipHostMalloc failed for the LSI staging buffer");
            std::memset(lod, 0, 8 * (size_t)B * pstride);
        }

        /// buffers of the device-side step for a batch of this structure (once per batch object)
        void create_step(const StepShape &sh)
        {
            shape = sh;
            wl    = StepSlab(B, sh.total);
            if (hipMalloc((void **)&d_state, 8 * (size_t)B * sh.SD) != hipSuccess || hipMalloc((void **)&d_state_in, 8 * (size_t)B * sh.SD) != hipSuccess ||
                hipMalloc((void **)&d_res, 8 * (size_t)B * 4) != hipSuccess || hipMalloc((void **)&d_var, 4 * (size_t)B * (sh.dim0 ? sh.dim0 : 1)) != hipSuccess ||
                hipMalloc((void **)&d_wset, wl.bytes) != hipSuccess)
                throw Exception("hipMalloc failed (device-side LSI step)");
            state_host.assign((size_t)B * sh.SD, 0.0);
            res_host.assign((size_t)B * 4, 0.0);
            wset_host.assign(wl.bytes, 0);
            on_device.assign(B, 0);
            device_step = true;
        }
        /// buffers of the resident iterations for a batch of this structure (once per batch object)
        void create_resident(const StepShape &sh, uint32_t off)
        {
            rshape = sh;
            r_off  = off;
            rl     = ResidentSlab(B, sh.total);
            if (hipMalloc((void **)&d_rstate, 8 * (size_t)B * sh.SD) != hipSuccess || hipMalloc((void **)&d_rws, rl.bytes) != hipSuccess ||
                hipMalloc((void **)&d_rvar, 4 * (size_t)B * (sh.dim0 ? sh.dim0 : 1)) != hipSuccess || hipMalloc((void **)&d_inst_limit, 4 * (size_t)B) != hipSuccess ||
                hipMalloc((void **)&d_inst_dims, 4 * (size_t)B * RESIDENT_DIMS_STRIDE) != hipSuccess)
                throw Exception("hipMalloc failed (resident LSI iterations)");
            rws_host.assign(rl.bytes, 0);
            rstate_host.assign((size_t)B * sh.SD, 0.0);
            fin_host.assign(4, 0u);
            is_resident.assign(B, 0);
            resident = true;
        }

        /// instance b (its equality problem of a regular iteration is formed and staged in the in block) leaves the host: state, working
        /// sets in list order (workingset.h) and counters go into the hand-over slabs
        template <class LSI>
        void hand_over(uint32_t b, const LSI &inst)
        {
            char *base = rws_host.data();
            pack_state(rstate_host.data() + (size_t)b * rshape.SD, rshape, inst.get_x(), inst.getObjectives());
            uint8_t *cs = rl.ctr_state(base, b);
            uint16_t *act = rl.act(base, b), *ina = rl.inact(base, b), *ip = rl.inact_pos(base, b), *na = rl.na(base, b);
            std::memset(cs, 0, rshape.total);
            for (uint32_t k = 0; k < rshape.nObj; k++) na[k] = static_cast<uint16_t>(inst.getObjectives()[k].getActiveCtrCount());
            walk_working_set(inst.getObjectives(), rshape.nObj, [&](uint32_t k, Index a, Index c, ConstraintActivationType t) { act[rshape.first[k] + a] = static_cast<uint16_t>(c), cs[rshape.first[k] + c] = static_cast<uint8_t>(t); },
                             [&](uint32_t k, Index i, Index c) { ina[rshape.first[k] + i] = static_cast<uint16_t>(c), ip[rshape.first[k] + c] = static_cast<uint16_t>(i); });
            int32_t *info = rl.info(base, b);
            info[0]       = static_cast<int32_t>(inst.getStatus());
            info[1]       = static_cast<int32_t>(inst.getIterationsCount());
            info[2]       = static_cast<int32_t>(inst.getActivationsCount());
            info[3]       = static_cast<int32_t>(inst.getDeactivationsCount());
            info[4]       = static_cast<int32_t>(inst.getFactorizationsCount());
            info[5]       = static_cast<int32_t>(totalrank[b]);
            info[6] = info[7] = 0; // prefix reuse: levels read back, summed over the resident factorizations; their number
            if (first_wrong_sign) // position in the reference's WS list = stamp (lexlsi.h: activate / deactivate keep that list ordered by activation)
            {
                uint32_t *stamp = rl.stamp(base, b);
                const std::vector<ConstraintInfo> &order = inst.getActivationOrder();
                for (size_t p = 0; p < order.size(); p++) stamp[rshape.first[order[p].get_obj_index()] + order[p].get_ctr_index()] = static_cast<uint32_t>(p);
                rl.next_stamp(base)[b] = static_cast<uint32_t>(order.size());
            }
            if (cycling) // iteration 0 ran on the host and may have told the handler of an ADD or a REMOVE: the device continues from there.  (No bound is
            {            // relaxed yet — a circle takes two changes, the host made at most one — so the uploaded constraint data is the handler's data.)
                const internal::CyclingHandler &ch = inst.getCyclingHandler();
                uint32_t *c                        = rl.cyc(base, b);
                std::fill(c, c + RESIDENT_CYC_STRIDE, 0u);
                c[CYC_VALID]     = ch.get_last_event().valid ? 1u : 0u;
                c[CYC_OPERATION] = static_cast<uint32_t>(ch.get_last_event().operation);
                c[CYC_OBJ]       = static_cast<uint32_t>(ch.get_last_event().what.obj_index);
                c[CYC_CTR]       = static_cast<uint32_t>(ch.get_last_event().what.ctr_index);
                c[CYC_TYPE]      = static_cast<uint32_t>(ch.get_last_event().what.ctr_type);
                c[CYC_COUNT]     = static_cast<uint32_t>(ch.get_counter());
                if (ch.get_counter() != 0) throw Exception("lexls_lsi_batch_run: a bound was relaxed before the instance became resident");
            }
            // what the instance logged on the host (iteration 0, with log_working_set_enabled) goes into its staging rows; the device counts on behind it
            if (wlog_host) put_working_set_log(inst.getWorkingSetLog(), wlog_cap, b, wlog_host, wlog_alpha_host, wlog_count_host);
            rl.alive(base)[b] = 1;
            is_resident[b]    = 1; // (its staged equality problem is served by the first resident stage, followed by its removal sweep)
        }

        ResidentArgs resident_args(int32_t max_factorizations)
        {
            ResidentArgs ra;
            std::memset(&ra, 0, sizeof(ra));
            void *d_out = NULL;
            hip_check(lexls_lse_device_ptr(h, LEXLS_ARRAY_X, &d_out)); // x is the head of the out slab (lexls_lse_round_layout)
            char *out = static_cast<char *>(d_out), *in = lexls_internal_round_in(h);
            ra.sh     = rshape;
            ra.B = B, ra.cap = cap, ra.nObjL = nObjL, ra.off = r_off;
            ra.max_factorizations = max_factorizations;
            ra.cdata     = lexls_internal_cdata_writable(h);
            ra.var       = d_rvar;
            ra.x_lse     = reinterpret_cast<const double *>(out + lay.x);
            ra.totalrank = reinterpret_cast<const uint32_t *>(out + lay.total_rank);
            ra.sens      = reinterpret_cast<const int32_t *>(out + lay.found);
            ra.state     = d_rstate;
            ra.ctr_state = rl.ctr_state(d_rws), ra.alive = rl.alive(d_rws), ra.act = rl.act(d_rws), ra.inact = rl.inact(d_rws), ra.inact_pos = rl.inact_pos(d_rws);
            ra.na = rl.na(d_rws), ra.info = rl.info(d_rws), ra.finished = rl.finished(d_rws);
            ra.dims      = reinterpret_cast<uint32_t *>(in + lay.dims);
            ra.nfixed    = reinterpret_cast<uint32_t *>(in + lay.nfixed);
            ra.fixed_idx = reinterpret_cast<uint32_t *>(in + lay.fixed_idx);
            ra.fixed_val = reinterpret_cast<double *>(in + lay.fixed_val);
            ra.skip      = reinterpret_cast<uint8_t *>(in + lay.skip);
            ra.objidx    = reinterpret_cast<int32_t *>(in + lay.obj_index);
            ra.row_src   = reinterpret_cast<uint32_t *>(in + lay.row_src);
            ra.row_ld    = reinterpret_cast<uint32_t *>(in + lay.row_ld);
            ra.fixed_type = reinterpret_cast<uint8_t *>(in + lay.fixed_type);
            ra.ctr_type   = reinterpret_cast<uint8_t *>(in + lay.ctr_type);
            ra.resume     = lexls_internal_resume_levels(h);
            ra.first_wrong_sign = first_wrong_sign ? 1u : 0u;
            ra.wrong_sign = d_wrong_sign, ra.stamp = rl.stamp(d_rws), ra.next_stamp = rl.next_stamp(d_rws);
            ra.cycling = cycling ? 1u : 0u, ra.cycling_max_counter = cycling_max_counter, ra.cycling_relax_step = cycling_relax_step, ra.cyc = rl.cyc(d_rws);
            ra.wlog = d_wlog, ra.wlog_alpha = d_wlog_alpha, ra.wlog_count = d_wlog_count, ra.wlog_cap = wlog_cap; // (NULL: off)
            ra.maxabs = reinterpret_cast<const double *>(out + lay.max_abs);
            ra.inst_max_fact = inst_limits ? d_inst_limit : NULL;
            ra.inst_dims     = inst_dims ? d_inst_dims : NULL;
            return ra;
        }

        /// the removal rule of the run that starts (deactivate_first_wrong_sign); the set's buffers are made at the first run that needs them
        void set_first_wrong_sign(bool on)
        {
            first_wrong_sign = on;
            if (!on || d_wrong_sign) return;
            void *p = NULL;
            hip_check(lexls_lse_device_ptr(h, LEXLS_ARRAY_WRONG_SIGN, &p));
            d_wrong_sign = static_cast<uint8_t *>(p);
            wrong_sign_host.assign((size_t)B * (n + cap), 0);
        }

        /// cycling handling of the run that starts (on: the resident iterations do it; a run that handles cycling on the host passes off)
        void set_cycling(bool on, double relax_step, uint32_t max_counter) { cycling = on, cycling_relax_step = relax_step, cycling_max_counter = max_counter; }

        /// this group's rows of the log slab (set_working_set_log of the batch object; NULL pointers: logging off)
        void bind_working_set_log(uint32_t cap_, int32_t *d_log, double *d_alpha, uint32_t *d_count, int32_t *h_log, double *h_alpha, uint32_t *h_count)
        {
            wlog_cap = cap_;
            d_wlog = d_log, d_wlog_alpha = d_alpha, d_wlog_count = d_count;
            wlog_host = h_log, wlog_alpha_host = h_alpha, wlog_count_host = h_count;
        }
        /// a run starts: no entries, every row zero (rows behind an instance's last entry stay zero) — in the group's stream, ahead of everything that logs
        void clear_working_set_log()
        {
            if (!d_wlog) return;
            if (hipMemsetAsync(d_wlog, 0, 4 * (size_t)B * wlog_cap * RESIDENT_WLOG_FIELDS, stream) != hipSuccess || hipMemsetAsync(d_wlog_alpha, 0, 8 * (size_t)B * wlog_cap, stream) != hipSuccess ||
                hipMemsetAsync(d_wlog_count, 0, 4 * (size_t)B, stream) != hipSuccess)
                throw Exception("hipMemsetAsync failed (working-set log)");
        }

        /// the same by kernels (lexls_lsi_batch_enqueue_device: no memset nodes in a captured run, lsi_zero_words_kernel)
        void clear_working_set_log_by_kernel()
        {
            if (!d_wlog) return;
            auto zero = [&](void *p, size_t words) {
                const size_t blocks = (words + 255) / 256;
                hipLaunchKernelGGL(lsi_zero_words_kernel, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, stream, static_cast<uint32_t *>(p), words);
            };
            zero(d_wlog, (size_t)B * wlog_cap * RESIDENT_WLOG_FIELDS);
            zero(d_wlog_alpha, 2 * (size_t)B * wlog_cap);
            zero(d_wlog_count, (size_t)B);
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_zero_words_kernel launch failed (working-set log)");
        }

        /// the handed-over instances start: slabs up, then `count` whole iterations are enqueued (nothing is waited for)
        void begin_resident()
        {
            *rl.finished(rws_host.data()) = 0u;
            if (hipMemcpyAsync(d_rws, rws_host.data(), first_wrong_sign ? rl.bytes_stamps : rl.bytes_core, hipMemcpyHostToDevice, stream) != hipSuccess ||
                (cycling && hipMemcpyAsync(d_rws + rl.o_cyc, rws_host.data() + rl.o_cyc, rl.bytes_cyc, hipMemcpyHostToDevice, stream) != hipSuccess) ||
                hipMemcpyAsync(d_rstate, rstate_host.data(), 8 * (size_t)B * rshape.SD, hipMemcpyHostToDevice, stream) != hipSuccess)
                throw Exception("hipMemcpyAsync failed (resident hand-over)");
            if (d_wlog && (hipMemcpyAsync(d_wlog, wlog_host, 4 * (size_t)B * wlog_cap * RESIDENT_WLOG_FIELDS, hipMemcpyHostToDevice, stream) != hipSuccess ||
                           hipMemcpyAsync(d_wlog_alpha, wlog_alpha_host, 8 * (size_t)B * wlog_cap, hipMemcpyHostToDevice, stream) != hipSuccess ||
                           hipMemcpyAsync(d_wlog_count, wlog_count_host, 4 * (size_t)B, hipMemcpyHostToDevice, stream) != hipSuccess))
                throw Exception("hipMemcpyAsync failed (working-set log hand-over)");
            rounds_resident = 0;
            fused_all       = false;
            fused_refused   = false; // (decided per run: the next one may be of another kind — plain / regularized — or under another LEXLS_LSI_NO_FUSED)
            rounds_fs_at_handover   = rounds_fs;
            rounds_sens_at_handover = rounds_sens;
            iterations_at_handover.assign(B, 0);
            for (uint32_t b = 0; b < B; b++) iterations_at_handover[b] = rl.info(rws_host.data(), b)[1];
        }
        void enqueue_resident(int count, double tolW, double tolC, int32_t max_factorizations)
        {
            const double t0        = now();
            const ResidentArgs ra  = resident_args(max_factorizations);
            for (int i = 0; i < count && !fused_all; i++)
            {
                if (rounds_resident == 0 && !phase1_on_device)
                    hip_check(lexls_internal_upload_round_trusted(h, in_block.data(), 1)); // the problems the host formed last
                else
                {
                    // every iteration that is left, of every instance, in ONE persistent launch (lsi_fused_impl.h) where the shape has one: an
                    // instance runs l-QR -> removal sweep -> iteration until it stops, at most max_factorizations times
                    if (!fused_refused)
                    {
                        const int rc = lexls_internal_resident_fused(h, rshape.dim0 ? 1 : 0, max_factorizations > 0 ? max_factorizations : 1, tolW, tolC, &ra, sizeof(ra));
                        if (rc == LEXLS_OK)
                        {
                            fused_all = true;
                            rounds_resident++, rounds_fs++, rounds_sens++;
                            break;
                        }
                        if (rc != 1) hip_check(rc);
                        fused_refused = true;
                    }
                    hip_check(lexls_internal_round_resident(h, rshape.dim0 ? 1 : 0)); // the problems lsi_iterate_kernel formed
                    lexls_internal_arm_resume(h);                                     // ... and the levels it found unchanged
                }
                hip_check(lexls_lse_factorize_solve(h, 1));
                hip_check(first_wrong_sign ? lexls_lse_sensitivity_collect_resident(h, tolW, tolC) : lexls_lse_sensitivity_resident(h, tolW, tolC)); // speculative: used when the step is not blocked
                hipLaunchKernelGGL(lsi_iterate_kernel, dim3((B + 3) / 4), dim3(256), 4 * resident_lds_per_wave(rshape.SD, rshape.total), stream, ra);
                if (hipGetLastError() != hipSuccess) throw Exception("lsi_iterate_kernel launch failed");
                rounds_resident++, rounds_fs++, rounds_sens++;
            }
            if (hipMemcpyAsync(fin_host.data(), rl.finished(d_rws), 4, hipMemcpyDeviceToHost, stream) != hipSuccess) throw Exception("hipMemcpyAsync failed (finished count)");
            t_enqueue += now() - t0;
        }
        /// waits for what is enqueued; true when every handed-over instance has stopped
        bool resident_done()
        {
            finish_stage();
            return fin_host[0] >= n_resident;
        }
        /// the phase clocks a -DLEXLS_FUSED_STAMPS build of the persistent launch leaves in the multiplier buffer
        void dump_stamps()
        {
            std::vector<double> lam((size_t)B * (n + cap));
            hip_check(lexls_lse_get_lambda(h, lam.data()));
            hip_check(lexls_lse_synchronize(h));
            double sum[6] = {0, 0, 0, 0, 0, 0}, most[6] = {0, 0, 0, 0, 0, 0};
            for (uint32_t b = 0; b < B; b++)
            {
                const double *o = lam.data() + (size_t)b * (n + cap);
                for (int i = 0; i < 6; i++) sum[i] += o[i];
                if (o[4] > most[4])
                    for (int i = 0; i < 6; i++) most[i] = o[i];
            }
            std::fprintf(stderr, "persistent launch, cycles per iteration [l-QR | step | removal search (per iteration) | finish], iterations, searches: all instances %.0f | %.0f | %.0f | %.0f, %.0f, %.0f; the longest-running one %.0f | %.0f | %.0f | %.0f, %.0f, %.0f\n",
                         sum[0] / sum[4], sum[1] / sum[4], sum[2] / sum[4], sum[3] / sum[4], sum[4], sum[5], most[0] / most[4], most[1] / most[4], most[2] / most[4], most[3] / most[4], most[4], most[5]);
        }
        /// with_state = false: x and v went from the device slab to device arrays of the caller (scatter_results)
        /// keep_kernel_name: resident_kernel was taken when the launch was enqueued (enqueue_fused; other factorizations have followed it since)
        void download_resident(bool stamps_dump, bool with_state = true, bool keep_kernel_name = false)
        {
            if (hipMemcpyAsync(rws_host.data(), d_rws, rl.bytes_core, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                (cycling && hipMemcpyAsync(rws_host.data() + rl.o_cyc, d_rws + rl.o_cyc, rl.bytes_cyc, hipMemcpyDeviceToHost, stream) != hipSuccess) || // the relaxations done
                (with_state && hipMemcpyAsync(rstate_host.data(), d_rstate, 8 * (size_t)B * rshape.SD, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
                hipStreamSynchronize(stream) != hipSuccess)
                throw Exception("download of the resident state failed");
            if (!keep_kernel_name) resident_kernel = lexls_lse_last_kernel(h); // the persistent launch, or the l-QR kernel of the last stage
            if (fused_all && stamps_dump) dump_stamps();
            if (fused_all) // the persistent launch: the stages it ran = the iterations of the instance that ran longest (statistics only)
            {
                int32_t most = 0;
                for (uint32_t b = 0; b < B; b++)
                    if (is_resident[b])
                    {
                        const int32_t d = rl.info(rws_host.data(), b)[1] - iterations_at_handover[b];
                        most            = d > most ? d : most;
                    }
                rounds_resident = most;
                rounds_fs       = rounds_fs_at_handover + most;
                rounds_sens     = rounds_sens_at_handover + most;
            }
        }
        uint8_t *mode() { return wl.mode(wset_host.data()); }

        /// Phase 1 as device work, first half: checks, working sets, stamps, counters, the state of a given x0 and the first equality problem, written
        /// by lsi_phase1_setup_kernel into the resident slabs and the in slab (what runner::setup + LexLSI::begin() + hand_over put there).
        /// d_x0 / d_guess / d_v0: device arrays of this group's instances or NULL (d_v0, the caller's initial residuals, is read where it lies and
        /// only together with d_x0); first: the group's first instance in the batch.  The constraint data
        /// and the variable indices are in the handle / d_rvar already (same stream).  The fault word comes back with the next synchronisation
        /// run_fault (lexls_lsi_batch_enqueue_device): the word of the whole run, shared by the groups and cleared by the caller — it stays on the device
        /// d_mask (lexls_lsi_batch_set_instance_mask): this group's bytes of the caller's instance mask or NULL, read by the kernel where they lie
        /// d_limits (lexls_lsi_batch_set_instance_max_factorizations): this group's words of the caller's limits or NULL; the kernel copies what counts
        /// for this run into d_inst_limit, which every later kernel of the run reads (resident_args)
        /// d_obj_dims (lexls_lsi_batch_set_instance_obj_dims): this group's rows of the caller's counts (B x nObj) or NULL; the kernel checks them against
        /// the capacities and copies them into d_inst_dims, likewise
        /// hot (P1_HOT_*, lsi_phase1_setup.h): the run's hot-start options where they act — with d_x0 and without d_v0; 0: lsi_phase1_setup_kernel as ever
        void enqueue_phase1_setup(const double *d_x0, const uint8_t *d_guess, uint32_t first, int32_t max_factorizations, const double *d_v0 = NULL, uint32_t *run_fault = NULL,
                                  const uint8_t *d_mask = NULL, const int32_t *d_limits = NULL, const uint32_t *d_obj_dims = NULL, uint32_t hot = 0)
        {
            const double t0 = now();
            if (!d_p1_fault && !run_fault)
            {
                if (hipMalloc((void **)&d_p1_fault, 16) != hipSuccess) throw Exception("hipMalloc failed (phase 1 on the device)");
                p1_fault_host.assign(4, 0xffffffffu);
            }
            hip_check(lexls_internal_ensure_gather_buffer(h));
            phase1_on_device = true;
            inst_limits      = d_limits != NULL;
            inst_dims        = d_obj_dims != NULL;
            Phase1Args pa;
            pa.ra = resident_args(max_factorizations);
            pa.x0 = d_x0, pa.guess = d_guess, pa.v0 = d_v0, pa.fault = run_fault ? run_fault : d_p1_fault, pa.first = first, pa.mask = d_mask, pa.limits = d_limits, pa.obj_dims = d_obj_dims;
            pa.hot = (d_x0 && !d_v0) ? hot : 0u;
            if (!run_fault && hipMemsetAsync(d_p1_fault, 0xff, 16, stream) != hipSuccess) throw Exception("hipMemsetAsync failed (phase 1 on the device)");
            if (pa.hot)
                hipLaunchKernelGGL(lsi_phase1_setup_hot_kernel, dim3((B + 3) / 4), dim3(256), 4 * resident_lds_per_wave(rshape.SD, rshape.total) + (d_obj_dims ? P1_COUNTS_LDS : 0), stream, pa);
            else
                hipLaunchKernelGGL(lsi_phase1_setup_kernel, dim3((B + 3) / 4), dim3(256), 4 * resident_lds_per_wave(rshape.SD, rshape.total) + (d_obj_dims ? P1_COUNTS_LDS : 0), stream, pa);
            if (hipGetLastError() != hipSuccess || (!run_fault && hipMemcpyAsync(p1_fault_host.data(), d_p1_fault, 4, hipMemcpyDeviceToHost, stream) != hipSuccess))
                throw Exception("lsi_phase1_setup_kernel launch failed");
            t_enqueue += now() - t0;
        }
        /// lexls_lsi_batch_enqueue_device, behind the setup kernel: a run whose fault word is set goes no further (lsi_phase1_gate_kernel)
        void enqueue_phase1_gate(const uint32_t *run_fault, int32_t max_factorizations)
        {
            hipLaunchKernelGGL(lsi_phase1_gate_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, resident_args(max_factorizations), run_fault);
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_phase1_gate_kernel launch failed");
        }
        /// ... and behind iteration 0 every iteration that is left, in the persistent launch: the caller has asked lexls_internal_resident_fused_serves
        void enqueue_fused(double tolW, double tolC, int32_t max_factorizations)
        {
            const ResidentArgs ra = resident_args(max_factorizations);
            const int rc          = lexls_internal_resident_fused(h, rshape.dim0 ? 1 : 0, max_factorizations > 0 ? max_factorizations : 1, tolW, tolC, &ra, sizeof(ra));
            if (rc == 1) throw Exception("lexls_lsi_batch_enqueue_device: the persistent launch was refused after lexls_internal_resident_fused_serves had accepted it");
            hip_check(rc);
            fused_all = true;
            rounds_resident++, rounds_fs++, rounds_sens++;
            resident_kernel = lexls_lse_last_kernel(h);
        }
        /// the books behind a device phase 1 (enqueue_phase1_stage, enqueue_phase1_v0): every instance is resident, iteration 0 was phase 1's
        void every_instance_resident_behind_iteration_0()
        {
            std::fill(is_resident.begin(), is_resident.end(), 1);
            n_resident      = B;
            rounds_resident = 0;
            fused_all = fused_refused = false;
            rounds_fs_at_handover   = rounds_fs;
            rounds_sens_at_handover = rounds_sens;
            iterations_at_handover.assign(B, 1); // iteration 0 belongs to phase 1
        }
        /// second half: the stage of every resident iteration on the first problem — row gather + l-QR, the speculative removal search — and
        /// lsi_phase1_finish_kernel (iteration 0).  Every instance is resident from here on; the count of stopped instances comes back
        /// (poll = false, lexls_lsi_batch_enqueue_device: nobody waits for the count)
        /// hot: as enqueue_phase1_setup's; without x0 the state is formed here, and P1_HOT_V_MIDPOINT is the one option that acts on it
        void enqueue_phase1_stage(bool has_x0, double tolW, double tolC, int32_t max_factorizations, bool poll = true, uint32_t hot = 0)
        {
            const double t0       = now();
            const ResidentArgs ra = resident_args(max_factorizations);
            hip_check(lexls_internal_round_resident(h, rshape.dim0 ? 1 : 0)); // (no resume levels: nothing has been factorized yet)
            hip_check(lexls_lse_factorize_solve(h, 1));
            hip_check(first_wrong_sign ? lexls_lse_sensitivity_collect_resident(h, tolW, tolC) : lexls_lse_sensitivity_resident(h, tolW, tolC));
            if (!has_x0 && (hot & P1_HOT_V_MIDPOINT))
                hipLaunchKernelGGL(lsi_phase1_finish_hot_kernel, dim3((B + 3) / 4), dim3(256), 4 * resident_lds_per_wave(rshape.SD, rshape.total), stream, ra, 0u);
            else
                hipLaunchKernelGGL(lsi_phase1_finish_kernel, dim3((B + 3) / 4), dim3(256), 4 * resident_lds_per_wave(rshape.SD, rshape.total), stream, ra, has_x0 ? 1u : 0u);
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_phase1_finish_kernel launch failed");
            rounds_fs++, rounds_sens++;
            if (poll && hipMemcpyAsync(fin_host.data(), rl.finished(d_rws), 4, hipMemcpyDeviceToHost, stream) != hipSuccess) throw Exception("hipMemcpyAsync failed (finished count)");
            every_instance_resident_behind_iteration_0();
            t_enqueue += now() - t0;
        }
        /// use_phase1_v0: in the place of enqueue_phase1_stage — no factorization, no removal search, lsi_phase1_v0_kernel (iteration 0 on dx = 0)
        void enqueue_phase1_v0(int32_t max_factorizations, bool poll = true)
        {
            const double t0       = now();
            const ResidentArgs ra = resident_args(max_factorizations);
            hipLaunchKernelGGL(lsi_phase1_v0_kernel, dim3((B + 3) / 4), dim3(256), 4 * resident_lds_per_wave(rshape.SD, rshape.total), stream, ra);
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_phase1_v0_kernel launch failed");
            if (poll && hipMemcpyAsync(fin_host.data(), rl.finished(d_rws), 4, hipMemcpyDeviceToHost, stream) != hipSuccess) throw Exception("hipMemcpyAsync failed (finished count)");
            every_instance_resident_behind_iteration_0();
            t_enqueue += now() - t0;
        }
        /// x / info / active / v of this group's instances from the slabs into device arrays of the caller (d_info6 / d_active / d_v may be NULL);
        /// with_fixed: the active simple bounds for lexls_lsi_batch_get_lambda as well (fix_var_host / fix_val_host, behind the next synchronisation);
        /// d_cyc_count (B words or NULL): the relaxations of every instance's cycling handler, zeros for a run without cycling handling
        /// run_fault (lexls_lsi_batch_enqueue_device): the run's fault word — with it set the kernel writes nothing but d_status (one word or NULL: the
        /// fault word, 0xffffffff for a good run), and nothing comes back to the host here (fetch_fixed_bounds, when the caller has waited)
        /// d_mask: this group's bytes of the instance mask or NULL — the rows of a skipped instance are not stored
        void scatter_results(double *d_x, int32_t *d_info6, uint8_t *d_active, double *d_v, bool with_fixed, uint32_t *d_cyc_count = NULL, const uint32_t *run_fault = NULL,
                             uint32_t *d_status = NULL, const uint8_t *d_mask = NULL)
        {
            with_fixed = with_fixed && rshape.dim0 != 0;
            if (with_fixed && !d_fix_var)
            {
                if (hipMalloc((void **)&d_fix_var, 4 * (size_t)B * rshape.dim0) != hipSuccess || hipMalloc((void **)&d_fix_val, 8 * (size_t)B * rshape.dim0) != hipSuccess)
                    throw Exception("hipMalloc failed (phase 1 on the device)");
                fix_var_host.assign((size_t)B * rshape.dim0, 0u);
                fix_val_host.assign((size_t)B * rshape.dim0, 0.0);
            }
            ScatterArgs sa;
            std::memset(&sa, 0, sizeof(sa));
            sa.sh = rshape, sa.B = B;
            sa.state = d_rstate, sa.cdata = lexls_internal_cdata(h), sa.var = d_rvar;
            sa.ctr_state = rl.ctr_state(d_rws), sa.act = rl.act(d_rws), sa.na = rl.na(d_rws), sa.info = rl.info(d_rws);
            sa.x = d_x, sa.v = d_v, sa.info6 = d_info6, sa.active = d_active;
            sa.fix_var = with_fixed ? d_fix_var : NULL, sa.fix_val = with_fixed ? d_fix_val : NULL;
            sa.cyc = cycling ? rl.cyc(d_rws) : NULL, sa.cyc_count = d_cyc_count;
            sa.mask = d_mask;
            if (run_fault)
                hipLaunchKernelGGL(lsi_result_scatter_gated_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, sa, run_fault, d_status);
            else
                hipLaunchKernelGGL(lsi_result_scatter_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, sa);
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_result_scatter_kernel launch failed");
            if (with_fixed && !run_fault && (hipMemcpyAsync(fix_var_host.data(), d_fix_var, 4 * (size_t)B * rshape.dim0, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                               hipMemcpyAsync(fix_val_host.data(), d_fix_val, 8 * (size_t)B * rshape.dim0, hipMemcpyDeviceToHost, stream) != hipSuccess))
                throw Exception("hipMemcpyAsync failed (active simple bounds)");
        }
        /// lexls_lsi_batch_enqueue_device with d_lambda, behind scatter_results: get_lambda's stage with the final equality problems formed on the device
        /// (lsi_lambda_form_kernel; d_map: the group's [nact | pos]) — rows gathered, factorized with the factor kept on a bit-exact kernel, every
        /// objective's multipliers in one sweep.  -> the multipliers (B x nObjL x (n + cap)) for lsi_lambda_scatter_kernel
        /// d_mask: this group's bytes of the instance mask or NULL — a skipped instance posts an empty problem
        const double *enqueue_lambda(int32_t max_factorizations, uint32_t *d_map, const uint32_t *run_fault, const uint8_t *d_mask = NULL)
        {
            void *d_rank = NULL, *d_fcol = NULL;
            hip_check(lexls_lse_device_ptr(h, LEXLS_ARRAY_RANK, &d_rank));
            hip_check(lexls_lse_device_ptr(h, LEXLS_ARRAY_FIRST_COL, &d_fcol));
            hipLaunchKernelGGL(lsi_lambda_form_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, resident_args(max_factorizations), d_map, static_cast<uint32_t *>(d_rank),
                               static_cast<uint32_t *>(d_fcol), run_fault, d_mask);
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_lambda_form_kernel launch failed");
            const int policy = lexls_internal_kernel_policy(h);
            hip_check(lexls_lse_set_kernel_policy(h, 5)); // bit-exact kernels whatever the shape (the factor of the reference's getLambda)
            int rc = lexls_internal_round_resident(h, rshape.dim0 ? 1 : 0);
            if (rc == LEXLS_OK) rc = lexls_lse_factorize(h);
            hip_check(lexls_lse_set_kernel_policy(h, policy));
            hip_check(rc);
            hip_check(lexls_lse_multipliers(h));
            const double *d_mult = lexls_internal_multipliers(h, NULL);
            if (!d_mult) throw Exception("lexls_lsi_batch_enqueue_device: no multipliers");
            return d_mult;
        }
        /// the active simple bounds scatter_results left on the device, for a caller that kept them there (enqueued; download_resident waits)
        void fetch_fixed_bounds()
        {
            if (!d_fix_var || !rshape.dim0) return;
            if (hipMemcpyAsync(fix_var_host.data(), d_fix_var, 4 * (size_t)B * rshape.dim0, hipMemcpyDeviceToHost, stream) != hipSuccess ||
                hipMemcpyAsync(fix_val_host.data(), d_fix_val, 8 * (size_t)B * rshape.dim0, hipMemcpyDeviceToHost, stream) != hipSuccess)
                throw Exception("hipMemcpyAsync failed (active simple bounds)");
        }
        /// a host caller's guess / x0 for the setup kernel: staged in device buffers of the group (NULL in, NULL out)
        const uint8_t *stage_guess(const uint8_t *h_guess)
        {
            if (!h_guess) return NULL;
            if (!d_p1_guess && hipMalloc((void **)&d_p1_guess, (size_t)B * rshape.total) != hipSuccess) throw Exception("hipMalloc failed (phase 1 on the device)");
            if (hipMemcpyAsync(d_p1_guess, h_guess, (size_t)B * rshape.total, hipMemcpyHostToDevice, stream) != hipSuccess) throw Exception("upload of the active-set guess failed");
            return d_p1_guess;
        }
        const double *stage_x0(const double *h_x0)
        {
            if (!h_x0) return NULL;
            if (!d_p1_x0 && hipMalloc((void **)&d_p1_x0, 8 * (size_t)B * n) != hipSuccess) throw Exception("hipMalloc failed (phase 1 on the device)");
            if (hipMemcpyAsync(d_p1_x0, h_x0, 8 * (size_t)B * n, hipMemcpyHostToDevice, stream) != hipSuccess) throw Exception("upload of x0 failed");
            return d_p1_x0;
        }

        /// per-solve state: what a freshly created context holds (a context serves many lexls_lsi_batch_run calls)
        void reset()
        {
            dims.bind(in_block.data(), lay.dims, (size_t)B * nObjL, 0);
            nfixed.bind(in_block.data(), lay.nfixed, B, 0);
            fixed_idx.bind(in_block.data(), lay.fixed_idx, (size_t)B * n, 0);
            fixed_val.bind(in_block.data(), lay.fixed_val, (size_t)B * n, 0.0);
            skip.bind(in_block.data(), lay.skip, B, 0);
            objidx.bind(in_block.data(), lay.obj_index, B, -1);
            row_src.bind(in_block.data(), lay.row_src, (size_t)B * cap, 0);
            row_ld.bind(in_block.data(), lay.row_ld, (size_t)B * cap, 0);
            fixed_type.bind(in_block.data(), lay.fixed_type, (size_t)B * n, static_cast<uint8_t>(CTR_ACTIVE_UB));
            ctr_type.bind(in_block.data(), lay.ctr_type, (size_t)B * cap, static_cast<uint8_t>(CTR_INACTIVE));
            x_dl.bind(out_block.data(), lay.x, (size_t)B * n, 0.0);
            tr_dl.bind(out_block.data(), lay.total_rank, B, 0);
            sens.bind(out_block.data(), lay.found, (size_t)B * 3, 0);
            maxabs.bind(out_block.data(), lay.max_abs, B, 0.0);
            if (lod) std::memset(lod, 0, 8 * (size_t)B * pstride);
            x.assign((size_t)B * n, 0.0);
            totalrank.assign(B, 0);
            reg_factor.assign((size_t)B * nObjL, 0.0);
            rounds_fs = rounds_sens = rounds_step = 0;
            t_enqueue = t_wait = 0.0;
            if (device_step)
            {
                std::fill(wset_host.begin(), wset_host.end(), 0);
                std::fill(on_device.begin(), on_device.end(), 0);
                handover.store(false);
            }
            stage_fs = stage_sens = false;
            phase1_on_device = false;
            inst_limits      = false;
            inst_dims        = false;
            if (resident)
            {
                std::fill(rws_host.begin(), rws_host.begin() + rl.bytes_core, 0); // (the stamps behind: hand_over writes every one a run reads)
                std::fill(is_resident.begin(), is_resident.end(), 0);
                n_resident      = 0;
                rounds_resident = 0;
            }
        }
        ~BatchCtx()
        {
            if (h) lexls_lse_destroy(h);
            void *dev[] = {d_state, d_state_in, d_res, d_var, d_wset, d_rstate, d_rvar, d_rws, d_p1_fault, d_p1_guess, d_p1_x0, d_fix_var, d_fix_val, d_inst_limit, d_inst_dims};
            for (void *q : dev)
                if (q) (void)hipFree(q);
            if (stream) (void)hipStreamDestroy(stream);
            if (stream_sens) (void)hipStreamDestroy(stream_sens);
            if (ev_uploaded) (void)hipEventDestroy(ev_uploaded);
            if (ev_sens_done) (void)hipEventDestroy(ev_sens_done);
            if (ev_joined) (void)hipEventDestroy(ev_joined);
            if (lod) (void)hipHostFree(lod);
        }

        /// working sets up, (state hand-over,) lsi_step_kernel, verdicts back: enqueued behind the equality solve of the stage
        void enqueue_step()
        {
            if (hipMemcpyAsync(d_wset, wset_host.data(), wl.bytes, hipMemcpyHostToDevice, stream) != hipSuccess) throw Exception("hipMemcpyAsync failed (working sets)");
            if (handover.exchange(false) &&
                hipMemcpyAsync(d_state_in, state_host.data(), 8 * (size_t)B * shape.SD, hipMemcpyHostToDevice, stream) != hipSuccess)
                throw Exception("hipMemcpyAsync failed (state hand-over)");
            void *d_x = NULL;
            hip_check(lexls_lse_device_ptr(h, LEXLS_ARRAY_X, &d_x));
            StepArgs sa;
            sa.sh        = shape;
            sa.B         = B;
            sa.cdata     = lexls_internal_cdata(h);
            sa.var       = d_var;
            sa.x_lse     = static_cast<const double *>(d_x);
            sa.state     = d_state;
            sa.state_in  = d_state_in;
            sa.mode = wl.mode(d_wset), sa.ctr_state = wl.ctr_state(d_wset), sa.inact_pos = wl.inact_pos(d_wset);
            sa.res       = d_res;
            hipLaunchKernelGGL(lsi_step_kernel, dim3((B + 3) / 4), dim3(256), 8 * (size_t)shape.SD * 4, stream, sa);
            if (hipGetLastError() != hipSuccess ||
                hipMemcpyAsync(res_host.data(), d_res, 8 * (size_t)B * 4, hipMemcpyDeviceToHost, stream) != hipSuccess)
                throw Exception("lsi_step_kernel launch / result copy failed");
        }

        /// Enqueue ONE stage on this group's stream: a batched factorize+solve for the instances with skip == 0 (if serve_fs) and a batched
        /// ObjectiveSensitivity for the instances with objidx >= 0 (if serve_sens) — disjoint sets of instances.  Nothing is waited for.
        void enqueue_stage(bool serve_fs, bool serve_sens, bool use_step, bool x_needed, double tolW, double tolC)
        {
            const double t0 = now();
            stage_fs   = serve_fs;
            stage_sens = serve_sens;
            if (serve_fs)
            {
                if (reg_type != 0 && reg_dirty.exchange(false)) // the factors are the same every round: uploaded once (this call synchronises)
                {
                    hip_check(lexls_lse_set_cg_iterations(h, reg_cg_iters));
                    hip_check(lexls_lse_set_regularization(h, reg_type, reg_factor.data(), 1, reg_variable));
                }
                // dims, fixed variables, types, skip flags, sensitivity levels and row references: one copy (+ the gather kernel)
                hip_check(lexls_internal_upload_round_trusted(h, in_block.data(), gather ? 1 : 0));
                if (serve_sens && hipEventRecord(ev_uploaded, stream) != hipSuccess) throw Exception("hipEventRecord failed");
                if (!gather) hip_check(lexls_lse_set_problem_host(h, lod));
                hip_check(lexls_lse_factorize_solve(h, 1));
                rounds_fs++;
                if (use_step) rounds_step++;
                if (use_step) enqueue_step(); // the step of the iteration, right behind its equality solve (same stream)
            }
            if (serve_sens)
            {
                if (serve_fs && !spec_sens)
                {
                    // disjoint instances (a problem is either re-factorised or asked for multipliers): the two kernels are both
                    // latency-bound at these batch sizes and share the chip — second stream, joined again before the download
                    if (hipStreamWaitEvent(stream_sens, ev_uploaded, 0) != hipSuccess) throw Exception("hipStreamWaitEvent failed");
                    hip_check(lexls_lse_set_stream(h, stream_sens));
                    hip_check(first_wrong_sign ? lexls_lse_sensitivity_collect_resident(h, tolW, tolC) : lexls_lse_sensitivity_resident(h, tolW, tolC));
                    hip_check(lexls_lse_set_stream(h, stream));
                    if (hipEventRecord(ev_sens_done, stream_sens) != hipSuccess || hipStreamWaitEvent(stream, ev_sens_done, 0) != hipSuccess)
                        throw Exception("hipEventRecord / hipStreamWaitEvent failed");
                }
                else if (serve_fs)
                    hip_check(first_wrong_sign ? lexls_lse_sensitivity_collect_resident(h, tolW, tolC) : lexls_lse_sensitivity_resident(h, tolW, tolC)); // behind the l-QR kernel: it reads the factors just made
                else
                    hip_check(first_wrong_sign ? lexls_lse_sensitivity_collect(h, objidx.data(), 0, tolW, tolC) : lexls_lse_sensitivity(h, objidx.data(), 0, tolW, tolC));
                // the set itself, for the instances whose removal search the host still runs (phase 1: SlotLSE::ObjectiveSensitivity)
                if (first_wrong_sign && hipMemcpyAsync(wrong_sign_host.data(), d_wrong_sign, (size_t)B * (n + cap), hipMemcpyDeviceToHost, stream) != hipSuccess)
                    throw Exception("hipMemcpyAsync failed (wrong-sign set)");
                rounds_sens++;
            }
            // x / total rank / sensitivity verdicts in one copy.  (The CORRECT_SIGN_OF_LAMBDA marks ObjectiveSensitivity leaves on the
            // device, lexlse.h:866-987, only matter between the levels of ONE removal search — which is one launch here,
            // lexls_lse_set_sensitivity_scan — so they never have to come back: the next equality problem sets every row's type anew.)
            if (x_needed || !serve_fs)
                hip_check(lexls_lse_download_round(h, out_block.data(), NULL));
            else
            {
                // every equality solve of this stage feeds a device-side step: x stays on the device, only the tail of the out slab
                // (total ranks, sensitivity verdicts) comes back
                void *d_out = NULL;
                hip_check(lexls_lse_device_ptr(h, LEXLS_ARRAY_X, &d_out)); // x is the head of the out slab (lexls_lse_round_layout)
                if (hipMemcpyAsync(out_block.data() + lay.total_rank, static_cast<char *>(d_out) + lay.total_rank, lay.out_bytes - lay.total_rank, hipMemcpyDeviceToHost,
                                   stream) != hipSuccess)
                    throw Exception("hipMemcpyAsync failed (results without x)");
            }
            t_enqueue += now() - t0;
        }

        /// wait for the stage in flight (the ONE synchronisation of a stage); its results are taken over per instance, on the worker pool
        void finish_stage()
        {
            const double t0 = now();
            hip_check(lexls_lse_synchronize(h));
            t_wait += now() - t0;
        }
        void take_solution(uint32_t b)
        {
            std::copy(x_dl.begin() + (size_t)b * n, x_dl.begin() + (size_t)(b + 1) * n, x.begin() + (size_t)b * n);
            totalrank[b] = tr_dl[b];
        }
    };
} // namespace
