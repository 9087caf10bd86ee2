// Phase 1 of a lock-step LexLSI batch as device work (lsi_batch.h: run_phase1_device): what the host worker pool otherwise does over host LexLSI
// objects in front of the first resident stage.  With the default modify_* parameters and set_min_init_ctr_violation = true it is the three steps
// below; other values of those four (h_params slots 12 .. 15) make lsi_phase1_setup_hot_kernel the first of them, which repairs the working set of
// the guess against x0 (lsi_phase1_setup.h: p1_hot_working_set) before it forms the state.  use_phase1_v0 (slot 16) puts lsi_phase1_v0_kernel in the place of the second and third step: iteration 0 without a factorization
//     lsi_phase1_setup_kernel   checks, working set, stamps, counters, [x | v | A x] from x0, the first equality problem
//     l-QR + removal search     the stage every resident iteration runs (lexls_lse_factorize_solve, lexls_lse_sensitivity_*_resident)
//     lsi_phase1_finish_kernel  without x0: x = x_lse, A x, v; then iteration 0 = lsi_iterate_body, the resident iteration itself
// One wavefront per instance, four per workgroup, the LDS of lsi_iterate_kernel.  Included once, by lsi_batch_ctx.h.
#pragma once
#include "lexls_lsi_device.h"

namespace
{
    struct Phase1Args
    {
        ResidentArgs ra;
        const double *x0;     // B x n, or NULL: the instances start from the solution of their first equality problem
        const uint8_t *guess; // B x total, or NULL
        const double *v0;     // B x total, or NULL: with x0 the instances' v is this array as it stands (set_v0, objective.h:226-236); read only with x0
        uint32_t *fault;      // one word for the run: min over the faulty instances of (index in the batch) * 8 + P1_* code
        uint32_t first;       // index in the batch of this group's instance 0
        const uint8_t *mask;  // B bytes, or NULL (lexls_lsi_batch_set_instance_mask): 0 = the instance is skipped in this run
        const int32_t *limits; // B words, or NULL (lexls_lsi_batch_set_instance_max_factorizations): the instance's own factorization limit, <= 0 = none
        const uint32_t *obj_dims; // B x nObj words, or NULL (lexls_lsi_batch_set_instance_obj_dims): the rows every objective of the instance has, <= sh.dim[k]
        uint32_t hot;             // P1_HOT_* (lsi_phase1_setup.h): the run's hot-start options, 0 = the defaults (lsi_phase1_setup_kernel; else lsi_phase1_setup_hot_kernel)
    };

    /// byte b of an instance mask (NULL: every instance is solved).  The bytes are the caller's, rewritten in place between two runs and between two
    /// replays of a captured run: read where they lie by a vector load of every lane (volatile: never a load through the scalar cache)
    __device__ __forceinline__ uint32_t lsi_mask_byte(const uint8_t *mask, uint32_t b) { return mask ? (uint32_t) * reinterpret_cast<const volatile uint8_t *>(mask + b) : 1u; }

    /// the limit instance b runs under: its entry of the caller's array when that is 1 .. max_factorizations - 1, the run's parameter otherwise (an
    /// entry <= 0 is "no budget of its own"; the run's parameter bounds everyone: it is the persistent launch's loop count).  The words are the
    /// caller's, rewritten in place between runs and replays like the mask's bytes: a volatile vector load, never through the scalar cache
    __device__ __forceinline__ int32_t lsi_instance_limit(const int32_t *limits, uint32_t b, int32_t max_factorizations)
    {
        const int32_t L = *reinterpret_cast<const volatile int32_t *>(limits + b);
        return (L >= 1 && L < max_factorizations) ? L : max_factorizations;
    }

    /// count k of instance b (lexls_lsi_batch_set_instance_obj_dims).  The words are the caller's, rewritten in place between runs and replays like the
    /// mask's bytes: a volatile vector load, never through the scalar cache
    __device__ __forceinline__ uint32_t lsi_instance_obj_dim(const uint32_t *obj_dims, uint32_t b, uint32_t nObj, uint32_t k)
    {
        return *reinterpret_cast<const volatile uint32_t *>(obj_dims + (size_t)b * nObj + k);
    }

    /// Objective::initialize_Ax + initialize_v0 (objective.h:162-196, set_min_init_ctr_violation) for the x in x_s (LDS, n doubles), lane =
    /// constraint: st = [x | v | A x].  A x is apply_A's ordered chain per row (objective.h:435-455).  cs: the activation types (LDS).
    /// v0 (the instance's total doubles, or NULL): Objective::phase1 with v0_is_specified — A x is formed, initialize_v0 is not run, v is v0
    /// RAGGED, cnt: the instance's row counts (p1_rows) — the v and A x of an absent row are 0 (the slab may hold an earlier run's), nothing of it is
    /// read.  Without RAGGED cnt is not looked at, as in lsi_step_wave
    /// HOT: set_min_init_ctr_violation = false (P1_HOT_V_MIDPOINT) — the inactive rows take p1_initial_v's other branch (objective.h:188-191)
    template <bool RAGGED = false, bool HOT = false>
    __device__ __forceinline__ void lsi_phase1_state(const StepShape &sh, const double *data, const uint32_t *var_b, const double *x_s, const uint8_t *cs, double *st,
                                                     const double *v0 = nullptr, const uint32_t *cnt = nullptr)
    {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t n = sh.n, total = sh.total;
        for (uint32_t j = lane; j < n; j += 64) st[j] = x_s[j];
        for (uint32_t g = lane; g < total; g += 64)
        {
            uint32_t k = 0;
            while (k + 1 < sh.nObj && g >= sh.first[k + 1]) k++;
            const uint32_t dim = sh.dim[k], c = g - sh.first[k];
            if constexpr (RAGGED)
                if (c >= cnt[k]) // an absent row (cnt: wave-uniform)
                {
                    st[n + g]         = 0.0;
                    st[n + total + g] = 0.0;
                    continue;
                }
            const double *blk  = data + sh.off[k];
            double ax, lb, ub;
            if (sh.simple[k])
            {
                ax = x_s[var_b[c]];
                lb = blk[c];
                ub = blk[c + dim];
            }
            else
            {
                ax = 0.0;
                for (uint32_t j = 0; j < n; j++) ax = lexls::dfma(blk[c + (size_t)j * dim], x_s[j], ax);
                lb = blk[c + (size_t)n * dim];
                ub = blk[c + (size_t)(n + 1) * dim];
            }
            const uint32_t t = cs[g];
            double v;
            if (v0)
                v = v0[g];
            else if (HOT)
                v = p1_initial_v(t, ax, lb, ub, true, sh.tol_feasibility);
            else if (t == CTR_ACTIVE_LB)
                v = ax - lb;
            else if (t == CTR_ACTIVE_UB)
                v = ax - ub;
            else if (t != CTR_INACTIVE) // CTR_ACTIVE_EQ keeps the first loop's value (objective.h:164)
                v = ax - 0.5 * (lb + ub);
            else if (ax <= lb)
                v = ax - lb;
            else if (ax >= ub)
                v = ax - ub;
            else
                v = 0.0;
            st[n + g]         = v;
            st[n + total + g] = ax;
        }
    }

    /// dynamic LDS lsi_phase1_setup_kernel takes on top of the four wavefronts' slices when the run has row counts (Phase1Args::obj_dims)
    constexpr size_t P1_COUNTS_LDS = 4 * 4 * (size_t)STEP_MAX_OBJ;

    /// RAGGED: the run has row counts (p.obj_dims != NULL).  Without it nothing of them is compiled in: the kernel a batch without counts has always run
    /// HOT: the run's hot-start options are not the defaults (p.hot != 0).  With an x0 and no v0 lane 0 runs p1_hot_working_set behind the working set
    /// of the guess — on the copy of x0 in LDS, which P1_HOT_MODIFY_X rewrites; the caller's x0, guess and v0 are only read — and the state is formed
    /// from that copy.  Without HOT nothing of it is compiled in
    template <bool RAGGED, bool HOT = false>
    __device__ __forceinline__ void lsi_phase1_setup_body(const Phase1Args &p)
    {
        const ResidentArgs &a = p.ra;
        const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
        const uint32_t b    = blockIdx.x * 4 + wib;
        if (b >= a.B) return;
        const StepShape &sh  = a.sh;
        const uint32_t n = sh.n, total = sh.total;
        const ResidentView v = resident_view(a, b, wib);
        uint8_t *cls         = reinterpret_cast<uint8_t *>(v.dv_s);  // total bytes of the step's LDS, free here
        uint32_t *stamp_s    = reinterpret_cast<uint32_t *>(v.adx_s); // total words
        const uint8_t *guess = p.guess ? p.guess + (size_t)b * total : nullptr;

        // ---- the instance mask: the wavefront of instance 0 counts the skipped instances of the group — they are stopped from the start — into
        // `finished`, which it resets anyway (everything that counts on runs in later kernels) ----
        uint32_t nskip = 0;
        if (p.mask && b == 0)
            for (uint32_t i = 0; i < a.B; i += 64) nskip += (uint32_t)__popcll(__ballot(i + lane < a.B && lsi_mask_byte(p.mask, i + lane) == 0));
        if (lsi_mask_byte(p.mask, b) == 0) // (wave-uniform)
        {
            // A skipped instance: none of its data is read.  It is left as lsi_iterate_finish leaves a stopped one (not alive, passed over by the l-QR
            // and the removal search) with an empty working set, an empty equality problem and zero counters: what the host downloads of it and
            // what lexls_lsi_batch_get_lambda forms of it is an empty entry
            for (uint32_t k = lane; k < a.nObjL; k += 64) a.dims[(size_t)b * a.nObjL + k] = 0u;
            for (uint32_t r = lane; r < a.cap; r += 64) a.row_ld[(size_t)b * a.cap + r] = 0u;
            if (lane < STEP_MAX_OBJ) v.g_na[lane] = 0;
            if (lane < RESIDENT_INFO_STRIDE) v.info[lane] = lane == 0 ? (int32_t)TERMINATION_STATUS_UNKNOWN : 0;
            if (lane < RESIDENT_CYC_STRIDE) a.cyc[(size_t)b * RESIDENT_CYC_STRIDE + lane] = 0u;
            if (lane == 0)
            {
                a.nfixed[b] = 0u;
                a.alive[b]  = 0;
                a.skip[b]   = 1;
                a.objidx[b] = -1;
                if (b == 0) *a.finished = nskip;
            }
            return;
        }

        // ---- the instance's row counts: lane = objective, into LDS (STEP_MAX_OBJ words per wavefront behind the four wavefronts' slices: a launch
        // with counts asks for them, P1_COUNTS_LDS), where every lane and the serial part below read them.  A count above its capacity ends the
        // instance here: with it the rows to check are not even known ----
        const uint32_t *cnt = nullptr;
        if constexpr (RAGGED)
        {
            extern __shared__ double smem[];
            uint32_t *cnt_s = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(smem) + 4 * resident_lds_per_wave(sh.SD, total)) + wib * STEP_MAX_OBJ;
            bool above      = false;
            if (lane < sh.nObj)
            {
                const uint32_t c = lsi_instance_obj_dim(p.obj_dims, b, sh.nObj, lane);
                above            = c > sh.dim[lane];
                cnt_s[lane]      = c;
            }
            if (__ballot(above))
            {
                if (lane == 0) atomicMin(p.fault, (p.first + b) * 8u + (uint32_t)P1_OBJ_DIM);
                return;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            asm volatile("" ::: "memory");
            cnt = cnt_s;
        }

        // ---- the checks, lane = constraint (present rows only) ----
        uint32_t fault = 0xffffffffu;
        for (uint32_t g = lane; g < total; g += 64)
        {
            uint32_t k = 0;
            while (k + 1 < sh.nObj && g >= sh.first[k + 1]) k++;
            if constexpr (RAGGED)
                if (g - sh.first[k] >= cnt[k])
                {
                    cls[g] = 0;
                    continue;
                }
            const uint8_t rc = p1_row_class(sh, v.data, k, g - sh.first[k]);
            cls[g]           = rc;
            if (rc == P1_ROW_FAULT) fault = min(fault, (uint32_t)P1_LB_ABOVE_UB);
            if (guess && p1_guess_fault(guess[g]) != P1_OK) fault = min(fault, (uint32_t)P1_GUESS_TYPE);
        }
        for (uint32_t c = lane; c < (sh.dim0 ? p1_rows<RAGGED>(sh, cnt, 0) : 0u); c += 64) // (dim0: 0 without a simple-bounds objective)
        {
            const uint32_t f = p1_var_fault<RAGGED>(sh, v.var, c, cnt);
            if (f != P1_OK) fault = min(fault, f);
        }
        const uint32_t worst = (uint32_t)(-lexls::wave_maxi(-(int)min(fault, 0xffffu))); // (wave-uniform)
        if (worst != 0xffffu) // nothing more for a faulty instance: its variable indices may point anywhere
        {
            if (lane == 0) atomicMin(p.fault, (p.first + b) * 8u + worst);
            return;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        asm volatile("" ::: "memory");

        // ---- the working set: one lane, in the reference's order ----
        const bool repair = HOT && p.x0 && !p.v0 && (p.hot & (P1_HOT_MODIFY_X | P1_HOT_TYPE_ACTIVE | P1_HOT_TYPE_INACTIVE)); // (uniform over the launch)
        if constexpr (HOT)
            if (repair)
            {
                for (uint32_t j = lane; j < n; j += 64) v.dx_s[j] = p.x0[(size_t)b * n + j];
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                asm volatile("" ::: "memory");
            }
        if (lane == 0)
        {
            uint32_t next = 0;
            p1_build_working_set<RAGGED>(sh, cls, guess, v.cs, v.act, v.ina, v.ipos, v.na, stamp_s, &next, cnt);
            if constexpr (HOT)
                if (repair) p1_hot_working_set<RAGGED>(sh, v.data, v.var, v.dx_s, p.hot, v.cs, v.act, v.ina, v.ipos, v.na, stamp_s, &next, cls, cnt); // (cls is read no more: the marks)
            a.next_stamp[b] = next;
            a.alive[b]      = 1;
            a.skip[b]       = 0;
            a.objidx[b]     = 0; // the removal search runs behind the factorization (speculative)
            if (b == 0) *a.finished = nskip; // (0 without a mask)
            // the budget of this run is the one that stands in the caller's array now: every later kernel reads this copy (a skipped or a faulty
            // instance has returned above: its entry is not read)
            if (p.limits) a.inst_max_fact[b] = lsi_instance_limit(p.limits, b, a.max_factorizations);
        }
        // ... and so are its row counts (the LDS copy: the values the checks above were made with)
        if (RAGGED && lane < RESIDENT_DIMS_STRIDE) a.inst_dims[(size_t)b * RESIDENT_DIMS_STRIDE + lane] = lane < sh.nObj ? cnt[lane] : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        asm volatile("" ::: "memory");
        for (uint32_t g = lane; g < total; g += 64)
        {
            v.g_act[g]  = v.act[g];
            v.g_ina[g]  = v.ina[g];
            v.g_ipos[g] = v.ipos[g];
            v.g_cs[g]   = v.cs[g];
            if (v.cs[g]) a.stamp[(size_t)b * total + g] = stamp_s[g];
        }
        if (lane < STEP_MAX_OBJ) v.g_na[lane] = v.na[lane];
        if (lane < RESIDENT_INFO_STRIDE) v.info[lane] = lane == 0 ? (int32_t)TERMINATION_STATUS_UNKNOWN : 0; // counters zero, nothing factorized yet
        if (lane < RESIDENT_CYC_STRIDE) a.cyc[(size_t)b * RESIDENT_CYC_STRIDE + lane] = 0u;                  // the cycling handler has seen no event

        // ---- [x | v | A x] of a given x0 (without one: after the first solve, lsi_phase1_finish_kernel) ----
        if (p.x0)
        {
            if (!repair) // (with it the copy is there already, and may have been rewritten)
                for (uint32_t j = lane; j < n; j += 64) v.dx_s[j] = p.x0[(size_t)b * n + j];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            asm volatile("" ::: "memory");
            const double *v0 = p.v0 ? p.v0 + (size_t)b * total : nullptr;
            if (HOT && (p.hot & P1_HOT_V_MIDPOINT))
                lsi_phase1_state<RAGGED, HOT>(sh, v.data, v.var, v.dx_s, v.cs, v.st, v0, cnt);
            else
                lsi_phase1_state<RAGGED>(sh, v.data, v.var, v.dx_s, v.cs, v.st, v0, cnt);
        }

        // ---- the first equality problem ----
        const EqualityProblemSlab slab = {a.dims, a.nfixed, a.fixed_idx, a.fixed_val, a.row_src, a.row_ld, a.fixed_type, a.ctr_type};
        lsi_form_equality_problem(sh, a.off, a.nObjL, a.cap, b, v.data, v.var, v.na, v.act, v.cs, slab, lane, 64u);
    }

    __global__ __launch_bounds__(256) void lsi_phase1_setup_kernel(Phase1Args p)
    {
        if (p.obj_dims) // (uniform over the launch)
            lsi_phase1_setup_body<true>(p);
        else
            lsi_phase1_setup_body<false>(p);
    }

    /// ... of a run whose hot-start options are not the defaults (Phase1Args::hot != 0): a kernel of its own, so that the one above stays what it is
    __global__ __launch_bounds__(256) void lsi_phase1_setup_hot_kernel(Phase1Args p)
    {
        if (p.obj_dims) // (uniform over the launch)
            lsi_phase1_setup_body<true, true>(p);
        else
            lsi_phase1_setup_body<false, true>(p);
    }

    /// behind the first factorization and its removal search: iteration 0.  has_x0 == 0: phase 1 takes x = x_lse first (lexlsi.h:350-357), the step
    /// that follows is then dx = 0.  The rest is the resident iteration: nFactorizations = 1, the blocking test or the removal, iteration_finish
    /// with its termination tests, the next equality problem
    /// HOT: set_min_init_ctr_violation = false (P1_HOT_V_MIDPOINT) in a run without x0 — lsi_phase1_finish_hot_kernel; lsi_phase1_finish_kernel is what it was
    template <bool HOT>
    __device__ __forceinline__ void lsi_phase1_finish_body(const ResidentArgs &a, uint32_t has_x0)
    {
        const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
        const uint32_t b    = blockIdx.x * 4 + wib;
        if (b >= a.B) return;
        if (!a.alive[b]) return;
        if (!has_x0)
        {
            const ResidentView v = resident_view(a, b, wib);
            for (uint32_t j = lane; j < a.sh.n; j += 64) v.dx_s[j] = a.x_lse[(size_t)b * a.sh.n + j];
            for (uint32_t g = lane; g < a.sh.total; g += 64) v.cs[g] = v.g_cs[g];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            asm volatile("" ::: "memory");
            if (a.inst_dims) // (wave-uniform)
                lsi_phase1_state<true, HOT>(a.sh, v.data, v.var, v.dx_s, v.cs, v.st, nullptr, resident_counts(a, b));
            else
                lsi_phase1_state<false, HOT>(a.sh, v.data, v.var, v.dx_s, v.cs, v.st);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // the step reads the state back from memory
            asm volatile("" ::: "memory");
        }
        lsi_iterate_body(a, b, wib);
    }
    __global__ __launch_bounds__(256) void lsi_phase1_finish_kernel(ResidentArgs a, uint32_t has_x0) { lsi_phase1_finish_body<false>(a, has_x0); }
    __global__ __launch_bounds__(256) void lsi_phase1_finish_hot_kernel(ResidentArgs a, uint32_t has_x0) { lsi_phase1_finish_body<true>(a, has_x0); }

    /// use_phase1_v0 (lexlsi.h:880-915, :1175): behind the setup kernel, in place of the first stage and lsi_phase1_finish_kernel — iteration 0 without an
    /// equality problem solved.  The step is dx = 0 (the "solution" handed to lsi_step_wave is the state's own x), formStep and the blocking test
    /// run on it, the blocking constraint joins or nothing changes, and the next equality problem — the first one this run factorizes — is formed
    /// (lsi_iterate_finish<., true>)
    __global__ __launch_bounds__(256) void lsi_phase1_v0_kernel(ResidentArgs a)
    {
        const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
        const uint32_t b    = blockIdx.x * 4 + wib;
        if (b >= a.B) return;
        if (!a.alive[b]) return;
        const ResidentView v = resident_view(a, b, wib);
        resident_load_lists(a, v, lane);
        StepVerdict r;
        if (a.inst_dims) // (wave-uniform)
            lsi_step_wave<true>(a.sh, v.data, v.var, v.st, v.st, v.st, v.cs, v.ipos, v.dx_s, v.adx_s, v.dv_s, r.alpha, r.blk_obj, r.blk_ctr, r.blk_type, resident_counts(a, b));
        else
            lsi_step_wave(a.sh, v.data, v.var, v.st, v.st, v.st, v.cs, v.ipos, v.dx_s, v.adx_s, v.dv_s, r.alpha, r.blk_obj, r.blk_ctr, r.blk_type);
        lsi_iterate_finish<false, true>(a, b, wib, r);
    }

    /// where the results of a run go when the caller's arrays are device memory (lexls_lsi_batch_run_device); fix_var / fix_val: what
    /// lexls_lsi_batch_get_lambda needs of the active simple bounds (variable and bound, working-set order), NULL when it is not offered;
    /// cyc_count (B words, or NULL): the relaxations every instance's cycling handler did, from cyc (the handlers' slab; NULL: a run without
    /// cycling handling, zeros)
    struct ScatterArgs
    {
        StepShape sh;
        uint32_t B;
        const double *state, *cdata;
        const uint32_t *var;
        const uint8_t *ctr_state;
        const uint16_t *act, *na;
        const int32_t *info;
        double *x, *v;
        int32_t *info6;
        uint8_t *active;
        uint32_t *fix_var;
        double *fix_val;
        const uint32_t *cyc;
        uint32_t *cyc_count;
        const uint8_t *mask; // B bytes or NULL: the rows of an instance whose byte is 0 are not stored (lexls_lsi_batch_set_instance_mask)
    };
    __device__ __forceinline__ void lsi_result_scatter_body(const ScatterArgs &s)
    {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t b    = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (b >= s.B) return;
        if (lsi_mask_byte(s.mask, b) == 0) return; // a skipped instance: the caller's rows keep their bits
        const uint32_t n = s.sh.n, total = s.sh.total;
        const double *st = s.state + (size_t)b * s.sh.SD;
        for (uint32_t j = lane; j < n; j += 64) s.x[(size_t)b * n + j] = st[j];
        if (s.v)
            for (uint32_t g = lane; g < total; g += 64) s.v[(size_t)b * total + g] = st[n + g];
        if (s.active)
            for (uint32_t g = lane; g < total; g += 64) s.active[(size_t)b * total + g] = s.ctr_state[(size_t)b * total + g];
        if (s.info6 && lane < 6) s.info6[(size_t)b * 6 + lane] = s.info[(size_t)b * RESIDENT_INFO_STRIDE + lane];
        if (s.cyc_count && lane == 0) s.cyc_count[b] = s.cyc ? s.cyc[(size_t)b * RESIDENT_CYC_STRIDE + CYC_COUNT] : 0u;
        if (s.fix_var && s.sh.dim0)
        {
            const uint32_t d0 = s.sh.dim0, na0 = s.na[(size_t)b * RESIDENT_NA_STRIDE];
            const double *blk = s.cdata + (size_t)b * s.sh.per_data + s.sh.off[0];
            for (uint32_t i = lane; i < na0 && i < d0; i += 64)
            {
                const uint32_t c = s.act[(size_t)b * total + i], t = s.ctr_state[(size_t)b * total + c];
                s.fix_var[(size_t)b * d0 + i] = s.var[(size_t)b * d0 + c];
                s.fix_val[(size_t)b * d0 + i] = t == CTR_ACTIVE_LB ? blk[c] : blk[c + d0];
            }
        }
    }
    __global__ __launch_bounds__(256) void lsi_result_scatter_kernel(ScatterArgs s) { lsi_result_scatter_body(s); }

    /// lexls_lsi_batch_enqueue_device, at the head of the run in the caller's stream: the run's fault word says "no fault" (four words are kept for it)
    __global__ __launch_bounds__(64) void lsi_fault_reset_kernel(uint32_t *fault)
    {
        if (threadIdx.x < 4) fault[threadIdx.x] = 0xffffffffu;
    }
    /// ... and the group's rows of the working-set log are empty.  Kernels, where the synchronous run has hipMemsetAsync: a captured memset node did not
    /// keep its pattern over back-to-back replays of the graph on the MI355X runtime (the fault word read B * nVar), a kernel node does
    __global__ __launch_bounds__(256) void lsi_zero_words_kernel(uint32_t *p, size_t words)
    {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
    }
    /// lexls_lsi_batch_enqueue_device: nobody on the host has looked at the setup kernels' fault word (Phase1Args::fault, one word for the whole run, every
    /// group's setup kernel complete) when the rest of the run is enqueued, so the device acts on it.  Behind the setup kernel of a group: a run with
    /// an input error has every instance of the group stopped the way lsi_iterate_finish stops one (alive 0, skip 1, no removal search, counted as
    /// finished) — the l-QR, the removal sweep, lsi_phase1_finish_kernel and the persistent launch then pass over every instance
    __global__ __launch_bounds__(256) void lsi_phase1_gate_kernel(ResidentArgs a, const uint32_t *fault)
    {
        if (*fault == 0xffffffffu) return;
        const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
        if (b >= a.B) return;
        a.alive[b]  = 0;
        a.skip[b]   = 1;
        a.objidx[b] = -1;
        if (b == 0) *a.finished = a.B;
    }
    /// ... the multipliers of such a run (d_lambda): what lexls_lsi_batch_get_lambda's form_final_problem posts from the downloaded working sets, from
    /// the slabs where they live — instance b's final equality problem into the in slab (lsi_form_equality_problem on its final working set), not
    /// skipped, no removal search, and map = [nact (B) | pos (B x total)]: the user row of every active constraint in working-set order, for
    /// lsi_lambda_scatter_kernel.  One wavefront per instance.  A run with an input error posts EMPTY problems, skipped, with the ranks and first
    /// columns of a factorization of nothing (rank / fcol: the handle's arrays): the sweep of the multipliers, which passes over nobody, finds no rows.
    /// So does every instance an instance mask skips (mask: the group's bytes or NULL)
    __global__ __launch_bounds__(256) void lsi_lambda_form_kernel(ResidentArgs a, uint32_t *map, uint32_t *rank, uint32_t *fcol, const uint32_t *fault, const uint8_t *mask)
    {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t b    = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (b >= a.B) return;
        const StepShape &sh  = a.sh;
        const uint32_t total = sh.total;
        if (*fault != 0xffffffffu || lsi_mask_byte(mask, b) == 0)
        {
            for (uint32_t k = lane; k < a.nObjL; k += 64)
            {
                a.dims[(size_t)b * a.nObjL + k] = 0u;
                rank[(size_t)b * a.nObjL + k]   = 0u;
                fcol[(size_t)b * a.nObjL + k]   = 0u;
            }
            for (uint32_t r = lane; r < a.cap; r += 64) a.row_ld[(size_t)b * a.cap + r] = 0u;
            if (lane == 0)
            {
                a.nfixed[b] = 0u;
                a.skip[b]   = 1;
                a.objidx[b] = -1;
                map[b]      = 0u;
            }
            return;
        }
        const uint16_t *na = a.na + (size_t)b * RESIDENT_NA_STRIDE, *act = a.act + (size_t)b * total;
        const uint8_t *cs  = a.ctr_state + (size_t)b * total;
        const EqualityProblemSlab slab = {a.dims, a.nfixed, a.fixed_idx, a.fixed_val, a.row_src, a.row_ld, a.fixed_type, a.ctr_type};
        lsi_form_equality_problem(sh, a.off, a.nObjL, a.cap, b, a.cdata + (size_t)b * sh.per_data, a.var + (size_t)b * sh.dim0, na, act, cs, slab, lane, 64u);
        if (lane == 0) // (the lists are short)
        {
            uint32_t *pos = map + a.B + (size_t)b * total;
            uint32_t r    = 0;
            for (uint32_t k = 0; k < sh.nObj; k++)
                for (uint32_t i = 0; i < na[k] && r < total; i++) pos[r++] = sh.first[k] + act[sh.first[k] + i];
            map[b]      = r;
            a.skip[b]   = 0;
            a.objidx[b] = -1;
        }
    }
    /// ... and the scatter of such a run: with an input error nothing of the caller's arrays is written.  status (one word, or NULL; the launch of
    /// the batch's first group gets it): the fault word on both outcomes, 0xffffffff for a good run
    __global__ __launch_bounds__(256) void lsi_result_scatter_gated_kernel(ScatterArgs s, const uint32_t *fault, uint32_t *status)
    {
        const uint32_t f = *fault;
        if (status && blockIdx.x == 0 && threadIdx.x == 0) *status = f;
        if (f != 0xffffffffu) return;
        lsi_result_scatter_body(s);
    }
} // namespace
