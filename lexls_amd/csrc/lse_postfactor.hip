// The kernels behind a KEPT factor of the generic layout, one workgroup per problem: solve() alone, the residuals through Q, the objective
// sensitivity / multipliers, and the three least-norm solutions — with their launchers.  Like the factorization (lqr_generic.hip) they follow
// the reference statement by statement and evaluate every reduction in the order of the arithmetic contract (oracle/lexlse_oracle.h), so
// their results are bit-identical to the CPU oracle's (solve_generic's reciprocal form: the large path's tolerance contract).
#include "lexls_kernels.h"
#include "lexls_launch.h"
#include "lqr_wave_common.h"
#include "lqr_generic_steps.h"
#include "lexls_regularize.h" // (reg_scratch_doubles, reg_mu_doubles)
#include "lexls_sweep_impl.h"
#include "lse_kept_factor.h" // (stage_factor)
#include "lse_spd_solve.h"

#include <cstdlib>

namespace lexls
{
    namespace
    {
        // -----------------------------------------------------------------------------------------
        // solve() alone, from the factor in HBM
        // -----------------------------------------------------------------------------------------
        /// RECIP (the large path's step-per-pivot form, whose contract is values within 1e-10): a diagonal block's 64 reciprocals are formed
        /// at once, lane-parallel, and the chain multiplies — the division sequence (~400 cycles) sat on every one of the nVar dependent steps
        template <int NT, bool RECIP = false>
        __global__ __launch_bounds__(NT) void solve_generic_kernel(LseArgs a)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x;
#ifdef LEXLS_SOLVE_STAMPS
            long long sst[6] = {0, 0, 0, 0, 0, 0}, st0 = clock64();
#define SSTAMP(i) { const long long t_ = clock64(); sst[i] += t_ - st0; st0 = t_; }
#else
#define SSTAMP(i)
#endif
            const uint32_t n = a.nVar, cap = a.cap, nObj = a.nObj;
            const double *W  = a.fac + (size_t)b * cap * (n + 1);
            const size_t ld  = cap;
            double *xs       = smem;
            const uint32_t *dims = a.dims + (size_t)b * nObj;
            const uint32_t *rk = a.rank + (size_t)b * nObj, *fc = a.fcol + (size_t)b * nObj;
            const uint32_t *perm = a.perm + (size_t)b * n;
            const uint32_t nf    = a.nfixed ? a.nfixed[b] : 0;
            for (uint32_t i = tid; i < n; i += NT) xs[i] = (i < nf) ? a.fixed_val[(size_t)b * n + i] : 0.0;
            __syncthreads();
            uint32_t M = 0;
            for (uint32_t k = 0; k < nObj; k++) M += dims[k];
            uint32_t acc = 0, Fend = M;
            for (uint32_t k = nObj; k--;)
            {
                const uint32_t F = Fend - dims[k];
                Fend             = F;
                const uint32_t rank = rk[k];
                if (rank == 0) continue;
                const uint32_t Fc = fc[k];
                const uint32_t c0 = (acc > 0) ? fc[k + 1] : 0;
                for (uint32_t i = tid; i < rank; i += NT)
                {
                    double s = W[F + i + n * ld];
                    uint32_t j = 0;
                    if constexpr (NT >= 256) // (large levels: sixteen entries of the row requested together; the chain itself stays in order)
                    {
                        // (a batch = one trip to the stored factor, ~1.5 us: 64 entries per trip instead of 16 took the solve of configs[1] from
                        // 150 to NN us)
                        for (; j + 64 <= acc; j += 64)
                        {
                            double w64[64];
#pragma unroll
                            for (uint32_t u = 0; u < 64; u++) w64[u] = W[F + i + (c0 + j + u) * ld];
#pragma unroll
                            for (uint32_t u = 0; u < 64; u++) s = dfma(-w64[u], xs[c0 + j + u], s);
                        }
                        for (; j + 16 <= acc; j += 16)
                        {
                            double w16[16];
#pragma unroll
                            for (uint32_t u = 0; u < 16; u++) w16[u] = W[F + i + (c0 + j + u) * ld];
#pragma unroll
                            for (uint32_t u = 0; u < 16; u++) s = dfma(-w16[u], xs[c0 + j + u], s);
                        }
                    }
                    for (; j < acc; j++) s = dfma(-W[F + i + (c0 + j) * ld], xs[c0 + j], s);
                    xs[Fc + i] = s;
                }
                SSTAMP(0)
                if constexpr (NT >= 256)
                {
                    // Large levels: the triangular solve in blocks of 64 rows from the bottom.  ONE wavefront solves a diagonal block staged in
                    // LDS (lane = row; x_j by v_readlane: no workgroup barrier per variable), then every thread applies the block's 64 columns
                    // to a row above it.  Every x_i absorbs its columns in the same descending order as the unblocked loop: bit-identical.
                    constexpr uint32_t BS = 64, BL = 65;
                    double *Rb = xs + 2 * (size_t)n + 2; // BS x BL: the diagonal block, column-major, odd leading dimension
                    for (uint32_t jb = ((rank - 1) / BS) * BS;; jb -= BS)
                    {
                        const uint32_t nb = rank - jb < BS ? rank - jb : BS;
                        {
                            // thread = (row, column mod NT / 64) of the block: sixteen loads in flight per thread, no division per element
                            // (one element at a time behind "e % nb, e / nb" the staging took 6 us per block)
                            const uint32_t i = tid & 63u, j0 = tid >> 6;
                            constexpr uint32_t JS = NT / 64;
                            double st[BS / JS];
#pragma unroll
                            for (uint32_t u = 0; u < BS / JS; u++)
                            {
                                const uint32_t j = j0 + u * JS;
                                st[u]            = (i < nb && j < nb) ? W[F + jb + i + (Fc + jb + j) * ld] : 0.0;
                            }
#pragma unroll
                            for (uint32_t u = 0; u < BS / JS; u++)
                            {
                                const uint32_t j = j0 + u * JS;
                                if (i < nb && j < nb) Rb[i + j * BL] = st[u];
                            }
                        }
                        __syncthreads();
                        SSTAMP(1)
                        if (tid < 64)
                        {
                            // lane = row of the block, its entries ABOVE the diagonal in registers (zero from the diagonal down: the update
                            // below then needs no per-lane predicate — 64 of them, kept as 128 SGPRs, spilled), the chain fully unrolled: one
                            // step = x_j from lane j (v_readlane, constant lane) times the reciprocal diagonal (or divided), one fma for the
                            // rows above, lane j keeps x_j.  A lane's own entry is read before its step's fma can touch it.
                            double sv = tid < nb ? xs[Fc + jb + tid] : 0.0;
                            double rrow[BS];
#pragma unroll
                            for (uint32_t j = 0; j < BS; j++) rrow[j] = (tid < j && j < nb) ? Rb[tid + j * BL] : 0.0;
                            double dg = tid < nb ? Rb[tid * (BL + 1)] : 1.0; // this lane's diagonal entry (RECIP: its reciprocal)
                            if (RECIP) dg = 1.0 / dg;
                            double xfin = 0.0;
                            for_each_index<0, (int)BS>([&](auto jc) __attribute__((always_inline)) {
                                constexpr int j = (int)BS - 1 - decltype(jc)::value;
                                if ((uint32_t)j < nb) // (wave-uniform)
                                {
                                    const double xj = RECIP ? rdlane(sv, j) * rdlane(dg, j) : rdlane(sv, j) / rdlane(dg, j);
                                    sv              = dfma(-rrow[j], xj, sv);
                                    uint32_t tj = tid;
                                    asm volatile("" : "+v"(tj) : "v"(xj)); // (ties the lane test to the chain: sixty-four of them hoisted = 128 SGPRs, spilled)
                                    xfin = (tj == (uint32_t)j) ? xj : xfin;
                                }
                            });
                            sv = xfin;
                            if (tid < nb) xs[Fc + jb + tid] = sv;
                        }
                        __syncthreads();
                        SSTAMP(2)
                        for (uint32_t i = tid; i < jb; i += NT) // rows above the block: its columns, last first
                        {
                            double sv = xs[Fc + i];
                            uint32_t j = nb;
                            for (; j >= 64; j -= 64) // (a full block: its 64 entries of the row in ONE trip)
                            {
                                double w64[64];
#pragma unroll
                                for (uint32_t u = 0; u < 64; u++) w64[u] = W[F + i + (Fc + jb + j - 1 - u) * ld];
#pragma unroll
                                for (uint32_t u = 0; u < 64; u++) sv = dfma(-w64[u], xs[Fc + jb + j - 1 - u], sv);
                            }
                            for (; j >= 8; j -= 8)
                            {
                                double w8[8];
#pragma unroll
                                for (uint32_t u = 0; u < 8; u++) w8[u] = W[F + i + (Fc + jb + j - 1 - u) * ld];
#pragma unroll
                                for (uint32_t u = 0; u < 8; u++) sv = dfma(-w8[u], xs[Fc + jb + j - 1 - u], sv);
                            }
                            for (; j--;) sv = dfma(-W[F + i + (Fc + jb + j) * ld], xs[Fc + jb + j], sv);
                            xs[Fc + i] = sv;
                        }
                        __syncthreads();
                        SSTAMP(3)
                        if (jb == 0) break;
                    }
                }
                else
                {
                // the diagonal of R_k once into LDS; the column of the NEXT step is requested before the current step's division, so that a
                // step costs one division + one barrier instead of two dependent trips to the stored factor (same operations, same order)
                double *dgl = xs + n;
                for (uint32_t i = tid; i < rank; i += NT) dgl[i] = W[F + i + (Fc + i) * ld];
                double wcur = (rank >= 2 && tid + 1 < rank) ? W[F + tid + (Fc + rank - 1) * ld] : 0.0; // my row's entry of column rank-1
                __syncthreads();
                double xprev = 0.0;
                for (uint32_t j = rank; j--;)
                {
                    const double wnext = (j >= 1 && tid + 1 < j) ? W[F + tid + (Fc + j - 1) * ld] : 0.0;
                    if (j + 1 < rank && tid == 0) xs[Fc + j + 1] = xprev; // (nobody reads that entry any more in this loop)
                    const double xj = xs[Fc + j] / dgl[j];                 // every thread for itself: no hand-off
                    if (tid < j) xs[Fc + tid] = dfma(-wcur, xj, xs[Fc + tid]);
                    for (uint32_t i = tid + NT; i < j; i += NT) xs[Fc + i] = dfma(-W[F + i + (Fc + j) * ld], xj, xs[Fc + i]);
                    __syncthreads();
                    wcur  = wnext;
                    xprev = xj;
                }
                if (tid == 0) xs[Fc] = xprev;
                __syncthreads();
                }
                acc += rank;
            }
            // x = P x (lexlse.h:1044); scratch: the diagonal's place (free now), 16-byte aligned: xs = smem, an even number of doubles further on
            apply_permutation_by_following<NT>(a, b, perm, a.totalrank[b], xs, reinterpret_cast<uint32_t *>(xs + ((n + 1u) & ~1u)), tid);
            SSTAMP(4)
#ifdef LEXLS_SOLVE_STAMPS
            if (tid == 0)
                for (int i_ = 0; i_ < 5; i_++) a.lambda[(size_t)b * (n + cap) + 40 + i_] = (double)sst[i_];
#endif
        }

        // -----------------------------------------------------------------------------------------
        // get_v(): residuals through Q (lexlse.h:1560-1582)
        // -----------------------------------------------------------------------------------------
        template <int NT>
        __global__ __launch_bounds__(NT) void residual_kernel(LseArgs a)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x;
            const uint32_t n = a.nVar, cap = a.cap, nObj = a.nObj;
            const double *W  = a.fac + (size_t)b * cap * (n + 1);
            const double *hh = a.hh + (size_t)b * cap;
            double *v        = smem;       // cap
            double *bcast    = smem + cap; // 1
            const uint32_t *dims = a.dims + (size_t)b * nObj;
            for (uint32_t i = tid; i < cap; i += NT) v[i] = 0.0;
            __syncthreads();
            uint32_t F = 0;
            for (uint32_t k = 0; k < nObj; k++)
            {
                const uint32_t dim = dims[k], rank = a.rank[(size_t)b * nObj + k], Fc = a.fcol[(size_t)b * nObj + k];
                for (uint32_t i = rank + tid; i < dim; i += NT) v[F + i] = -W[F + i + (size_t)n * cap];
                __syncthreads();
                apply_q_block<NT>(W, cap, hh, F, Fc, dim, rank, v + F, bcast, tid);
                F += dim;
            }
            __syncthreads();
            for (uint32_t i = tid; i < cap; i += NT) a.v[(size_t)b * cap + i] = v[i];
        }

        // -----------------------------------------------------------------------------------------
        // ObjectiveSensitivity (lexlse.h:611-762) + findDescentDirection (:935-987)
        // -----------------------------------------------------------------------------------------
        struct SensState
        {
            double maxabs;
            uint32_t ctr;
            int obj, found;
        };

        /// scan one group of multipliers; sequential semantics of the reference (strict '<' keeps the first)
        __device__ void find_descent(uint8_t *types, const double *lambda, uint32_t count, double tolW, double tolC, int objTag, SensState *st)
        {
            for (uint32_t k = 0; k < count; k++)
            {
                const uint8_t t = types[k];
                if (t == CTR_ACTIVE_EQ || t == CORRECT_SIGN_OF_LAMBDA) continue;
                double al = lambda[k];
                if (t == CTR_ACTIVE_LB) al = -al;
                if (al > tolC)
                {
                    types[k] = CORRECT_SIGN_OF_LAMBDA;
                }
                else if (al < -tolW && al < st->maxabs)
                {
                    st->maxabs = al;
                    st->ctr    = k;
                    st->obj    = objTag;
                    st->found  = 1;
                }
            }
        }

        /// the collecting form (lexlse.h:866-910, deactivate_first_wrong_sign): same marks, and every wrong-sign multiplier of the group is noted in
        /// `mask` instead of the most negative one being kept; st->ctr counts them
        __device__ void collect_wrong_sign(uint8_t *types, const double *lambda, uint32_t count, double tolW, double tolC, uint8_t *mask, SensState *st)
        {
            for (uint32_t k = 0; k < count; k++)
            {
                const uint8_t t = types[k];
                if (t == CTR_ACTIVE_EQ || t == CORRECT_SIGN_OF_LAMBDA) continue;
                double al = lambda[k];
                if (t == CTR_ACTIVE_LB) al = -al;
                if (al > tolC)
                {
                    types[k] = CORRECT_SIGN_OF_LAMBDA;
                }
                else if (al < -tolW)
                {
                    mask[k] = 1;
                    st->ctr++;
                    st->found = 1;
                }
            }
        }

        /// collect != 0 (lexls_lse_sensitivity_collect): the wrong-sign SET of lexlse.h:511-602 goes to a.wrong_sign, sens = {set non-empty, entries,
        /// objective the search stopped at}, maxabs = 0
        template <int NT, bool STAGE>
        __global__ __launch_bounds__(NT) void sensitivity_kernel(LseArgs a, const int32_t *obj_index, int32_t obj_all, double tolW, double tolC, int scan_up, int collect)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x;
            const uint32_t n = a.nVar, cap = a.cap, nObj = a.nObj;
            const int32_t oi = obj_index ? obj_index[b] : obj_all;
            int32_t *sens    = a.sens + (size_t)b * 3;
            if (oi < 0 || (uint32_t)oi >= nObj)
            {
                if (tid == 0)
                {
                    sens[0]     = 0;
                    sens[1]     = -1;
                    sens[2]     = -2;
                    a.maxabs[b] = 0.0;
                }
                return;
            }
            const double *Wsrc  = a.fac + (size_t)b * cap * (n + 1);
            const double *hhsrc = a.hh + (size_t)b * cap;
            size_t ldsrc        = cap;
            uint8_t *types_l    = nullptr; // STAGE: LDS copy of the activation types (find_descent reads and marks one entry after the other)
            if (STAGE) // once per launch, shared by all the levels of a scan
            {
                // LDS: [LambdaFixed nVar | Lambda cap | rhs nVar | bcast | state | staged factor | Householder scalars]
                double *Wl  = smem + 2 * n + cap + 1 + (sizeof(SensState) + 7) / 8;
                double *hhl = Wl + (size_t)(cap | 1u) * (n + 1);
                for (uint32_t i = tid; i < cap; i += NT) hhl[i] = hhsrc[i]; // (every reflector of every level starts with its tau)
                types_l = reinterpret_cast<uint8_t *>(hhl + cap); // activation types: cap constraint rows, then nVar fixed variables
                for (uint32_t i = tid; i < cap; i += NT) types_l[i] = a.ctr_type[(size_t)b * cap + i];
                for (uint32_t i = tid; i < n; i += NT) types_l[cap + i] = a.fixed_type[(size_t)b * n + i];
                stage_factor<NT>(Wsrc, Wl, cap, n + 1, cap | 1u, tid);
                Wsrc  = Wl;
                hhsrc = hhl;
                ldsrc = cap | 1u;
            }
            // scan_up: what LexLSI's removal search does with one call per level (lexlsi.h:1121-1132) — levels oi, oi+1, ... until one
            // reports a wrong-sign multiplier or the last one is done — in ONE launch; the marks of a level are in place before the next
            for (uint32_t ObjIndex = (uint32_t)oi;; ObjIndex++)
            {
            const double *W  = Wsrc;
            const size_t ld  = ldsrc;
            const double *hh = hhsrc;
            const uint32_t *dims = a.dims + (size_t)b * nObj;
            const uint32_t *rk = a.rank + (size_t)b * nObj, *fc = a.fcol + (size_t)b * nObj;
            const uint32_t nf  = a.nfixed ? a.nfixed[b] : 0;
            uint8_t *ctr_type  = STAGE ? types_l : a.ctr_type + (size_t)b * cap;
            uint8_t *fix_type  = STAGE ? types_l + cap : a.fixed_type + (size_t)b * n;

            // LDS: [LambdaFixed nVar | Lambda cap | rhs nVar | bcast | state]
            double *LambdaFixed = smem;
            double *Lambda      = smem + n;
            double *rhs         = Lambda + cap;
            double *bcast       = rhs + n;
            SensState *st       = reinterpret_cast<SensState *>(bcast + 1);

            uint32_t nLambda = 0, Fobj = 0;
            for (uint32_t k = 0; k <= ObjIndex; k++)
            {
                if (k == ObjIndex) Fobj = nLambda;
                nLambda += dims[k];
            }
            for (uint32_t i = tid; i < n + cap + n; i += NT) smem[i] = 0.0;
            uint8_t *ws = collect ? a.wrong_sign + (size_t)b * (n + cap) : nullptr;
            if (collect) // (an objective is only looked at while the set is empty: cleared here, entries set by thread 0 behind the barrier)
                for (uint32_t i = tid; i < n + cap; i += NT) ws[i] = 0;
            if (tid == 0)
            {
                st->maxabs = 0.0;
                st->ctr    = 0;
                st->obj    = collect ? (int)ObjIndex : -2;
                st->found  = 0;
            }
            __syncthreads();

            uint32_t F = Fobj, Fc = fc[ObjIndex], dim = dims[ObjIndex], rank = rk[ObjIndex];
            if (a.reg_type == 7) // lexlse.h:647-651, :688-690 ("WARNING: TESTING" there): multipliers of the REGULARIZED problem
            {
                double *mu        = a.reg_mu + (size_t)b * reg_mu_doubles(n, nObj, cap);
                const double *res = mu + 2 * (size_t)nObj * n;
                if (tid == 0) // initialize_rhs (:1921-1959; oracle: initialize_rhs): ordered chains over at most nVar entries
                {
                    const double *X      = mu + (size_t)ObjIndex * n;
                    double *c            = mu + (size_t)(nObj + ObjIndex) * n; // X_mu_rhs.col(ObjIndex)
                    const uint32_t *perm = a.perm + (size_t)b * n;
                    const uint32_t TotalRank = a.totalrank[b];
                    const double f           = a.reg_factor[(size_t)b * nObj + ObjIndex];
                    for (uint32_t i = 0; i < n; i++) c[i] = X[i];
                    for (uint32_t k = 0; k < TotalRank; k++) // P' * .
                    {
                        const uint32_t j = perm[k];
                        const double t   = c[k];
                        c[k]             = c[j];
                        c[j]             = t;
                    }
                    for (uint32_t i = 0; i < n; i++) c[i] *= -f * f;
                    const uint32_t last = Fc + rank;
                    uint32_t Fk = 0, Fp = 0, nRank = 0;
                    for (uint32_t k = 0; k <= ObjIndex; k++)
                    {
                        const uint32_t Fck = fc[k], rkk = rk[k];
                        if (k > 0)
                        {
                            const uint32_t Fcp = fc[k - 1], rp = rk[k - 1], remain = last - Fck;
                            for (uint32_t j = 0; j < remain; j++)
                            {
                                double s = c[Fck + j];
                                for (uint32_t i = 0; i < rp; i++) s = dfma(-W[Fp + i + (Fck + j) * ld], c[Fcp + i], s);
                                c[Fck + j] = s;
                            }
                        }
                        for (uint32_t j = 0; j < rkk; j++) // R_k' z = c
                        {
                            double s = c[Fck + j];
                            for (uint32_t i = 0; i < j; i++) s = dfma(-W[Fk + i + (Fck + j) * ld], c[Fck + i], s);
                            c[Fck + j] = s / W[Fk + j + (Fck + j) * ld];
                        }
                        if (k < ObjIndex) nRank += rkk;
                        Fp = Fk;
                        Fk += dims[k];
                    }
                    for (uint32_t i = 0; i < nRank + nf; i++) rhs[i] = c[i];
                }
                for (uint32_t i = tid; i < dim; i += NT) Lambda[F + i] = res[F + i];
                __syncthreads();
            }
            else
            {
            for (uint32_t i = rank + tid; i < dim; i += NT) Lambda[F + i] = -W[F + i + n * ld];
            __syncthreads();
            if (STAGE && NT == 64 && dim <= 64)
                apply_q_wave(W, ld, hh, F, Fc, dim, rank, Lambda + F, tid);
            else
                apply_q_block<NT>(W, ld, hh, F, Fc, dim, rank, Lambda + F, bcast, tid);
            }
            if (tid == 0)
            {
                if (collect)
                    collect_wrong_sign(ctr_type + F, Lambda + F, dim, tolW, tolC, ws + n + F, st);
                else
                    find_descent(ctr_type + F, Lambda + F, dim, tolW, tolC, (int)ObjIndex, st);
            }

            if (ObjIndex > 0)
            {
                for (uint32_t c = tid; c < Fc; c += NT) // rhs.head(ColDim) -= L^T lambda (lexlse.h:706-707)
                {
                    rhs[c] -= chain_dot<8>(W + F + c * ld, Lambda + F, dim, 0.0);
                }
                __syncthreads();
                for (uint32_t k = ObjIndex; k--;)
                {
                    dim  = dims[k];
                    F    = F - dim;
                    Fc   = fc[k];
                    rank = rk[k];
                    for (uint32_t i = tid; i < rank; i += NT) Lambda[F + i] = rhs[Fc + i];
                    __syncthreads();
                    if (STAGE && NT == 64 && dim <= 64)
                        apply_q_wave(W, ld, hh, F, Fc, dim, rank, Lambda + F, tid);
                    else
                        apply_q_block<NT>(W, ld, hh, F, Fc, dim, rank, Lambda + F, bcast, tid);
                    for (uint32_t c = tid; c < Fc; c += NT)
                    {
                        rhs[c] -= chain_dot<8>(W + F + c * ld, Lambda + F, dim, 0.0);
                    }
                    if (tid == 0)
                    {
                        if (collect)
                            collect_wrong_sign(ctr_type + F, Lambda + F, dim, tolW, tolC, ws + n + F, st);
                        else
                            find_descent(ctr_type + F, Lambda + F, dim, tolW, tolC, (int)k, st);
                    }
                    __syncthreads();
                }
            }

            if (nf > 0) // lexlse.h:742-758
            {
                __syncthreads();
                for (uint32_t c = tid; c < nf; c += NT)
                {
                    double s = 0.0;
                    for (uint32_t i = 0; i < nLambda; i++) s = dfma(W[i + c * ld], Lambda[i], s);
                    LambdaFixed[c] = -s;
                }
                __syncthreads();
                if (tid == 0)
                {
                    // (collect: the reference's quirk, lexlse.h:599-600 — min(dims[0], nVarFixed) entries, the constraint multipliers Lambda[k])
                    if (collect)
                        collect_wrong_sign(fix_type, Lambda, dims[0] < nf ? dims[0] : nf, tolW, tolC, ws, st);
                    else
                        find_descent(fix_type, LambdaFixed, nf, tolW, tolC, -1, st);
                }
            }
            __syncthreads();

            double *out = a.lambda + (size_t)b * (n + cap);
            for (uint32_t i = tid; i < n + cap; i += NT)
            {
                double val = 0.0;
                if (i < nf)
                    val = LambdaFixed[i];
                else if (i < nf + nLambda)
                    val = Lambda[i - nf];
                out[i] = val;
            }
            if (tid == 0)
            {
                sens[0]     = st->found;
                sens[1]     = (st->found || collect) ? (int32_t)st->ctr : -1;
                sens[2]     = (st->found || collect) ? st->obj : -2;
                a.maxabs[b] = st->maxabs;
            }
            const int found = st->found; // (LDS, written before the last barrier)
            if (!scan_up || found || ObjIndex + 1 >= nObj) break;
            __syncthreads(); // the next level re-initialises the LDS arrays; its find_descent sees this level's marks (same thread)
            }
            if (STAGE) // the CORRECT_SIGN_OF_LAMBDA marks go back to the arrays lexls_lse_get_ctr_type / _fixed_type read
            {
                __syncthreads();
                for (uint32_t i = tid; i < cap; i += NT) a.ctr_type[(size_t)b * cap + i] = types_l[i];
                for (uint32_t i = tid; i < n; i += NT) a.fixed_type[(size_t)b * n + i] = types_l[cap + i];
            }
        }

        // -----------------------------------------------------------------------------------------
        // solveLeastNorm_1(): Givens sweep (lexlse.h:1052-1131).  Per problem `scratch` holds
        // RT (nVar x nVar, ld = nVar) followed by the rotation table (c,s pairs, <= nVar^2/2 doubles).
        // -----------------------------------------------------------------------------------------
        __device__ __forceinline__ void make_givens(double p2, double q, double &c, double &s)
        {
            if (q == 0.0)
            {
                c = p2 < 0.0 ? -1.0 : 1.0;
                s = 0.0;
            }
            else if (p2 == 0.0)
            {
                c = 0.0;
                s = q < 0.0 ? 1.0 : -1.0;
            }
            else if (fabs(p2) > fabs(q))
            {
                const double t = q / p2;
                double u       = sqrt(dfma(t, t, 1.0));
                if (p2 < 0.0) u = -u;
                c = 1.0 / u;
                s = -t * c;
            }
            else
            {
                const double t = p2 / q;
                double u       = sqrt(dfma(t, t, 1.0));
                if (q < 0.0) u = -u;
                s = -1.0 / u;
                c = -t * s;
            }
        }

        /// one problem's kept factor as the three least-norm routines read it: the factor and its level lists, the transpositions, and the split of
        /// the variables into nf fixed, nVarRank ranked and nVarFree free ones (ncol = nVarRank + nVarFree columns of [R T])
        struct LeastNormView
        {
            const double *W; // cap x (nVar + 1), column-major, ld = cap
            size_t ld;
            const uint32_t *dims, *rk, *fc, *perm;
            uint32_t n, nObj, nf, nVarRank, nVarFree, ncol;
        };
        __device__ __forceinline__ LeastNormView leastnorm_view(const LseArgs &a, uint32_t b)
        {
            const uint32_t n = a.nVar, cap = a.cap, nObj = a.nObj;
            LeastNormView v{a.fac + (size_t)b * cap * (n + 1), cap, a.dims + (size_t)b * nObj, a.rank + (size_t)b * nObj, a.fcol + (size_t)b * nObj, a.perm + (size_t)b * n, n, nObj,
                            a.nfixed ? a.nfixed[b] : 0, 0, 0, 0};
            for (uint32_t k = 0; k < nObj; k++) v.nVarRank += v.rk[k];
            v.nVarFree = n - (v.nVarRank + v.nf);
            v.ncol     = v.nVarRank + v.nVarFree;
            return v;
        }
        /// the compact [R T | rhs] copy (lexlse.h:1081-1094, :1166-1177): the levels' ranked rows one under the other into RT (leading dimension
        /// lr), their right-hand sides into rhs_dst.  No barrier
        template <int NT>
        __device__ __forceinline__ void leastnorm_compact_copy(const LeastNormView &v, double *RT, size_t lr, double *rhs_dst, uint32_t tid)
        {
            const double *W = v.W;
            const size_t ld = v.ld;
            uint32_t counter = 0, col_dim = v.ncol, F = 0;
            for (uint32_t k = 0; k < v.nObj; k++)
            {
                const uint32_t rank = v.rk[k], Fc = v.fc[k];
                for (uint32_t e = tid; e < rank * col_dim; e += NT)
                {
                    const uint32_t i = e % rank, j = e / rank;
                    if (j >= i) RT[counter + i + (counter + j) * lr] = W[F + i + (Fc + j) * ld];
                }
                for (uint32_t i = tid; i < rank; i += NT) rhs_dst[counter + i] = W[F + i + v.n * ld];
                counter += rank;
                col_dim -= rank;
                F += v.dims[k];
            }
        }
        /// x_rank = rhs - T_LOD x_free (lexlse.h:1193-1204) on xs = x by position, the free variables' values in place.  No barrier
        template <int NT>
        __device__ __forceinline__ void leastnorm_x_rank(const LeastNormView &v, double *xs, uint32_t tid)
        {
            const double *W = v.W;
            const size_t ld = v.ld;
            const uint32_t nf = v.nf, c0 = v.nf + v.nVarRank;
            uint32_t counter = 0, F = 0;
            for (uint32_t k = 0; k < v.nObj; k++)
            {
                const uint32_t rank = v.rk[k];
                for (uint32_t i = tid; i < rank; i += NT)
                {
                    double acc = 0.0;
                    for (uint32_t c = 0; c < v.nVarFree; c++) acc = dfma(W[F + i + (size_t)(c0 + c) * ld], xs[c0 + c], acc);
                    xs[nf + counter + i] = W[F + i + v.n * ld] - acc;
                }
                counter += rank;
                F += v.dims[k];
            }
        }

        template <int NT>
        __global__ __launch_bounds__(NT) void leastnorm_kernel(LseArgs a)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x;
            const LeastNormView v = leastnorm_view(a, b);
            const uint32_t n = v.n, nf = v.nf, nVarRank = v.nVarRank, nVarFree = v.nVarFree, ncol = v.ncol;
            double *RT              = a.scratch + (size_t)b * 2 * n * n; // nVarRank x ncol, ld = n
            double *rot             = RT + (size_t)n * n;               // (c, s) pairs in sweep order
            const size_t lr         = n;
            double *rhs             = smem;         // n
            double *xs              = smem + n;     // n
            double *cs              = smem + 2 * n; // 2

            for (uint32_t e = tid; e < n * n; e += NT) RT[e] = 0.0;
            for (uint32_t i = tid; i < n; i += NT)
            {
                rhs[i] = 0.0;
                xs[i]  = (i < nf) ? a.fixed_val[(size_t)b * n + i] : 0.0;
            }
            __syncthreads();
            leastnorm_compact_copy<NT>(v, RT, lr, rhs, tid);
            __syncthreads();

            uint32_t nrot = 0;
            for (uint32_t i = 0; i < nVarFree; i++) // zero T against R from the right (lexlse.h:1099-1110)
            {
                for (uint32_t j = nVarRank; j--;)
                {
                    if (tid == 0)
                    {
                        double c, s;
                        make_givens(RT[j + j * lr], RT[j + (nVarRank + i) * lr], c, s);
                        cs[0]             = c;
                        cs[1]             = s;
                        rot[2 * nrot]     = c;
                        rot[2 * nrot + 1] = s;
                    }
                    __syncthreads();
                    const double c = cs[0], s = cs[1];
                    for (uint32_t r = tid; r <= j; r += NT) // applyOnTheRight on RT.topRows(j+1)
                    {
                        const double x1 = RT[r + j * lr], y1 = RT[r + (nVarRank + i) * lr];
                        RT[r + j * lr]              = dfma(c, x1, -(s * y1));
                        RT[r + (nVarRank + i) * lr] = dfma(c, y1, s * x1);
                    }
                    nrot++;
                    __syncthreads();
                }
            }

            for (uint32_t j = nVarRank; j--;) // R^-1 rhs, column-oriented (lexlse.h:1115)
            {
                if (tid == 0) rhs[j] = rhs[j] / RT[j + j * lr];
                __syncthreads();
                const double xj = rhs[j];
                for (uint32_t i = tid; i < j; i += NT) rhs[i] = dfma(-RT[i + j * lr], xj, rhs[i]);
                __syncthreads();
            }

            if (tid == 0)
            {
                for (uint32_t k = nrot; k--;) // replay on the RHS in reverse (lexlse.h:1121-1124)
                {
                    const uint32_t fi = k / nVarRank, jj = nVarRank - 1 - (k % nVarRank);
                    const uint32_t gi = jj, gj = nVarRank + fi;
                    const double c = rot[2 * k], s = rot[2 * k + 1];
                    const double x1 = rhs[gi], y1 = rhs[gj];
                    rhs[gi] = dfma(c, x1, s * y1);
                    rhs[gj] = dfma(c, y1, -(s * x1));
                }
                for (uint32_t i = 0; i < ncol; i++) xs[nf + i] = rhs[i]; // lexlse.h:1129
            }
            __syncthreads();
            // x = P x (lexlse.h:1044).  Scratch: rhs' place (smem itself: 16-byte aligned), copied into xs above
            apply_permutation_by_following<NT>(a, b, v.perm, a.totalrank[b], xs, reinterpret_cast<uint32_t *>(rhs), tid);
        }
        /// solveLeastNorm_2 (lexlse.h:1138-1213): least-norm solution through the normal equations of the free variables.
        /// One 64-lane workgroup per problem on the factor in HBM; [R T | rhs] and D live in the per-problem scratch.
        /// Arithmetic order as oracle/lexlse_oracle.h::solveLeastNorm_2 (bit-identical).
        template <int NT>
        __global__ __launch_bounds__(NT) void leastnorm2_kernel(LseArgs a)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x;
            const LeastNormView v = leastnorm_view(a, b);
            const uint32_t n = v.n, nf = v.nf, nVarRank = v.nVarRank, nVarFree = v.nVarFree, ncol = v.ncol;
            const size_t lr         = nVarRank ? nVarRank : 1;
            double *RT              = a.scratch + (size_t)b * 2 * n * n; // nVarRank x (ncol + 1), column-major, ld = nVarRank
            double *D               = RT + lr * (ncol + 1);              // nVarFree x nVarFree, column-major (lower part used)
            const uint32_t ldd      = nVarFree ? nVarFree : 1;
            double *d               = smem;     // n
            double *xs              = smem + n; // n

            for (uint32_t e = tid; e < lr * (ncol + 1); e += NT) RT[e] = 0.0;
            for (uint32_t i = tid; i < n; i += NT)
            {
                d[i]  = 0.0;
                xs[i] = (i < nf) ? a.fixed_val[(size_t)b * n + i] : 0.0;
            }
            __syncthreads();
            leastnorm_compact_copy<NT>(v, RT, lr, RT + ncol * lr, tid);
            __syncthreads();
            // T <- R^-1 [T | rhs]: one column per lane, column-oriented back-substitution (lexlse.h:1180)
            for (uint32_t c = nVarRank + tid; c <= ncol; c += NT)
                for (uint32_t j = nVarRank; j--;)
                {
                    const double t = RT[j + c * lr] / RT[j + j * lr];
                    RT[j + c * lr] = t;
                    for (uint32_t i = 0; i < j; i++) RT[i + c * lr] = dfma(-RT[i + j * lr], t, RT[i + c * lr]);
                }
            __syncthreads();
            // D = I + T^T T (lower), d = T^T t_rhs (lexlse.h:1182-1188)
            for (uint32_t e = tid; e < nVarFree * nVarFree; e += NT)
            {
                const uint32_t i = e % nVarFree, j = e / nVarFree;
                if (i < j) continue;
                double acc = 0.0;
                for (uint32_t k = 0; k < nVarRank; k++) acc = dfma(RT[k + (nVarRank + i) * lr], RT[k + (nVarRank + j) * lr], acc);
                D[i + (size_t)j * ldd] = (i == j) ? acc + 1.0 : acc;
            }
            for (uint32_t j = tid; j < nVarFree; j += NT)
            {
                double acc = 0.0;
                for (uint32_t k = 0; k < nVarRank; k++) acc = dfma(RT[k + (nVarRank + j) * lr], RT[k + ncol * lr], acc);
                d[j] = acc;
            }
            __syncthreads();
            spd_solve<NT>(D, ldd, d, nVarFree, tid); // D z = d by Cholesky (lexlse.h:1190)
            for (uint32_t i = tid; i < nVarFree; i += NT) xs[nf + nVarRank + i] = d[i];
            __syncthreads();
            leastnorm_x_rank<NT>(v, xs, tid);
            __syncthreads();
            for (uint32_t j = nVarRank; j--;) // R^-1 on x.segment(nVarFixed, nVarRank) (lexlse.h:1205)
            {
                if (tid == 0) xs[nf + j] = xs[nf + j] / RT[j + j * lr];
                __syncthreads();
                const double xj = xs[nf + j];
                for (uint32_t i = tid; i < j; i += NT) xs[nf + i] = dfma(-RT[i + j * lr], xj, xs[nf + i]);
                __syncthreads();
            }
            // x = P x (lexlse.h:1044).  Scratch: d's place (smem itself: 16-byte aligned), copied into xs above
            apply_permutation_by_following<NT>(a, b, v.perm, a.totalrank[b], xs, reinterpret_cast<uint32_t *>(d), tid);
        }
        /// solveLeastNorm_3 (lexlse.h:1222-1277): least-norm solution from the null-space basis of the Tikhonov family,
        /// null_space(0:nVarRank, nVarFixed:) = [inv(R) | -inv(R) [T | rhs]].  Arithmetic order as the oracle's solveLeastNorm_3.
        template <int NT>
        __global__ __launch_bounds__(NT) void leastnorm3_kernel(LseArgs a)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x;
            const LeastNormView v = leastnorm_view(a, b);
            const uint32_t n = v.n, nf = v.nf, nVarRank = v.nVarRank, nVarFree = v.nVarFree;
            const double *NS  = a.reg_scratch + (size_t)b * reg_scratch_doubles(n); // n x (n+1), ld = n
            const uint32_t c0 = nf + nVarRank;
            double *D               = a.scratch + (size_t)b * 2 * n * n; // nVarFree x nVarFree (lower), column-major
            const uint32_t ldd      = nVarFree ? nVarFree : 1;
            double *d               = smem;     // n
            double *xs              = smem + n; // n
            double *out             = smem + 2 * n; // n

            for (uint32_t i = tid; i < n; i += NT) xs[i] = (i < nf) ? a.fixed_val[(size_t)b * n + i] : 0.0;
            for (uint32_t e = tid; e < nVarFree * nVarFree; e += NT)
            {
                const uint32_t i = e % nVarFree, j = e / nVarFree;
                if (i < j) continue;
                double acc = 0.0;
                for (uint32_t k = 0; k < nVarRank; k++) acc = dfma(NS[k + (size_t)(c0 + i) * n], NS[k + (size_t)(c0 + j) * n], acc);
                D[i + (size_t)j * ldd] = (i == j) ? acc + 1.0 : acc;
            }
            for (uint32_t j = tid; j < nVarFree; j += NT)
            {
                double acc = 0.0;
                for (uint32_t k = 0; k < nVarRank; k++) acc = dfma(NS[k + (size_t)(c0 + j) * n], NS[k + (size_t)(c0 + nVarFree) * n], acc);
                d[j] = acc;
            }
            __syncthreads();
            spd_solve<NT>(D, ldd, d, nVarFree, tid);
            for (uint32_t i = tid; i < nVarFree; i += NT) xs[c0 + i] = d[i];
            __syncthreads();
            leastnorm_x_rank<NT>(v, xs, tid);
            __syncthreads();
            for (uint32_t i = tid; i < nVarRank; i += NT) // x_rank <- triu(inv(R)) * x_rank
            {
                double acc = 0.0;
                for (uint32_t j = i; j < nVarRank; j++) acc = dfma(NS[i + (size_t)(nf + j) * n], xs[nf + j], acc);
                out[i] = acc;
            }
            __syncthreads();
            for (uint32_t i = tid; i < nVarRank; i += NT) xs[nf + i] = out[i];
            __syncthreads();
            // x = P x (lexlse.h:1044).  Scratch: xs = smem + n here, so the 16-byte alignment is counted from smem — behind x (n doubles from
            // xs) rounded up to an even number of doubles FROM SMEM; it overlays `out`, which has been copied into xs above
            apply_permutation_by_following<NT>(a, b, v.perm, a.totalrank[b], xs, reinterpret_cast<uint32_t *>(smem + ((2u * n + 1u) & ~1u)), tid);
        }
    } // namespace

    // ---------------------------------------------------------------------------------------------
    // launchers
    // ---------------------------------------------------------------------------------------------
    hipError_t launch_solve_generic(const LseArgs &a, hipStream_t s, bool reciprocal_diagonal, const char **variant)
    {
        const size_t lds = 16 * (size_t)a.nVar + 16 + (a.nVar + 1 <= 64 ? 0 : 8 * 64 * 65); // x by position + the diagonal of the level being solved (+ the 64 x 64 block of the blocked form)
        if (a.nVar + 1 <= 64)
        {
            hipError_t e = set_lds(solve_generic_kernel<64>, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((solve_generic_kernel<64>), dim3(a.batch), dim3(64), lds, s, a);
            if (variant) *variant = "solve_generic<64>";
        }
        else
        {
            hipError_t e = reciprocal_diagonal ? set_lds(solve_generic_kernel<256, true>, lds) : set_lds(solve_generic_kernel<256>, lds);
            if (e != hipSuccess) return e;
            if (reciprocal_diagonal)
                hipLaunchKernelGGL((solve_generic_kernel<256, true>), dim3(a.batch), dim3(256), lds, s, a);
            else
                hipLaunchKernelGGL((solve_generic_kernel<256>), dim3(a.batch), dim3(256), lds, s, a);
            if (variant) *variant = reciprocal_diagonal ? "solve_generic<256,reciprocal>" : "solve_generic<256>";
        }
        return hipGetLastError();
    }

    hipError_t launch_residual(const LseArgs &a, hipStream_t s, const char **variant)
    {
        const size_t lds = 8 * ((size_t)a.cap + 2);
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        hipError_t e = set_lds(residual_kernel<64>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((residual_kernel<64>), dim3(a.batch), dim3(64), lds, s, a);
        if (variant) *variant = "residual<64>";
        return hipGetLastError();
    }

    namespace
    {
        int cus_of_current_device() // (a process may drive several)
        {
            static int cus_of[64] = {0};
            int dev = 0;
            if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64)
            {
                if (!cus_of[dev] && (hipDeviceGetAttribute(&cus_of[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus_of[dev] <= 0)) cus_of[dev] = 256;
                return cus_of[dev];
            }
            return 256;
        }
    } // namespace

    /// the single-sweep form (sensitivity_sweep_kernel): level dims <= 16, at most 8 objectives per sweep, one wavefront per problem with
    /// the factor staged in LDS — what a lock-step LSI stage asks for.  max_level_dim comes from the caller (0 = unknown: not taken)
    bool sensitivity_sweep_serves(const LseArgs &a, uint32_t sweep_level_dim_hint)
    {
        return sweep_shape_serves(a.nVar, a.nObj, a.cap, a.reg_type, sweep_level_dim_hint) &&
               a.batch <= 4u * (uint32_t)cus_of_current_device() && !std::getenv("LEXLS_SENS_NO_SWEEP");
    }

    hipError_t launch_sensitivity(const LseArgs &a, const int32_t *d_obj_index, int32_t obj_all, double tolW, double tolC, hipStream_t s, bool scan_up, uint32_t sweep_level_dim_hint,
                                  bool collect, const char **variant)
    {
        if (collect && !a.wrong_sign) return hipErrorInvalidValue;
        const size_t lds = 8 * (2 * (size_t)a.nVar + a.cap + 2) + sizeof(SensState) + 16;
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        // Factor staged into LDS when latency is what counts: few problems per CU (a lock-step LSI stage) — with thousands of problems
        // the 20 KB per workgroup would cost the wavefronts in flight that hide the chains instead (4096 problems: 0.090 -> 0.126 ms)
        const size_t lds_staged = lds + 8 * ((size_t)(a.cap | 1u) * (a.nVar + 1) + a.cap) + (((size_t)a.cap + a.nVar + 15) & ~(size_t)15);
        const int cus           = cus_of_current_device();
        const size_t lds_sweep  = sweep_lds_bytes(a.nVar, a.cap);
        if (sensitivity_sweep_serves(a, sweep_level_dim_hint))
        {
            static_assert(SWEEP_MD == 16, "the names below spell the sweep's level capacity out");
            if (variant) *variant = sweep_level_dim_hint <= 12 ? (collect ? "sensitivity_sweep<12,collect>" : "sensitivity_sweep<12>") : (collect ? "sensitivity_sweep<16,collect>" : "sensitivity_sweep<16>");
            if (collect && sweep_level_dim_hint <= 12)
                hipLaunchKernelGGL((sensitivity_sweep_kernel<12, true>), dim3(a.batch), dim3(64), lds_sweep, s, a, d_obj_index, obj_all, tolW, tolC, scan_up ? 1 : 0);
            else if (collect)
                hipLaunchKernelGGL((sensitivity_sweep_kernel<SWEEP_MD, true>), dim3(a.batch), dim3(64), lds_sweep, s, a, d_obj_index, obj_all, tolW, tolC, scan_up ? 1 : 0);
            else if (sweep_level_dim_hint <= 12)
                hipLaunchKernelGGL(sensitivity_sweep_kernel<12>, dim3(a.batch), dim3(64), lds_sweep, s, a, d_obj_index, obj_all, tolW, tolC, scan_up ? 1 : 0);
            else
                hipLaunchKernelGGL(sensitivity_sweep_kernel<SWEEP_MD>, dim3(a.batch), dim3(64), lds_sweep, s, a, d_obj_index, obj_all, tolW, tolC, scan_up ? 1 : 0);
            return hipGetLastError();
        }
        // (up to a problem per CU the whole LDS is there for the taking: a single mid-size problem — configs[0] — walks its chains at LDS
        // latency instead of through L2)
        if ((lds_staged <= 40 * 1024 && a.batch <= 4u * (uint32_t)cus) || (lds_staged <= kMaxLdsBytes && a.batch <= (uint32_t)cus))
        {
            if (lds_staged > 64 * 1024)
            {
                hipError_t e = set_lds(sensitivity_kernel<64, true>, lds_staged);
                if (e != hipSuccess) return e;
            }
            hipLaunchKernelGGL((sensitivity_kernel<64, true>), dim3(a.batch), dim3(64), lds_staged, s, a, d_obj_index, obj_all, tolW, tolC, scan_up ? 1 : 0, collect ? 1 : 0);
            if (variant) *variant = "sensitivity<64,staged>";
            return hipGetLastError();
        }
        hipError_t e = set_lds(sensitivity_kernel<64, false>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((sensitivity_kernel<64, false>), dim3(a.batch), dim3(64), lds, s, a, d_obj_index, obj_all, tolW, tolC, scan_up ? 1 : 0, collect ? 1 : 0);
        if (variant) *variant = "sensitivity<64,hbm>";
        return hipGetLastError();
    }

    /// every objective's multipliers in one launch (multipliers_sweep_kernel) where the sweep serves the shape — as for the removal search, but
    /// whatever the batch size: there is no per-objective launch to weigh it against
    bool multipliers_sweep_serves(const LseArgs &a, uint32_t sweep_level_dim_hint)
    {
        return sweep_shape_serves(a.nVar, a.nObj, a.cap, a.reg_type, sweep_level_dim_hint) && !std::getenv("LEXLS_SENS_NO_SWEEP");
    }

    size_t multipliers_scratch_bytes(const LseArgs &a)
    {
        const size_t B = a.batch;
        return 8 * B * ((size_t)a.nVar + a.cap) + 8 * B + 4 * 3 * B + B * ((size_t)a.cap + a.nVar);
    }

    hipError_t sensitivity_scratch_args(const LseArgs &a, void *d_scratch, hipStream_t s, LseArgs *out)
    {
        LseArgs &t     = *out = a;
        const size_t B = a.batch;
        t.lambda       = static_cast<double *>(d_scratch);
        t.maxabs       = t.lambda + B * ((size_t)a.nVar + a.cap);
        t.sens         = reinterpret_cast<int32_t *>(t.maxabs + B);
        t.ctr_type     = reinterpret_cast<uint8_t *>(t.sens + 3 * B);
        t.fixed_type   = t.ctr_type + B * a.cap;
        hipError_t e   = hipMemcpyAsync(t.ctr_type, a.ctr_type, B * a.cap, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(t.fixed_type, a.fixed_type, B * a.nVar, hipMemcpyDeviceToDevice, s);
        return e;
    }

    hipError_t launch_multipliers(const LseArgs &a, double *d_out, uint32_t sweep_level_dim_hint, hipStream_t s, void *d_scratch, bool *swept, const char **variant)
    {
        const size_t ldo = (size_t)a.nVar + a.cap;
        if (multipliers_sweep_serves(a, sweep_level_dim_hint))
        {
            if (swept) *swept = true;
            if (variant) *variant = sweep_level_dim_hint <= 12 ? "multipliers_sweep<12>" : "multipliers_sweep<16>";
            if (sweep_level_dim_hint <= 12)
                hipLaunchKernelGGL(multipliers_sweep_kernel<12>, dim3(a.batch), dim3(64), sweep_lds_bytes(a.nVar, a.cap), s, a, d_out);
            else
                hipLaunchKernelGGL(multipliers_sweep_kernel<SWEEP_MD>, dim3(a.batch), dim3(64), sweep_lds_bytes(a.nVar, a.cap), s, a, d_out);
            return hipGetLastError();
        }
        if (swept) *swept = false;
        if (variant) *variant = "multipliers<per-objective>";
        // one sensitivity_kernel launch per objective, each copied into its column; the launches write the multipliers, decisions and marks into
        // scratch (the types are copied there first: the handle's own arrays stay as they are, as they do under the sweep)
        if (!d_scratch) return hipErrorInvalidValue;
        LseArgs t;
        hipError_t e = sensitivity_scratch_args(a, d_scratch, s, &t);
        for (uint32_t k = 0; k < a.nObj && e == hipSuccess; k++)
        {
            e = launch_sensitivity(t, nullptr, (int32_t)k, 1e-8, 1e-12, s, false, 0);
            if (e == hipSuccess) e = hipMemcpy2DAsync(d_out + k * ldo, 8 * ldo * a.nObj, t.lambda, 8 * ldo, 8 * ldo, a.batch, hipMemcpyDeviceToDevice, s);
        }
        return e;
    }

    hipError_t launch_leastnorm(const LseArgs &a, hipStream_t s, const char **variant)
    {
        const size_t lds = 8 * (2 * (size_t)a.nVar + 4);
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        hipError_t e = set_lds(leastnorm_kernel<64>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((leastnorm_kernel<64>), dim3(a.batch), dim3(64), lds, s, a);
        if (variant) *variant = "leastnorm_1<64>";
        return hipGetLastError();
    }

    hipError_t launch_leastnorm2(const LseArgs &a, hipStream_t s, const char **variant)
    {
        const size_t lds = 8 * (2 * (size_t)a.nVar + 4);
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        hipError_t e = set_lds(leastnorm2_kernel<64>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((leastnorm2_kernel<64>), dim3(a.batch), dim3(64), lds, s, a);
        if (variant) *variant = "leastnorm_2<64>";
        return hipGetLastError();
    }

    hipError_t launch_leastnorm3(const LseArgs &a, hipStream_t s, const char **variant)
    {
        const size_t lds = 8 * (3 * (size_t)a.nVar + 4);
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        hipError_t e = set_lds(leastnorm3_kernel<64>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((leastnorm3_kernel<64>), dim3(a.batch), dim3(64), lds, s, a);
        if (variant) *variant = "leastnorm_3<64>";
        return hipGetLastError();
    }
} // namespace lexls
