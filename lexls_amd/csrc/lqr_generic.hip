// Generic lexicographic-QR kernels: ONE WORKGROUP PER PROBLEM, any shape.  This unit: the factorization (+ solve) and the row gather;
// the kernels that run behind the kept factor are lse_postfactor.hip's.
//
// This is the shape-agnostic path of liblexls_hip: it factors and solves a problem of any size
// (matrix staged in LDS when it fits in the CU's 160 KiB, otherwise worked on in HBM/L2) and is the
// fallback behind the shape-specialised kernels.  It follows the reference algorithm statement by
// statement — LexLSE::factorize() lexlse.h:117-506, solve() :1015-1045 — and evaluates every
// reduction in the order fixed by the arithmetic contract in oracle/lexlse_oracle.h (ascending fma
// chains, first-occurrence argmax, IEEE division/sqrt), so its results are bit-identical to the
// CPU oracle's.  Parallelism inside a problem: columns across lanes for norms / Householder
// application (each lane owns whole columns, so every dot product is a lane-local ordered chain,
// no cross-lane reduction), rows across lanes for the column swap and the Gauss TRSM, elements
// across lanes for the trailing update.
//
// LDS image: column-major with an ODD leading dimension ldp so that "lane j reads (i, j)" hits 32
// distinct 8-byte bank pairs (ds_read_b64: bank = (addr/4) % 64, stride 2*ldp dwords).
#include "lexls_kernels.h"
#include "lexls_launch.h"
#include "lqr_wave_common.h"
#include "lqr_generic_steps.h"
#include "lexls_regularize.h"

#include <cfloat>

namespace lexls
{
    namespace
    {
// Diagnostic build only (-DLEXLS_GENERIC_STAMPS): thread 0 of lqr_generic_kernel accumulates shader-clock totals per phase and leaves them in
// the (otherwise unused) multiplier buffer; the product build contains no stamp.  Phases: 0 stage + init + fixed variables, 1 level norms,
// 2 pivot search, 3 fresh norm + reflector scalars, 4 column swap + essential part, 5 reflector application + down-date,
// 6 regularization + Gauss step, 7 results + factor store, 8 solve, 9 the dot-product phase of 5 (up to its barrier)
#ifdef LEXLS_GENERIC_STAMPS
#define GSTAMP_DECL                 \
    unsigned long long gs_acc[10];   \
    for (int i_ = 0; i_ < 10; i_++) gs_acc[i_] = 0; \
    unsigned long long gs_t0 = clock64();
#define GSTAMP(i)                                  \
    {                                              \
        const unsigned long long t_ = clock64();   \
        gs_acc[i] += t_ - gs_t0;                   \
        gs_t0 = t_;                                \
    }
#define GSTAMP_WRITE \
    if (tid == 0)    \
        for (int i_ = 0; i_ < 10; i_++) a.lambda[(size_t)b * (n + cap) + i_] = (double)gs_acc[i_];
#else
#define GSTAMP_DECL
#define GSTAMP(i)
#define GSTAMP_WRITE
#endif

        /// block-wide "first index of the maximum" (every thread passes its best candidate) with ONE barrier: the wavefront's maximum by DPP (wave_max), the first position that attains it by a minimum over the
        /// lanes that hold it, then the NT/64 wavefront results through LDS; the slots alternate with `parity` (a pivot's slots are not
        /// rewritten before the pivot after the next one, several barriers later).  rv / ri hold at least 32 entries (NT >= 64).
        template <int NT>
        __device__ __forceinline__ uint32_t block_argmax_fast(double v, uint32_t idx, double *rv, uint32_t *ri, uint32_t tid, uint32_t parity)
        {
            const double m = wave_max(v);
            unsigned c     = row_min16(v == m ? idx : 0xffffffffu);
            {
                const unsigned c0 = (unsigned)__builtin_amdgcn_readlane((int)c, 0), c1 = (unsigned)__builtin_amdgcn_readlane((int)c, 16);
                const unsigned c2 = (unsigned)__builtin_amdgcn_readlane((int)c, 32), c3 = (unsigned)__builtin_amdgcn_readlane((int)c, 48);
                const unsigned a01 = c0 < c1 ? c0 : c1, a23 = c2 < c3 ? c2 : c3;
                c = a01 < a23 ? a01 : a23;
            }
            if (NT == 64) return c;
            const uint32_t base = parity * 16u;
            if ((tid & 63u) == 0)
            {
                rv[base + (tid >> 6)] = m;
                ri[base + (tid >> 6)] = c;
            }
            __syncthreads();
            double fm   = rv[base];
            uint32_t fi = ri[base];
#pragma unroll
            for (uint32_t w = 1; w < (uint32_t)(NT / 64); w++)
            {
                const double v2   = rv[base + w];
                const uint32_t i2 = ri[base + w];
                if (v2 > fm || (v2 == fm && i2 < fi))
                {
                    fm = v2;
                    fi = i2;
                }
            }
            return fi;
        }

        /// s = fma(p_i, p_i, s) for i ascending.  The reads of a chunk of U are issued together and the next chunk is fetched (into the
        /// other of two register sets) before the current one is consumed, so the chain runs at the latency of the fused multiply-add
        /// instead of a memory round trip per term (same order, same result)
        template <int U>
        __device__ __forceinline__ double chain_square(const double *p, uint32_t len, double s)
        {
            uint32_t i = 0;
            if (len >= (uint32_t)U)
            {
                double v0[U], v1[U];
#pragma unroll
                for (int u = 0; u < U; u++) v0[u] = p[u];
                i = U;
                while (true)
                {
                    const bool more1 = i + U <= len;
                    if (more1)
                    {
#pragma unroll
                        for (int u = 0; u < U; u++) v1[u] = p[i + u];
                        i += U;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) s = dfma(v0[u], v0[u], s);
                    if (!more1) break;
                    const bool more0 = i + U <= len;
                    if (more0)
                    {
#pragma unroll
                        for (int u = 0; u < U; u++) v0[u] = p[i + u];
                        i += U;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) s = dfma(v1[u], v1[u], s);
                    if (!more0) break;
                }
            }
            for (; i < len; i++) s = dfma(p[i], p[i], s);
            return s;
        }
        /// the two chains of a pivot column in one pass: fresh = sum_{i<R} c_i^2 and tail = sum_{1<=i<R} c_i^2, each ascending from 0
        template <int U>
        __device__ __forceinline__ void chain_square_pair(const double *c, uint32_t R, double &fresh, double &tail)
        {
            double f = dfma(c[0], c[0], 0.0), t = 0.0;
            uint32_t i = 1;
            if (R >= 1u + (uint32_t)U)
            {
                double v0[U], v1[U];
#pragma unroll
                for (int u = 0; u < U; u++) v0[u] = c[1 + u];
                i = 1 + U;
                while (true)
                {
                    const bool more1 = i + U <= R;
                    if (more1)
                    {
#pragma unroll
                        for (int u = 0; u < U; u++) v1[u] = c[i + u];
                        i += U;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++)
                    {
                        f = dfma(v0[u], v0[u], f);
                        t = dfma(v0[u], v0[u], t);
                    }
                    if (!more1) break;
                    const bool more0 = i + U <= R;
                    if (more0)
                    {
#pragma unroll
                        for (int u = 0; u < U; u++) v0[u] = c[i + u];
                        i += U;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++)
                    {
                        f = dfma(v1[u], v1[u], f);
                        t = dfma(v1[u], v1[u], t);
                    }
                    if (!more0) break;
                }
            }
            for (; i < R; i++)
            {
                f = dfma(c[i], c[i], f);
                t = dfma(c[i], c[i], t);
            }
            fresh = f;
            tail  = t;
        }

        struct Shared
        {
            double tau, beta, den;
            uint32_t piv;
            int stop, degenerate;
        };

        // -----------------------------------------------------------------------------------------
        // factorize (+ solve)
        // -----------------------------------------------------------------------------------------
        template <int NT, bool LDSMAT>
        __global__ __launch_bounds__(NT) void lqr_generic_kernel(LseArgs a, int write_factor, int do_solve)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x;
            const uint32_t n = a.nVar, cap = a.cap, nObj = a.nObj;
            const size_t pstride = (size_t)cap * (n + 1);
            if (a.skip && a.skip[b]) return; // uniform per workgroup
            // terms per read batch of the ordered chains: the one-wavefront form serves large batches of small problems, where registers
            // are occupancy (16 -> 157 VGPRs, 3 wavefronts per SIMD: measured slower there); the wide forms run one workgroup per CU
            constexpr int CH = NT >= 256 ? 16 : 4;
            GSTAMP_DECL

            // ---- LDS carve-up (doubles first) ----
            double *W;
            size_t ld;
            double *p = smem;
            if (LDSMAT)
            {
                W  = p;
                ld = a.ldp;
                p += (size_t)a.ldp * (n + 1);
            }
            else
            {
                W  = a.fac + b * pstride;
                ld = cap;
            }
            double *norms  = p;
            double *xs     = norms + n;
            double *red_v  = xs + n;
            Shared *sh     = reinterpret_cast<Shared *>(red_v + NT);
            uint32_t *red_i  = reinterpret_cast<uint32_t *>(sh + 1);
            uint32_t *perm_s = red_i + NT;
            uint32_t *rk_s   = perm_s + n;
            uint32_t *fc_s   = rk_s + nObj;
            uint32_t *fr_s   = fc_s + nObj;

            const uint32_t *dims = a.dims + (size_t)b * nObj;
            uint32_t M           = 0;
            for (uint32_t k = 0; k < nObj; k++)
            {
                if (tid == 0)
                {
                    fr_s[k] = M;
                    rk_s[k] = 0;
                    fc_s[k] = 0;
                }
                M += dims[k];
            }

            // ---- fixed variables (lexlse.h:132-143): the column transpositions, and — when the matrix is staged into LDS — the column
            // order they leave behind, so that the staging pass below places the columns directly (one pass instead of one per variable)
            const uint32_t nf = a.nfixed ? a.nfixed[b] : 0;
            for (uint32_t i = tid; i < n; i += NT) perm_s[i] = i;
            const uint32_t *src = nullptr;
            if (nf > 0)
            {
                uint32_t *order = reinterpret_cast<uint32_t *>(norms); // norms is free until the level loop: n + n entries
                uint32_t *fidx  = order + n;                             // scratch copy of fixed_var_index
                uint32_t *where = reinterpret_cast<uint32_t *>(xs);    // xs is initialised after the staging pass: slot that holds a value
                for (uint32_t k = tid; k < nf; k += NT) fidx[k] = a.fixed_idx[(size_t)b * n + k];
                for (uint32_t v = tid; v < n; v += NT) where[v] = 0xffffffffu;
                __syncthreads();
                if (tid == 0)
                {
                    // lexlse.h:146-153: slot k takes its variable; the later slot that named variable k is redirected to the column that
                    // variable k was swapped into.  With distinct indices (the normal case) "the later slot" is a table look-up
                    bool distinct = true;
                    for (uint32_t i = 0; i < nf; i++)
                    {
                        const uint32_t v = fidx[i];
                        if (where[v] != 0xffffffffu) distinct = false;
                        else where[v] = i;
                    }
                    for (uint32_t k = 0; k < nf; k++)
                    {
                        const uint32_t coeff = fidx[k];
                        perm_s[k]            = coeff;
                        if (distinct)
                        {
                            const uint32_t i = where[k];
                            if (i != 0xffffffffu && i > k)
                            {
                                fidx[i]      = coeff;
                                where[coeff] = i;
                            }
                            continue;
                        }
                        for (uint32_t i = k + 1; i < nf; i++)
                        {
                            if (fidx[i] == k)
                            {
                                fidx[i] = coeff;
                                break;
                            }
                        }
                    }
                    if (LDSMAT)
                    {
                        for (uint32_t j = 0; j < n; j++) order[j] = j;
                        for (uint32_t k = 0; k < nf; k++) // swapping columns k and perm[k] = swapping where they come from
                        {
                            const uint32_t c = perm_s[k], t = order[k];
                            order[k]         = order[c];
                            order[c]         = t;
                        }
                    }
                }
                if (LDSMAT) src = reinterpret_cast<const uint32_t *>(norms);
                __syncthreads();
            }

            // ---- stage the problem (coalesced down the columns) ----
            const double *in = a.in + b * pstride;
            if (LDSMAT || in != W)
            {
                // every thread busy and eight independent loads in flight per thread (a column at a time leaves NT - M threads idle and
                // one global round trip per column on the critical path)
                const uint32_t total = M * (n + 1);
                constexpr int SU = 8;
                for (uint32_t e0 = tid; e0 < total; e0 += SU * NT)
                {
                    double v[SU];
                    uint32_t dst[SU];
#pragma unroll
                    for (int u = 0; u < SU; u++)
                    {
                        const uint32_t e = e0 + (uint32_t)u * NT;
                        const uint32_t j = e < total ? e / M : 0, i = e < total ? e - j * M : 0;
                        const size_t sj  = (src && j < n) ? src[j] : j;
                        v[u]             = e < total ? in[i + sj * cap] : 0.0;
                        dst[u]           = e < total ? (uint32_t)(i + j * ld) : 0xffffffffu;
                    }
#pragma unroll
                    for (int u = 0; u < SU; u++)
                        if (dst[u] != 0xffffffffu) W[dst[u]] = v[u];
                }
            }
            double *hh = a.hh + (size_t)b * cap;
            for (uint32_t i = tid; i < cap; i += NT) hh[i] = 0.0; // initialize(), lexlse.h:1683
            for (uint32_t i = tid; i < n; i += NT) xs[i] = (i < nf) ? a.fixed_val[(size_t)b * n + i] : 0.0;
            if (a.reg_type) // initialize(): null_space.setZero() (lexlse.h:1686)
            {
                double *NS = a.reg_scratch + (size_t)b * reg_scratch_doubles(n);
                for (uint32_t e = tid; e < n * (n + 1); e += NT) NS[e] = 0.0;
            }
            double *mu_x = nullptr, *mu_res = nullptr; // by-products of the experimental type 7 (lexlse.h:96-99, zeroed by initialize() :1687-1689)
            if (a.reg_type == 7)
            {
                mu_x   = a.reg_mu + (size_t)b * reg_mu_doubles(n, nObj, cap);
                mu_res = mu_x + 2 * (size_t)nObj * n;
                for (size_t e = tid; e < reg_mu_doubles(n, nObj, cap); e += NT) mu_x[e] = 0.0;
            }
            __syncthreads();

            // ---- fixed variables: their columns go first (done by the staging pass when the matrix lives in LDS), their contribution
            // goes to the RHS (lexlse.h:132-156) ----
            if (nf > 0)
            {
                if (!LDSMAT)
                    for (uint32_t k = 0; k < nf; k++)
                    {
                        const uint32_t coeff = perm_s[k];
                        if (coeff != k)
                            for (uint32_t i = tid; i < M; i += NT)
                            {
                                const double t    = W[i + k * ld];
                                W[i + k * ld]     = W[i + coeff * ld];
                                W[i + coeff * ld] = t;
                            }
                        __syncthreads();
                    }
                for (uint32_t i = tid; i < M; i += NT)
                {
                    double s = 0.0;
                    for (uint32_t k = 0; k < nf; k++) s = dfma(W[i + k * ld], xs[k], s);
                    W[i + n * ld] -= s;
                }
                __syncthreads();
            }

            uint32_t ColIndex  = nf;
            uint32_t TotalRank = nf;
            GSTAMP(0)

            if (ColIndex < n)
            {
                for (uint32_t ObjIndex = 0; ObjIndex < nObj; ObjIndex++)
                {
                    const uint32_t F = fr_s[ObjIndex], Fc = ColIndex, dim = dims[ObjIndex];
                    if (tid == 0) fc_s[ObjIndex] = Fc;

                    if (mu_res) // lexlse.h:191: the level's right-hand side after the eliminations, before its reflectors
                        for (uint32_t i = tid; i < dim; i += NT) mu_res[F + i] = W[F + i + n * ld];

                    // initial squared column norms of the level (lexlse.h:193-196): one ordered chain per column
                    for (uint32_t k = ColIndex + tid; k < n; k += NT)
                    {
                        norms[k] = chain_square<CH>(W + F + k * ld, dim, 0.0);
                    }
                    __syncthreads();
                    GSTAMP(1)

                    for (uint32_t counter = 0; counter < dim; counter++)
                    {
                        const uint32_t row = F + counter, R = dim - counter;

                        // pivot = first maximum of the down-dated norms (lexlse.h:205-206)
                        double bv   = -INFINITY;
                        uint32_t bi = 0xffffffffu;
                        for (uint32_t k = ColIndex + tid; k < n; k += NT)
                            if (norms[k] > bv)
                            {
                                bv = norms[k];
                                bi = k;
                            }
                        const uint32_t piv = block_argmax_fast<NT>(bv, bi, red_v, red_i, tid, counter & 1u);
                        GSTAMP(2)

                        // fresh norm, rank test, Householder scalars (lexlse.h:210-217, :241)
                        if (tid == 0)
                        {
                            const double *col = W + row + piv * ld;
                            double fresh, tailSq;
                            chain_square_pair<CH>(col, R, fresh, tailSq);
                            norms[piv]     = fresh;
                            sh->stop       = fresh < a.tol;
                            sh->degenerate = 0;
                            sh->tau        = 0.0;
                            if (!sh->stop)
                            {
                                perm_s[ColIndex]       = piv;
                                const double t         = norms[ColIndex];
                                norms[ColIndex]        = norms[piv];
                                norms[piv]             = t;
                                if (R > 1)
                                {
                                    const double c0 = col[0];
                                    if (tailSq <= DBL_MIN)
                                    {
                                        sh->degenerate = 1;
                                        sh->beta       = c0;
                                    }
                                    else
                                    {
                                        double beta = sqrt(dfma(c0, c0, tailSq));
                                        if (c0 >= 0.0) beta = -beta;
                                        sh->beta = beta;
                                        sh->den  = c0 - beta;
                                        sh->tau  = (beta - c0) / beta;
                                    }
                                }
                            }
                        }
                        __syncthreads();
                        GSTAMP(3)
                        if (sh->stop) break; // uniform

                        // column swap over ALL nCtr rows (lexlse.h:222-232) fused with writing beta / the essential part
                        {
                            const double den = sh->den, beta = sh->beta;
                            const int degenerate = sh->degenerate;
                            for (uint32_t i = tid; i < M; i += NT)
                            {
                                const double a1 = W[i + ColIndex * ld];
                                const double a2 = W[i + piv * ld];
                                double newc     = a2;
                                if (R > 1)
                                {
                                    if (i == row)
                                        newc = beta;
                                    else if (i > row && i < row + R)
                                        newc = degenerate ? 0.0 : a2 / den;
                                }
                                W[i + ColIndex * ld] = newc;
                                if (piv != ColIndex) W[i + piv * ld] = a1;
                            }
                            if (a.reg_type && piv != ColIndex) // lexlse.h:229-231: the rows of the basis above this level's first column
                            {
                                double *NS = a.reg_scratch + (size_t)b * reg_scratch_doubles(n);
                                for (uint32_t i = tid; i < Fc; i += NT)
                                {
                                    const double t               = NS[i + (size_t)ColIndex * n];
                                    NS[i + (size_t)ColIndex * n] = NS[i + (size_t)piv * n];
                                    NS[i + (size_t)piv * n]      = t;
                                }
                            }
                        }
                        __syncthreads();
                        GSTAMP(4)

                        // apply H to the trailing columns incl. the RHS (lexlse.h:243-246), then down-date (:262-266)
                        {
                            const double tau  = sh->tau;
                            const double *ess = W + row + 1 + ColIndex * ld;
                            // Two phases per batch of NT columns.  A: one thread per column walks the ordered dot product (the only serial
                            // part), updates the column's pivot-row entry and down-dates its norm.  B: ALL threads apply the rank-one
                            // update to the rows below (lanes along the rows, 32 at a time; the column-per-thread form left 3/4 of the
                            // workgroup idle through half of the step).  Same operations on every entry, same results.
                            const bool reflect = R > 1 && tau != 0.0; // uniform
                            for (uint32_t base = ColIndex + 1; base <= n; base += NT)
                            {
                                const uint32_t j = base + tid;
                                if (j <= n)
                                {
                                    double *col = W + row + j * ld;
                                    if (reflect)
                                    {
                                        double tmp = chain_dot<CH>(ess, col + 1, R - 1, 0.0);
                                        tmp += col[0];
                                        col[0]     = dfma(-tau, tmp, col[0]);
                                        red_v[tid] = tmp;
                                    }
                                    if (j < n) norms[j] = dfma(-col[0], col[0], norms[j]);
                                }
                                if (reflect)
                                {
                                    __syncthreads();
                                    GSTAMP(9)
                                    const uint32_t nb = (n + 1 - base < (uint32_t)NT) ? n + 1 - base : (uint32_t)NT;
                                    const uint32_t tx = tid & 31u, ty = tid >> 5;
                                    constexpr uint32_t CG = NT / 32; // column groups
                                    for (uint32_t i = 1 + tx; i < R; i += 32)
                                    {
                                        const double te = -(tau * ess[i - 1]);
                                        uint32_t c      = ty;
                                        for (; c + 3 * CG < nb; c += 4 * CG) // four columns per trip: their reads are issued together
                                        {
                                            double *p0 = W + row + i + (base + c) * ld, *p1 = p0 + CG * ld, *p2 = p1 + CG * ld, *p3 = p2 + CG * ld;
                                            const double c0 = *p0, c1 = *p1, c2 = *p2, c3 = *p3;
                                            const double t0 = red_v[c], t1 = red_v[c + CG], t2 = red_v[c + 2 * CG], t3 = red_v[c + 3 * CG];
                                            *p0 = dfma(te, t0, c0);
                                            *p1 = dfma(te, t1, c1);
                                            *p2 = dfma(te, t2, c2);
                                            *p3 = dfma(te, t3, c3);
                                        }
                                        for (; c < nb; c += CG)
                                        {
                                            double *p0 = W + row + i + (base + c) * ld;
                                            *p0        = dfma(te, red_v[c], *p0);
                                        }
                                    }
                                    if (base + NT <= n) __syncthreads(); // red_v is rewritten by the next batch
                                }
                            }
                            if (tid == 0 && R > 1) hh[row] = tau;
                        }
                        ColIndex++;
                        __syncthreads();
                        GSTAMP(5)
                        if (ColIndex == n) break;
                    }

                    const uint32_t rank = ColIndex - Fc;
                    if (tid == 0) rk_s[ObjIndex] = rank;
                    TotalRank += rank;

                    if (a.reg_type) // lexlse.h:277-411: the level's transformed right-hand side is damped before the Gauss step
                    {
                        __syncthreads();
                        const RegLevels lv = {fr_s, fc_s, rk_s, perm_s, hh, dim};
                        regularize_level<NT>(a, b, W, ld, nf, ObjIndex, F, Fc, rank, n - ColIndex, tid, &lv);
                    }

                    // Gauss step (lexlse.h:431-471)
                    if (ObjIndex + 1 < nObj && rank > 0)
                    {
                        const uint32_t Fn = F + dim;
                        for (uint32_t i = Fn + tid; i < M; i += NT) // L <- L R^-1, one row per lane (reciprocal of the diagonal, see oracle)
                        {
                            for (uint32_t p2 = 0; p2 < rank; p2++)
                            {
                                double s = W[i + (Fc + p2) * ld];
                                for (uint32_t q = 0; q < p2; q++) s = dfma(-W[i + (Fc + q) * ld], W[F + q + (Fc + p2) * ld], s);
                                W[i + (Fc + p2) * ld] = s * (1.0 / W[F + p2 + (Fc + p2) * ld]);
                            }
                        }
                        __syncthreads();
                        const uint32_t nrows = M - Fn, ncols = n - ColIndex + 1;
                        if (nrows > 0)
                            for (uint32_t e = tid; e < nrows * ncols; e += NT) // Trailing -= L * Up, one element per lane
                            {
                                const uint32_t i = Fn + e % nrows, j = ColIndex + e / nrows;
                                double t         = W[i + j * ld];
                                for (uint32_t p2 = 0; p2 < rank; p2++) t = dfma(-W[i + (Fc + p2) * ld], W[F + p2 + j * ld], t);
                                W[i + j * ld] = t;
                            }
                        __syncthreads();
                    }

                    GSTAMP(6)
                    if (ColIndex == n) // lexlse.h:475-490
                    {
                        if (tid == 0)
                            for (uint32_t k = ObjIndex + 1; k < nObj; k++) fc_s[k] = fc_s[k - 1] + rk_s[k - 1];
                        if (mu_x) // lexlse.h:483-486
                        {
                            __syncthreads();
                            for (uint32_t k = ObjIndex + 1; k < nObj; k++)
                            {
                                for (uint32_t i = tid; i < n; i += NT)
                                {
                                    mu_x[(size_t)k * n + i]          = mu_x[(size_t)(k - 1) * n + i];
                                    mu_x[(size_t)(nObj + k) * n + i] = mu_x[(size_t)(nObj + k - 1) * n + i];
                                }
                                for (uint32_t i = tid; i < dims[k]; i += NT) mu_res[fr_s[k] + i] = -W[fr_s[k] + i + n * ld];
                                __syncthreads();
                            }
                        }
                        break;
                    }
                }
            }
            __syncthreads();

            // ---- results of factorize() ----
            for (uint32_t k = tid; k < nObj; k += NT)
            {
                a.rank[(size_t)b * nObj + k] = rk_s[k];
                a.fcol[(size_t)b * nObj + k] = fc_s[k];
            }
            for (uint32_t i = tid; i < n; i += NT) a.perm[(size_t)b * n + i] = (i < TotalRank) ? perm_s[i] : i;
            if (tid == 0) a.totalrank[b] = TotalRank;
            if (LDSMAT && write_factor)
            {
                double *out = a.fac + b * pstride;
                for (uint32_t j = 0; j <= n; j++)
                    for (uint32_t i = tid; i < M; i += NT) out[i + (size_t)j * cap] = W[i + j * ld];
            }

            GSTAMP(7)
            // ---- solve(): block back-substitution (lexlse.h:1015-1045) ----
            if (do_solve)
            {
                uint32_t acc = 0;
                for (uint32_t k = nObj; k--;)
                {
                    const uint32_t rank = rk_s[k];
                    if (rank == 0) continue;
                    const uint32_t F = fr_s[k], Fc = fc_s[k];
                    const uint32_t c0 = (acc > 0) ? fc_s[k + 1] : 0;
                    for (uint32_t i = tid; i < rank; i += NT)
                    {
                        double s = W[F + i + n * ld];
                        for (uint32_t j = 0; j < acc; j++) s = dfma(-W[F + i + (c0 + j) * ld], xs[c0 + j], s);
                        xs[Fc + i] = s;
                    }
                    __syncthreads();
                    for (uint32_t j = rank; j--;)
                    {
                        if (tid == 0) xs[Fc + j] = xs[Fc + j] / W[F + j + (Fc + j) * ld];
                        __syncthreads();
                        const double xj = xs[Fc + j];
                        for (uint32_t i = tid; i < j; i += NT) xs[Fc + i] = dfma(-W[F + i + (Fc + j) * ld], xj, xs[Fc + i]);
                        __syncthreads();
                    }
                    acc += rank;
                }
                // x = P x (lexlse.h:1044): variable i follows the transpositions, first to last, from position i to its final position
                // (solve_generic_kernel explains); the entries of x by position are only read
                __syncthreads();
                for (uint32_t i = tid; i < n; i += NT)
                {
                    uint32_t p = i;
#pragma unroll 8
                    for (uint32_t k = 0; k < TotalRank; k++)
                    {
                        const uint32_t pk = perm_s[k];
                        p                 = (p == k) ? pk : ((p == pk) ? k : p);
                    }
                    a.x[(size_t)b * n + i] = xs[p];
                }
            }
            GSTAMP(8)
            GSTAMP_WRITE
        }
    } // namespace

    // ---------------------------------------------------------------------------------------------
    // launchers
    // ---------------------------------------------------------------------------------------------
    namespace
    {
        static_assert(sizeof(Shared) == kGenericSharedBytes, "generic_lds_bytes (lexls_lds.h) counts the Shared block");

        template <int NT, bool LDSMAT>
        hipError_t launch_lqr_t(const LseArgs &a, bool write_factor, bool do_solve, hipStream_t s)
        {
            const size_t lds = generic_lds_bytes(a.ldp, a.nVar, a.nObj, NT, LDSMAT);
            hipError_t e     = set_lds(lqr_generic_kernel<NT, LDSMAT>, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((lqr_generic_kernel<NT, LDSMAT>), dim3(a.batch), dim3(NT), lds, s, a, write_factor ? 1 : 0, do_solve ? 1 : 0);
            return hipGetLastError();
        }
    } // namespace

    hipError_t launch_lqr_generic(LseArgs a, uint32_t max_rows, KernelId id, bool write_factor, bool do_solve, hipStream_t s)
    {
        a.ldp = odd_ld(max_rows);
        switch (id)
        {
        case KernelId::generic_64_lds: return launch_lqr_t<64, true>(a, write_factor, do_solve, s);
        case KernelId::generic_256_lds: return launch_lqr_t<256, true>(a, write_factor, do_solve, s);
        case KernelId::generic_1024_lds: return launch_lqr_t<1024, true>(a, write_factor, do_solve, s);
        case KernelId::generic_1024_hbm: return launch_lqr_t<1024, false>(a, true, do_solve, s);
        default: return hipErrorInvalidValue; // (none: nVar too large for the norm table)
        }
    }

    namespace
    {
        /// LOD <- rows of the resident constraint data (Objective::formLexLSE, objective.h:434-494, done on the device): one
        /// workgroup per problem; consecutive threads write consecutive rows of one LOD column (coalesced stores)
        __global__ __launch_bounds__(256) void gather_rows_kernel(LseArgs a, const double *cdata, uint64_t per_problem, const uint32_t *row_src,
                                                                  const uint32_t *row_ld, double *dst)
        {
            const uint32_t b = blockIdx.x;
            if (a.skip && a.skip[b]) return;
            const uint32_t n = a.nVar, cap = a.cap;
            const double *src   = cdata + (size_t)b * per_problem;
            double *out         = dst + (size_t)b * cap * (n + 1);
            const uint32_t *rs  = row_src + (size_t)b * cap;
            const uint32_t *rl  = row_ld + (size_t)b * cap;
            for (uint32_t idx = threadIdx.x; idx < cap * (n + 1); idx += blockDim.x)
            {
                const uint32_t r = idx % cap, j = idx / cap;
                const uint32_t l = rl[r];
                if (l == 0) continue;
                const uint32_t ld = l & 0x7fffffffu, ub = l >> 31;
                out[idx] = src[rs[r] + (size_t)(j < n ? j : n + ub) * ld];
            }
        }

    } // namespace

    hipError_t launch_gather_rows(const LseArgs &a, const double *d_cdata, uint64_t per_problem, const uint32_t *d_row_src, const uint32_t *d_row_ld,
                                  double *d_dst, hipStream_t s)
    {
        hipLaunchKernelGGL(gather_rows_kernel, dim3(a.batch), dim3(256), 0, s, a, d_cdata, per_problem, d_row_src, d_row_ld, d_dst);
        return hipGetLastError();
    }
} // namespace lexls
