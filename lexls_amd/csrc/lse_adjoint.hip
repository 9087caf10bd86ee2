// The adjoint family of the LexLSE solve: gradients of x = M b + N x_fixed of a KEPT factor with respect to the right-hand sides and the fixed
// values (one cotangent or many per pass), the solve map M on a new right-hand side, and the gradient with respect to the matrix that chains
// them, each on ONE view of the factor and ONE rule for a level's rank (KeptFactor, trusted_rank: lse_kept_factor.h), each a sequence of the
// steps that lse_kept_steps.h states once (wave_*: one vector per wavefront; lane_*: lane = vector; shared_*: work of the problem).
// Tolerance contract; no atomics.
#include "lexls_launch.h"
#include "lse_kept_factor.h"
#include "lse_kept_steps.h"
#include "lse_spd_solve.h"
#include <cstdlib>
#include <cstring>

namespace lexls
{
    namespace
    {
        // adjoint of factorize()'s right-hand-side updates + solve(): grad_rhs = M^T g, grad_fixed = N^T g  (x = M b + N x_fixed for fixed A)
        /// One wavefront per problem, the factor read where it is kept (never staged): every pass has the lanes along the ROWS of one factor
        /// column — consecutive addresses — and ends in a wavefront sum, so no step sends 64 requests a column apart.  Columns go AU at a time:
        /// their first 64 rows are requested together, then the (dependent) steps consume them.
        /// LDS (adjoint_lds_bytes): gh = g in factor column order (nVar), cb = the gradient of the right-hand side, LOD row order (cap; y of
        /// level k = R_k^-T gh_k is written straight into rows F .. F + rank of it), the transpositions (nVar words).
        template <int NT>
        __global__ __launch_bounds__(NT) void solve_adjoint_kernel(LseArgs a, const double *__restrict__ g, double *__restrict__ grad_rhs, double *__restrict__ grad_fixed)
        {
            static_assert(NT == 64, "one wavefront per problem: the reductions are wavefront sums");
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, lane = threadIdx.x;
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W, *hh = kf.hh;
            double *gh = smem, *cb = smem + n;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(cb + cap);

            // ---- (a) gh = P^T g: variable i sits at the position it reaches by following the transpositions first to last ----
            wave_step_a<NT>(a.perm + (size_t)b * n, g + (size_t)b * n, perm_l, gh, cb, n, cap, T, lane);

            // ---- (b) the reverse of solve(), levels ascending: y = R_k^-T gh_k, then gh -= [T_k]^T y on the pivot columns of the later levels ----
            kf.for_levels_ascending([&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                wave_reverse_solve_level<NT>(W, cap, gh, cb, F, Fc, rank, T, lane);
            });

            // ---- (c) the reverse of factorize()'s right-hand-side updates, levels descending: the transposed Gauss step (the multipliers L sit in
            // the level's pivot columns, rows of the later levels), then the level's reflectors, last first ----
            kf.for_levels_descending(kf.total_rows(), [&](uint32_t k, uint32_t dim, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                const uint32_t Fn = F + dim;
                if (k + 1 < nObj && Fn < M) wave_gauss_transposed<NT>(W, cap, cb, F, Fn, M, Fc, rank, lane);
                wave_reflectors_reversed<NT>(W, hh, cap, cb, F, Fc, dim, rank, lane);
            });
            __syncthreads();

            // ---- (d) grad_rhs = cb (rows behind the problem's own stay 0); grad_fixed_j = gh_j - (column j of the fixed variables)^T cb ----
            wave_step_d<NT>(W, gh, cb, grad_rhs, grad_fixed, b, n, cap, kf.nf, M, lane);
        }

        /// solve_adjoint_kernel for a factor of a REGULARIZED factorize() of type 1, 3, 4, 5, 8 or 9 with a constant factor per level (f = a.reg_factor,
        /// held fixed as A is): x = M_reg b + N_reg x_fixed is still affine, and grad_rhs = M_reg^T g, grad_fixed = N_reg^T g.  Forward, level k
        /// replaces its right-hand side y (rows F .. F + rank, behind the reflectors) by y' = P y + Q r when rank > 0 and |f| >= 1e-15 (P = W D^-1 W^T,
        /// Q = mu W D^-1 U^T, D the level's damped normal matrix (shared_damped_normal_matrix), mu = f^2; W = [R | T] for types 1, 5, 8 and R for 3, 4;
        /// U = the rows of the null-space basis NS above the level's columns at entry to the level, absent for 4 and 5; type 9: y' = f y), and types
        /// 1, 3, 8 then give NS's right-hand side column r new rows and subtract L y' from it, L = [U_R ; I] R^-1.  Steps (a), (b), (d) and the Gauss
        /// and reflector parts of (c) are solve_adjoint_kernel's.  New: the rebuild of NS from the factor (types 1, 3, 8; A side only — in the factor's FINAL column order: the
        /// forward column swaps act on NS and on T alike, and D, W t and U t do not change under a common permutation of their columns) with a
        /// snapshot of U per level; in (c) behind the transposed Gauss step, with r~ the cotangent of r (zero behind the last level):
        ///     types 1, 3, 8:  y~' -= R^-T (U_R^T r~[0, m0) + r~[m0, m0 + rank)), the level's own rows of r~ dropped
        ///     damped:         t = D^-1 W^T y~',  y~ = W t,  r~[0, m0) += mu U t           (type 9: y~ = f y~')
        /// IN_LDS: NS, D and the snapshots in LDS (adjoint_reg_lds_bytes), else in `work` (adjoint_reg_matrix_doubles per problem).  No atomics
        template <int NT, bool IN_LDS>
        __global__ __launch_bounds__(NT) void solve_adjoint_reg_kernel(LseArgs a, const double *__restrict__ g, double *__restrict__ grad_rhs, double *__restrict__ grad_fixed,
                                                                       double *__restrict__ work)
        {
            static_assert(NT == 64, "one wavefront per problem: the reductions are wavefront sums");
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, lane = threadIdx.x;
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, nf = kf.nf, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W, *hh = kf.hh;
            const RegularizedLevels reg = regularized_levels_of(a, b);
            double *gh = smem, *cb = gh + n, *rbar = cb + cap, *dv = rbar + n;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(dv + n);
            // (n words behind 3 n + cap doubles: the matrices start on an 8-byte boundary at perm_l + 2 ((n + 1) / 2))
            double *mat = IN_LDS ? reinterpret_cast<double *>(perm_l + 2 * ((n + 1) / 2)) : work + (size_t)b * adjoint_reg_matrix_doubles(n, nObj);
            double *NS = mat, *D = NS + (size_t)n * n, *SN = D + (size_t)n * n;
            auto w = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double { return W[i + (size_t)j * cap]; };

            // ---- (a) gh = P^T g ----
            for (uint32_t i = lane; i < n; i += NT) rbar[i] = 0.0;
            if (reg.accum)
                for (uint32_t i = lane; i < n * n; i += NT) NS[i] = 0.0;
            wave_step_a<NT>(a.perm + (size_t)b * n, g + (size_t)b * n, perm_l, gh, cb, n, cap, T, lane);

            // ---- (b) the reverse of solve(), levels ascending (solve() reads the regularized right-hand sides: cb rows F .. F + rank are y~') ----
            kf.for_levels_ascending([&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                wave_reverse_solve_level<NT>(W, cap, gh, cb, F, Fc, rank, T, lane);
            });

            // ---- the rebuild of NS, levels ascending, U snapshot first ----
            uint32_t soff = reg.accum ? shared_rebuild_nullspace<NT>(kf, reg, w, NS, SN, lane) : 0; // doubles of SN in use

            // ---- (c) the reverse of factorize()'s right-hand-side updates, levels descending ----
            // (a plain loop, not KeptFactor's walk: under the walk this instantiation takes 134 registers instead of 117 and loses a wavefront per SIMD)
            uint32_t Fend = 0;
            for (uint32_t k = 0; k < nObj; k++) Fend += kf.dims[k];
            for (uint32_t k = nObj; k--;)
            {
                const uint32_t dim = kf.dims[k];
                const uint32_t F   = Fend - dim;
                Fend               = F;
                const auto [rank, Fc] = kf.level(k, dim);
                if (rank == 0 || F + dim > M) continue;
                const uint32_t Fn = F + dim;
                if (k + 1 < nObj && Fn < M) wave_gauss_transposed<NT>(W, cap, cb, F, Fn, M, Fc, rank, lane);
                const uint32_t m0 = Fc > nf ? Fc - nf : 0, N = reg.width(n, Fc, rank);
                const double *U   = SN; // the level's snapshot: m0 x N, leading dimension m0
                double *yb        = cb + F;
                if (reg.accum)
                {
                    soff -= m0 * N;
                    U = SN + soff;
                    // y~' -= R^-T (U_R^T r~[0, m0) + r~[m0, m0 + rank)): the sum into dv, then R^T column by column as step (b) does
                    for (uint32_t j = lane; j < rank; j += NT)
                    {
                        double acc = rbar[m0 + j];
                        for (uint32_t s = 0; s < m0; s++) acc = dfma(U[s + (size_t)j * m0], rbar[s], acc);
                        dv[j] = acc;
                    }
                    __syncthreads();
                    for (uint32_t j = 0; j < rank; j++)
                    {
                        const double *col = W + F + (size_t)(Fc + j) * cap;
                        const double s    = column_dot(col, dv, j, lane < j ? col[lane] : 0.0, lane);
                        const double vj   = (dv[j] - s) / col[j];
                        __syncthreads(); // (every lane has read dv[j])
                        if (lane == 0)
                        {
                            dv[j] = vj;
                            yb[j] -= vj;
                        }
                        __syncthreads();
                    }
                }
                const double f = reg.fac[k];
                if (reg.acts(f))
                {
                    if (reg.type == 9)
                    {
                        for (uint32_t i = lane; i < rank; i += NT) yb[i] *= f;
                    }
                    else
                    {
                        const double mu = f * f;
                        shared_damped_normal_matrix<NT>(w, U, m0, reg.accum, mu, D, n, F, Fc, rank, N, m0, lane);
                        for (uint32_t c = lane; c < N; c += NT) dv[c] = lane_wt_y<1>(w, yb, F, Fc, rank, c); // dv = W^T y~' (y~' dense: LD 1)
                        __syncthreads();
                        spd_solve<NT>(D, n, dv, N, lane); // dv = t
                        for (uint32_t i = lane; i < rank; i += NT) // y~ = W t
                        {
                            double acc = 0.0;
                            for (uint32_t c = i; c < N; c++) acc = dfma(w(F + i, Fc + c), dv[c], acc);
                            yb[i] = acc;
                        }
                        if (reg.accum)
                            for (uint32_t s = lane; s < m0; s += NT) // r~ += mu U t
                            {
                                double acc = 0.0;
                                for (uint32_t c = 0; c < N; c++) acc = dfma(U[s + (size_t)c * m0], dv[c], acc);
                                rbar[s] = dfma(mu, acc, rbar[s]);
                            }
                    }
                    __syncthreads();
                }
                wave_reflectors_reversed<NT>(W, hh, cap, cb, F, Fc, dim, rank, lane);
            }
            __syncthreads();

            // ---- (d) grad_rhs = cb; grad_fixed_j = gh_j - (column j of the fixed variables)^T cb (the fixed values enter the right-hand side
            // in front of every level, and r through y' alone) ----
            wave_step_d<NT>(W, gh, cb, grad_rhs, grad_fixed, b, n, cap, nf, M, lane);
        }

        // gradient with respect to the matrix (lexls_lse_solve_adjoint_matrix): the solve map on a new right-hand side, the assembly
        /// out = M rhs for x = M b + N x_fixed of the kept factor (fixed values zero): the transpose of solve_adjoint_kernel's steps (c), (b), (a),
        /// in that order.  One wavefront per problem, the factor read where it is kept, the right-hand side a cap-vector in LDS.  Every pass has
        /// the LANES ALONG THE ROWS of one factor column (consecutive addresses); the reflector dot products are the only cross-lane traffic
        /// (wave_sum).  rhs is batch x cap in LOD row order; only_level (may be NULL): rows outside level only_level[b] are read as zero (< 0: all
        /// of them).  out is batch x nVar in the order of x, zero on fixed and free variables.
        /// LDS (adjoint_lds_bytes): z = the solution in factor column order (nVar), t = the right-hand side (cap), the transpositions (nVar words).
        /// FIXED (lexls_lse_solve_rhs): a fixed variable takes its slot of fixed (batch x nVar, slot j < nfixed) instead of zero.
        template <int NT, bool FIXED = false>
        __global__ __launch_bounds__(NT) void apply_solve_map_kernel(LseArgs a, const double *__restrict__ rhs, const int32_t *__restrict__ only_level, double *__restrict__ out,
                                                                     const double *__restrict__ fixed)
        {
            static_assert(NT == 64, "one wavefront per problem: the reductions are wavefront sums");
            constexpr uint32_t AU = 4;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, lane = threadIdx.x;
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, nf = kf.nf, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W, *hh = kf.hh;
            const uint32_t *dims = kf.dims;
            double *z = smem, *t = smem + n;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(t + cap);
            uint32_t lo = 0, hi = M; // the rows of rhs that count
            if (only_level)
            {
                const int32_t ks = only_level[b];
                lo = hi = 0;
                if (ks >= 0 && (uint32_t)ks < nObj)
                {
                    for (uint32_t k = 0; k < (uint32_t)ks; k++) lo += dims[k];
                    hi = lo + dims[ks];
                    if (hi > M) hi = M;
                }
            }
            for (uint32_t i = lane; i < n; i += NT) perm_l[i] = a.perm[(size_t)b * n + i];
            for (uint32_t i = lane; i < n; i += NT) z[i] = 0.0;
            for (uint32_t i = lane; i < cap; i += NT) t[i] = (i >= lo && i < hi) ? rhs[(size_t)b * cap + i] : 0.0;
            __syncthreads();

            // ---- (c)^T factorize()'s right-hand-side updates, levels ascending: the level's reflectors, first to last, then the Gauss step (the
            // multipliers L sit in the level's pivot columns, rows of the later levels) ----
            uint32_t F = 0;
            for (uint32_t k = 0; k < nObj; k++)
            {
                const uint32_t dim = dims[k];
                const auto [rank, Fc] = kf.level(k, dim);
                if (rank > 0 && F + dim <= M)
                {
                    // the reflectors on rows F + j .. F + dim - 1, AU at a time: their scalars and first 64 rows are requested together
                    for (uint32_t j0 = 0; j0 < rank; j0 += AU)
                    {
                        double e[AU], tau[AU];
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++)
                        {
                            const uint32_t j = j0 + u;
                            const bool on    = j < rank;
                            tau[u] = on ? hh[F + j] : 0.0;
                            e[u]   = (on && lane + 1 < dim - j) ? W[F + j + 1 + lane + (size_t)(Fc + j) * cap] : 0.0;
                        }
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++)
                        {
                            const uint32_t j = j0 + u;
                            if (j >= rank) break;
                            apply_stored_reflector(W + F + j + 1 + (size_t)(Fc + j) * cap, t + F + j, dim - j, tau[u], e[u], lane);
                        }
                    }
                    const uint32_t Fn = F + dim;
                    if (k + 1 < nObj && Fn < M)
                    {
                        for (uint32_t i = lane; i < M - Fn; i += NT) // a row of the later levels: its multipliers against the level's top
                        {
                            double acc = t[Fn + i];
                            uint32_t p = 0;
                            for (; p + AU <= rank; p += AU)
                            {
                                double w[AU];
#pragma unroll
                                for (uint32_t u = 0; u < AU; u++) w[u] = W[Fn + i + (size_t)(Fc + p + u) * cap];
#pragma unroll
                                for (uint32_t u = 0; u < AU; u++) acc = dfma(-w[u], t[F + p + u], acc);
                            }
                            for (; p < rank; p++) acc = dfma(-W[Fn + i + (size_t)(Fc + p) * cap], t[F + p], acc);
                            t[Fn + i] = acc;
                        }
                        __syncthreads();
                    }
                }
                F += dim;
            }

            // ---- (b)^T solve(), levels descending: the top of the level minus [T_k] z on the pivot columns of the later levels, then the
            // triangle column by column, last first: z_c = t_c / R_cc, t[rows above] -= W[rows, c] z_c ----
            uint32_t Fend = F;
            for (uint32_t k = nObj; k--;)
            {
                const uint32_t dim = dims[k];
                F                  = Fend - dim;
                Fend               = F;
                const auto [rank, Fc] = kf.level(k, dim);
                if (rank == 0 || F + dim > M) continue;
                for (uint32_t i = lane; i < rank; i += NT)
                {
                    double acc = t[F + i];
                    uint32_t c = T;
                    for (; c >= Fc + rank + AU; c -= AU)
                    {
                        double w[AU];
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++) w[u] = W[F + i + (size_t)(c - 1 - u) * cap];
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++) acc = dfma(-w[u], z[c - 1 - u], acc);
                    }
                    for (; c > Fc + rank; c--) acc = dfma(-W[F + i + (size_t)(c - 1) * cap], z[c - 1], acc);
                    t[F + i] = acc;
                }
                __syncthreads();
                // (the column and the diagonal entry of the NEXT step are requested before the division of the current one)
                double wcur = (lane + 1 < rank) ? W[F + lane + (size_t)(Fc + rank - 1) * cap] : 0.0;
                double dcur = W[F + rank - 1 + (size_t)(Fc + rank - 1) * cap];
                for (uint32_t j = rank; j--;)
                {
                    const double wnext = (j >= 1 && lane + 1 < j) ? W[F + lane + (size_t)(Fc + j - 1) * cap] : 0.0;
                    const double dnext = j >= 1 ? W[F + j - 1 + (size_t)(Fc + j - 1) * cap] : 1.0;
                    const double zc    = t[F + j] / dcur; // every lane for itself: no hand-off (row j is not written in this step)
                    if (lane == 0) z[Fc + j] = zc;
                    if (lane < j) t[F + lane] = dfma(-wcur, zc, t[F + lane]);
                    for (uint32_t i = lane + 64; i < j; i += 64) t[F + i] = dfma(-W[F + i + (size_t)(Fc + j) * cap], zc, t[F + i]);
                    __syncthreads();
                    wcur = wnext;
                    dcur = dnext;
                }
            }
            __syncthreads();

            // ---- (a)^T out = P z: variable i takes the entry of the position it reaches by following the transpositions first to last ----
            for (uint32_t i = lane; i < n; i += NT)
            {
                const uint32_t p       = position_after_transpositions(perm_l, T, i);
                if constexpr (FIXED)
                    out[(size_t)b * n + i] = p < nf ? fixed[(size_t)b * n + p] : (p < T ? z[p] : 0.0);
                else
                    out[(size_t)b * n + i] = (p >= nf && p < T) ? z[p] : 0.0;
            }
        }

        /// k*[b] = the last level of non-zero rank as apply_solve_map_kernel trusts the ranks (-1: none — every variable fixed, or no pivot at all):
        /// the level whose multipliers and whose share of y the matrix gradient needs.  One thread per problem.
        __global__ __launch_bounds__(64) void adjoint_matrix_level_kernel(LseArgs a, int32_t *__restrict__ kstar)
        {
            const uint32_t b = blockIdx.x * 64 + threadIdx.x;
            if (b >= a.batch) return;
            const KeptFactor kf = kept_factor_of(a, b);
            int32_t ks = -1;
            uint32_t F = 0;
            for (uint32_t k = 0; k < kf.nObj; k++)
            {
                const uint32_t dim = kf.dims[k];
                const auto [rank, Fc] = kf.level(k, dim);
                if (rank > 0 && F + dim <= kf.M) ks = (int32_t)k;
                F += dim;
            }
            kstar[b] = ks;
        }

        /// G[b] (nVar + 1 columns of cap rows, the layout of the problem data: entry (row i, column j) at j * cap + i):
        ///     column j < nVar = - y x_j - lambda u_j,   column nVar = y
        /// with x the solution (a.x), y = M^T g (batch x cap), lambda the multipliers of level kstar[b] as sensitivity_kernel leaves them (batch x
        /// (nVar + cap): row i at nfixed + i), u = M y~ (batch x nVar).  Rows behind the problem's own are zero.
        /// differentiable[b] (may be NULL) = 1 where the problem is RANK-STABLE: every variable fixed, or rank_k == min(dim_k, nVar - Fc_k) for every
        /// level k (Fc_k the level's first column; 0 where Fc_k >= nVar) — else 0, and the whole of G[b] is exact zeros.
        /// One workgroup of NT / 64 wavefronts per problem: a wavefront takes every (NT / 64)-th column, its lanes run along the rows, so every store
        /// is a run of consecutive addresses.  LDS: x and u (2 nVar doubles).  No atomics: same bits run to run.
        /// Not on the KeptFactor view, on purpose: it walks no factor.  Its rule is about the STORED ranks (never trusted_rank), it needs neither T
        /// nor the factor, and it reads nfixed as stored — unclamped for the flag, held to nVar where it indexes lam
        template <int NT>
        __global__ __launch_bounds__(NT) void adjoint_matrix_kernel(LseArgs a, const double *__restrict__ y, const double *__restrict__ lam, const double *__restrict__ u,
                                                                    const int32_t *__restrict__ kstar, double *__restrict__ G, uint8_t *__restrict__ differentiable)
        {
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
            const uint32_t n = a.nVar, cap = a.cap, nObj = a.nObj;
            const uint32_t *dims = a.dims + (size_t)b * nObj, *rk = a.rank + (size_t)b * nObj, *fc = a.fcol + (size_t)b * nObj;
            const uint32_t nf = a.nfixed ? a.nfixed[b] : 0;
            double *xs = smem, *us = smem + n;
            for (uint32_t i = tid; i < n; i += NT)
            {
                xs[i] = a.x[(size_t)b * n + i];
                us[i] = u[(size_t)b * n + i];
            }
            uint32_t M   = 0;
            bool stable  = true; // (uniform: every thread evaluates the rule for itself)
            for (uint32_t k = 0; k < nObj; k++)
            {
                const uint32_t room = fc[k] < n ? n - fc[k] : 0;
                if (rk[k] != (dims[k] < room ? dims[k] : room)) stable = false;
                M += dims[k];
            }
            if (nf >= n) stable = true;
            if (M > cap) M = cap;
            if (tid == 0 && differentiable) differentiable[b] = stable ? 1 : 0;
            const bool with_lambda = kstar[b] >= 0;
            __syncthreads();
            double *Gb = G + (size_t)b * cap * (n + 1);
            for (uint32_t i = lane; i < cap; i += 64)
            {
                const bool own  = stable && i < M;
                const double yi = own ? y[(size_t)b * cap + i] : 0.0;
                const double li = (own && with_lambda) ? lam[(size_t)b * (n + cap) + (nf < n ? nf : n) + i] : 0.0;
                for (uint32_t j = wave; j <= n; j += NT / 64)
                {
                    double val = 0.0;
                    if (own) val = j < n ? dfma(-li, us[j], -(yi * xs[j])) : yi;
                    Gb[(size_t)j * cap + i] = val;
                }
            }
        }

        /// solve_adjoint_kernel's steps (a)-(d) for up to 64 cotangents of one problem at once, LANE = COTANGENT: one wavefront per (problem,
        /// tile of 64 cotangents), lane l of tile t owns cotangent 64 t + l; lanes beyond ncot compute on zeros and store nothing.  Everything
        /// that steers the control flow (dims, ranks, first columns, tau == 0) belongs to the problem, so it is wavefront-uniform; every factor
        /// entry is the same for all lanes (STAGED: a broadcast read of the image stage_factor left in LDS; else a read of the stored factor at
        /// a wavefront-uniform address); every dot product is the lane's own serial dfma chain in ascending row order — no cross-lane
        /// reduction and no barrier between the steps, and a cotangent's bits do not depend on its lane, its tile or its neighbours.
        /// LDS (adjoint_multi_lds_bytes): gh[nVar][LD], cb[cap][LD], LD = 65 (odd: "lane = cotangent" walks take consecutive words, the
        /// transposed walks of the load and store phases a stride of 65 words — both conflict-free), the transpositions and the position
        /// each variable reaches (2 nVar words), then STAGED the factor's nVar columns (odd leading dimension) and hh.
        /// Global traffic: a tile's rows of G, grad_rhs and grad_fixed are contiguous; consecutive lanes take consecutive addresses and the
        /// transposition happens in LDS.  No atomics.
        template <int NT, bool STAGED>
        __global__ __launch_bounds__(NT) void solve_adjoint_multi_kernel(LseArgs a, const double *__restrict__ G, uint32_t ncot, double *__restrict__ grad_rhs,
                                                                         double *__restrict__ grad_fixed)
        {
            static_assert(NT == 64, "one wavefront per (problem, tile): lane = cotangent");
            constexpr uint32_t LD = kAdjointMultiLd;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x;
            if (b >= a.batch || tile * 64u >= ncot) return; // (block-uniform)
            const uint32_t kt = ncot - tile * 64u < 64u ? ncot - tile * 64u : 64u; // live cotangents of this tile
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W;
            double *gh       = smem;
            double *cb       = gh + (size_t)n * LD;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(cb + (size_t)cap * LD);
            uint32_t *pos_l  = perm_l + n;
            double *L        = reinterpret_cast<double *>(pos_l + n); // (2 n words: still 8-byte aligned)
            const uint32_t ldl = cap | 1u; // odd_ld(cap)
            double *hh_l       = L + (size_t)ldl * n;
            // entry (r, c) of the factor, r < M <= cap, c < T <= nVar; the Householder scalar of row r < cap
            auto Wat = [&](uint32_t r, uint32_t c) __attribute__((always_inline)) -> double { return STAGED ? L[r + c * ldl] : W[r + (size_t)c * cap]; };
            auto tau_at = [&](uint32_t r) __attribute__((always_inline)) -> double { return STAGED ? hh_l[r] : kf.hh[r]; };
            const size_t row0 = (size_t)b * ncot + (size_t)tile * 64u; // the tile's kt rows of G, grad_rhs and grad_fixed are contiguous from here

            // ---- staging, and (a) gh = P^T g for every cotangent of the tile ----
            for (uint32_t i = lane; i < n; i += NT) perm_l[i] = a.perm[(size_t)b * n + i];
            for (uint32_t i = lane; i < (n + cap) * LD; i += NT) smem[i] = 0.0; // gh and cb (dead lanes, absent rows, unreached positions: zeros)
            if (STAGED)
            {
                for (uint32_t i = lane; i < cap; i += NT) hh_l[i] = kf.hh[i];
                stage_factor<NT>(W, L, cap, n, ldl, lane); // (ends in a barrier)
            }
            else
                __syncthreads();
            for (uint32_t i = lane; i < n; i += NT) pos_l[i] = position_after_transpositions(perm_l, T, i);
            __syncthreads();
            lane_gather_by_position<NT, LD>(G + row0 * n, pos_l, gh, kt, n, lane);
            __syncthreads();
            double *ghl = gh + lane, *cbl = cb + lane; // this lane's column of the state

            // ---- (b) the reverse of solve(), levels ascending ----
            kf.for_levels_ascending([&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                lane_reverse_solve_level<LD>(Wat, ghl, cbl, F, Fc, rank, T);
            });

            // ---- (c) the reverse of factorize()'s right-hand-side updates, levels descending: the transposed Gauss step, then the level's
            // reflectors, last first ----
            kf.for_levels_descending(kf.total_rows(), [&](uint32_t k, uint32_t dim, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                const uint32_t Fn = F + dim;
                if (k + 1 < nObj && Fn < M) lane_gauss_transposed<LD>(Wat, cbl, F, Fn, M, Fc, rank);
                lane_reflectors_reversed<LD>(Wat, tau_at, cbl, F, Fc, dim, rank);
            });

            // ---- (d) grad_fixed_j = gh_j - (column j of the fixed variables)^T cb, left in gh_j; then both outputs, transposed through LDS ----
            lane_step_d<NT, LD>(Wat, gh, cb, grad_rhs, grad_fixed, row0, kt, n, cap, kf.nf, M, lane);
        }

        /// solve_adjoint_reg_kernel's steps (a)-(d) for up to 64 cotangents of one problem at once, LANE = COTANGENT, the way
        /// solve_adjoint_multi_kernel recasts solve_adjoint_kernel: one wavefront per (problem, tile of 64 cotangents); lanes beyond ncot compute on
        /// zeros and store nothing.  Two kinds of phases alternate, with barriers between them:
        ///   SHARED (work of the problem, the lanes spread over rows and entries: the shared_* steps solve_adjoint_reg_kernel calls too): the rebuild
        ///     of NS with a snapshot of U per level (types 1, 3, 8), and per damped level the formation of D and its LL^T (spd_factor<NT>,
        ///     lse_spd_solve.h: either form).  EVERY TILE REPEATS THIS WORK.
        ///   PER LANE (work of the cotangent): steps (b), (c), (d) on the lane's own column of gh, cb, r~ and dv (LDS, [index][lane], leading
        ///     dimension 65); every dot product, substitution and matrix-vector product is the lane's own serial dfma chain in a fixed order — among
        ///     them the two triangular substitutions against the shared L, row by row (entry i receives the products j = 0 .. i-1, backwards
        ///     j = N-1 .. i+1, the order of spd_solve's column sweeps).  No cross-lane reduction on cotangent data: a cotangent's bits do not depend
        ///     on its lane, its tile or its neighbours.  Not promised bit-equal to solve_adjoint_reg_kernel (whose dot products are wavefront sums).
        /// Everything that steers the control flow (dims, ranks, first columns, tau == 0, the |f| < 1e-15 gate, the type) belongs to the problem:
        /// wavefront-uniform.  The factor is read where it is kept, at wavefront-uniform addresses.
        /// IN_LDS: NS, D and the snapshots behind the state in LDS (adjoint_reg_multi_lds_bytes), read by broadcast; else in `work`,
        /// adjoint_reg_matrix_doubles per (problem, tile), at wavefront-uniform addresses.  No atomics.
        template <int NT, bool IN_LDS>
        __global__ __launch_bounds__(NT) void solve_adjoint_reg_multi_kernel(LseArgs a, const double *__restrict__ G, uint32_t ncot, double *__restrict__ grad_rhs,
                                                                             double *__restrict__ grad_fixed, double *__restrict__ work)
        {
            static_assert(NT == 64, "one wavefront per (problem, tile): lane = cotangent");
            constexpr uint32_t LD = kAdjointMultiLd;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x;
            if (b >= a.batch || tile * 64u >= ncot) return; // (block-uniform)
            const uint32_t kt = ncot - tile * 64u < 64u ? ncot - tile * 64u : 64u; // live cotangents of this tile
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, nf = kf.nf, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W, *hh = kf.hh;
            const RegularizedLevels reg = regularized_levels_of(a, b);
            double *gh = smem, *cb = gh + (size_t)n * LD, *rbar = cb + (size_t)cap * LD, *dv = rbar + (size_t)n * LD;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(dv + (size_t)n * LD);
            uint32_t *pos_l  = perm_l + n;
            // (2 n words: the matrices start on an 8-byte boundary)
            double *mat = IN_LDS ? reinterpret_cast<double *>(pos_l + n) : work + ((size_t)b * gridDim.y + tile) * adjoint_reg_matrix_doubles(n, nObj);
            double *NS = mat, *D = NS + (size_t)n * n, *SN = D + (size_t)n * n;
            auto w = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double { return W[i + (size_t)j * cap]; };
            auto tau_at = [&](uint32_t r) __attribute__((always_inline)) -> double { return hh[r]; };
            const size_t row0 = (size_t)b * ncot + (size_t)tile * 64u; // the tile's kt rows of G, grad_rhs and grad_fixed are contiguous from here

            // ---- (a) gh = P^T g for every cotangent of the tile; the rest of the state zero ----
            for (uint32_t i = lane; i < n; i += NT) perm_l[i] = a.perm[(size_t)b * n + i];
            for (uint32_t i = lane; i < (3 * n + cap) * LD; i += NT) smem[i] = 0.0;
            if (reg.accum)
                for (uint32_t i = lane; i < n * n; i += NT) NS[i] = 0.0;
            __syncthreads();
            for (uint32_t i = lane; i < n; i += NT) pos_l[i] = position_after_transpositions(perm_l, T, i);
            __syncthreads();
            lane_gather_by_position<NT, LD>(G + row0 * n, pos_l, gh, kt, n, lane);
            __syncthreads();
            double *ghl = gh + lane, *cbl = cb + lane, *rbl = rbar + lane, *dvl = dv + lane; // this lane's column of the state

            // ---- (b) the reverse of solve(), levels ascending (cb rows F .. F + rank are y~'), per lane ----
            kf.for_levels_ascending([&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                lane_reverse_solve_level<LD>(w, ghl, cbl, F, Fc, rank, T);
            });

            // ---- SHARED: the rebuild of NS, levels ascending, U snapshot first ----
            uint32_t soff = reg.accum ? shared_rebuild_nullspace<NT>(kf, reg, w, NS, SN, lane) : 0; // doubles of SN in use

            // ---- (c) the reverse of factorize()'s right-hand-side updates, levels descending ----
            kf.for_levels_descending(kf.total_rows(), [&](uint32_t k, uint32_t dim, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                const uint32_t Fn = F + dim;
                if (k + 1 < nObj && Fn < M) lane_gauss_transposed<LD>(w, cbl, F, Fn, M, Fc, rank);
                const uint32_t m0 = Fc > nf ? Fc - nf : 0, N = reg.width(n, Fc, rank);
                const double *U   = SN; // the level's snapshot: m0 x N, leading dimension m0
                double *yb        = cbl + F * LD;
                if (reg.accum)
                {
                    soff -= m0 * N;
                    U = SN + soff;
                    // y~' -= R^-T (U_R^T r~[0, m0) + r~[m0, m0 + rank)): the sum into dv, then R^T row by row
                    for (uint32_t j = 0; j < rank; j++)
                    {
                        double acc = rbl[(m0 + j) * LD];
                        for (uint32_t s = 0; s < m0; s++) acc = dfma(U[s + (size_t)j * m0], rbl[s * LD], acc);
                        dvl[j * LD] = acc;
                    }
                    for (uint32_t j = 0; j < rank; j++)
                    {
                        double s = 0.0;
                        for (uint32_t i = 0; i < j; i++) s = dfma(w(F + i, Fc + j), dvl[i * LD], s);
                        const double vj = (dvl[j * LD] - s) / w(F + j, Fc + j);
                        dvl[j * LD]     = vj;
                        yb[j * LD] -= vj;
                    }
                }
                const double f = reg.fac[k];
                if (reg.acts(f)) // (uniform)
                {
                    if (reg.type == 9)
                    {
                        for (uint32_t i = 0; i < rank; i++) yb[i * LD] *= f;
                    }
                    else
                    {
                        const double mu = f * f;
                        // SHARED: D and its LL^T
                        shared_damped_normal_matrix<NT>(w, U, m0, reg.accum, mu, D, n, F, Fc, rank, N, m0, lane);
                        __syncthreads();
                        spd_factor<NT>(D, n, N, lane); // (ends in a barrier: every lane reads all of L from here on)
                        // PER LANE: dv = W^T y~', then L z = dv and L^T t = z in place, y~ = W t, r~ += mu U t
                        for (uint32_t c = 0; c < N; c++) dvl[c * LD] = lane_wt_y<LD>(w, yb, F, Fc, rank, c);
                        lane_spd_substitute<LD>(D, n, dvl, N);
                        lane_w_t<LD>(w, yb, dvl, F, Fc, rank, N);
                        if (reg.accum)
                            for (uint32_t s = 0; s < m0; s++)
                            {
                                double acc = 0.0;
                                for (uint32_t c = 0; c < N; c++) acc = dfma(U[s + (size_t)c * m0], dvl[c * LD], acc);
                                rbl[s * LD] = dfma(mu, acc, rbl[s * LD]);
                            }
                        __syncthreads(); // (every lane has read L: the next damped level overwrites D)
                    }
                }
                lane_reflectors_reversed<LD>(w, tau_at, cbl, F, Fc, dim, rank);
            });

            // ---- (d) grad_fixed_j = gh_j - (column j of the fixed variables)^T cb, left in gh_j; then both outputs, transposed through LDS ----
            lane_step_d<NT, LD>(w, gh, cb, grad_rhs, grad_fixed, row0, kt, n, cap, nf, M, lane);
        }

        // forward-mode tangents (lexls_lse_solve_tangent): the two right-hand sides from the direction, the solve map on many right-hand sides
        /// One pass over the direction d[A | b] of tangent c = blockIdx.y of problem b = blockIdx.x (dlod: ntan x batch x the layout of the problem
        /// data): per row i of the problem's own   r_i = db_i - sum_j dA_ij x_j - sum_{j < nf} W(i, j) dfixed_j   (the last sum is the fixed
        /// slots' share of the right-hand side: the transpose of solve_adjoint_kernel's step (d), the untouched columns j < nf of the factor),
        /// per column j   w_j = sum_i dA_ij lambda_i   (lambda: the multipliers of level kstar[b] as sensitivity_kernel leaves them, row i at
        /// nfixed + i; zero without such a level).  R is batch x ntan x cap (zero behind the problem's own rows), Wv batch x ntan x nVar in the
        /// order of x: the layouts launch_solve_adjoint_multi reads and writes.
        /// One wavefront, the LANES ALONG THE ROWS of one column of the direction (consecutive addresses), AU columns requested together; every
        /// entry of the problem's own rows is loaded exactly once, no entry behind them is loaded at all.  r_i is the lane's own dfma chain over
        /// the columns in ascending order; w_j is one wavefront sum per column and trip of 64 rows, the trips added in ascending order by lane 0.
        /// LDS (tangent_rhs_lds_bytes): x, w, the fixed slots' tangents (nVar each), lambda (cap).  No atomics.
        template <int NT>
        __global__ __launch_bounds__(NT) void tangent_rhs_kernel(LseArgs a, const double *__restrict__ dlod, const double *__restrict__ dfixed, const double *__restrict__ lam,
                                                                 const int32_t *__restrict__ kstar, uint32_t ntan, double *__restrict__ R, double *__restrict__ Wv)
        {
            static_assert(NT == 64, "one wavefront per (problem, tangent): the column sums are wavefront sums");
            constexpr uint32_t AU = 8;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
            if (b >= a.batch || c >= ntan) return; // (block-uniform)
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nf = kf.nf, M = kf.M;
            const double *__restrict__ W = kf.W;
            double *xs = smem, *ws = xs + n, *df = ws + n, *ls = df + n;
            const bool with_lambda = kstar[b] >= 0;
            const size_t slot      = (size_t)c * a.batch + b; // tangent-major inputs
            for (uint32_t i = lane; i < n; i += NT)
            {
                xs[i] = a.x[(size_t)b * n + i];
                ws[i] = 0.0;
                df[i] = (dfixed && i < nf) ? dfixed[slot * n + i] : 0.0;
            }
            for (uint32_t i = lane; i < cap; i += NT) ls[i] = (with_lambda && i < M) ? lam[(size_t)b * (n + cap) + nf + i] : 0.0;
            __syncthreads();
            const double *__restrict__ D = dlod + slot * (size_t)cap * (n + 1);
            double *Rb = R + ((size_t)b * ntan + c) * cap;
            for (uint32_t i0 = 0; i0 < cap; i0 += NT)
            {
                const uint32_t i = i0 + lane;
                const bool live  = i < M;
                if (i0 < M) // (uniform) a trip with rows of the problem's own
                {
                    double acc      = live ? D[(size_t)n * cap + i] : 0.0;
                    const double li = live ? ls[i] : 0.0;
                    for (uint32_t j0 = 0; j0 < n; j0 += AU)
                    {
                        double v[AU], s[AU];
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++) v[u] = (live && j0 + u < n) ? D[(size_t)(j0 + u) * cap + i] : 0.0;
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++)
                        {
                            if (j0 + u < n) acc = dfma(-v[u], xs[j0 + u], acc);
                            s[u] = wave_sum(v[u] * li);
                        }
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++)
                            if (lane == 0 && j0 + u < n) ws[j0 + u] += s[u];
                    }
                    for (uint32_t j0 = 0; j0 < nf; j0 += AU)
                    {
                        double v[AU];
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++) v[u] = (live && j0 + u < nf) ? W[i + (size_t)(j0 + u) * cap] : 0.0;
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++)
                            if (j0 + u < nf) acc = dfma(-v[u], df[j0 + u], acc);
                    }
                    if (i < cap) Rb[i] = live ? acc : 0.0;
                }
                else if (i < cap)
                    Rb[i] = 0.0;
            }
            __syncthreads();
            for (uint32_t j = lane; j < n; j += NT) Wv[((size_t)b * ntan + c) * n + j] = ws[j];
        }

        /// dx = M (R - E_k* Y) + the fixed slots, for up to 64 right-hand sides of one problem at once, LANE = RIGHT-HAND SIDE: the transpose of
        /// solve_adjoint_multi_kernel's steps (c), (b), (a), in that order — apply_solve_map_kernel's mathematics, solve_adjoint_multi_kernel's
        /// division of the work.  One wavefront per (problem, tile of 64 tangents), lane l of tile t owns tangent 64 t + l; lanes beyond ntan
        /// compute on zeros and store nothing.  Everything that steers the control flow belongs to the problem (wavefront-uniform); every factor
        /// entry is the same for all lanes; every sum is the lane's own serial dfma chain in a fixed order — no cross-lane sum, no barrier
        /// between the steps, and a tangent's bits do not depend on its lane, its tile or its neighbours.
        /// R, Y: batch x ntan x cap (tangent_rhs_kernel's r; M^T w as launch_solve_adjoint(_multi) leaves it: only its rows of level kstar[b] are
        /// read and subtracted).  dfixed (may be NULL: zeros), dx: ntan x batch x nVar; dx_i = the fixed slot's tangent where variable i is
        /// fixed, z of its pivot column, 0 where it is free.  differentiable[b] (may be NULL; written by tile 0) = adjoint_matrix_kernel's
        /// rank-stability rule on the STORED ranks; a problem that fails it gets exact zeros in all its rows of dx.
        /// PLACE (TangentPlacement, lexls_lds.h): 0 the state z[nVar][LD], t[cap][LD] (LD = 65) and the staged factor in LDS, 1 the state in LDS
        /// and the factor read where it is kept, 2 the state in `work` (tangent_map_work_doubles per (problem, tile), LD = 64).  No atomics.
        /// TANGENT == false (lexls_lse_solve_rhs): x = M R + the fixed slots for EVERY problem — no rank-stability rule, no flags, Y and kstar unread.
        template <int NT, int PLACE, bool TANGENT = true>
        __global__ __launch_bounds__(NT) void apply_solve_map_multi_kernel(LseArgs a, const double *__restrict__ R, const double *__restrict__ Y, const int32_t *__restrict__ kstar,
                                                                           const double *__restrict__ dfixed, uint32_t ntan, double *__restrict__ dx,
                                                                           uint8_t *__restrict__ differentiable, double *work)
        {
            static_assert(NT == 64, "one wavefront per (problem, tile): lane = right-hand side");
            constexpr bool STAGED = PLACE == 0, IN_WORK = PLACE == 2;
            constexpr uint32_t LD = IN_WORK ? kTangentWorkLd : kAdjointMultiLd;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x;
            if (b >= a.batch || tile * 64u >= ntan) return; // (block-uniform)
            const uint32_t kt = ntan - tile * 64u < 64u ? ntan - tile * 64u : 64u; // live tangents of this tile
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, nf = kf.nf, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W;
            const uint32_t *dims = kf.dims;
            double *state    = IN_WORK ? work + ((size_t)b * gridDim.y + tile) * tangent_map_work_doubles(n, cap) : smem;
            double *z        = state;
            double *t        = z + (size_t)n * LD;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(IN_WORK ? smem : t + (size_t)cap * LD);
            uint32_t *pos_l  = perm_l + n;
            double *L        = reinterpret_cast<double *>(pos_l + n); // (2 n words: still 8-byte aligned)
            const uint32_t ldl = cap | 1u;                            // odd_ld(cap)
            double *hh_l       = L + (size_t)ldl * n;
            auto Wat = [&](uint32_t r, uint32_t c) __attribute__((always_inline)) -> double { return STAGED ? L[r + c * ldl] : W[r + (size_t)c * cap]; };
            auto tau_at = [&](uint32_t r) __attribute__((always_inline)) -> double { return STAGED ? hh_l[r] : kf.hh[r]; };

            // the rank-stability rule of adjoint_matrix_kernel (the STORED ranks and nfixed as stored; uniform)
            bool stable = true;
            if constexpr (TANGENT)
            {
                for (uint32_t k = 0; k < nObj; k++)
                {
                    const uint32_t room = kf.fc[k] < n ? n - kf.fc[k] : 0;
                    if (kf.rk[k] != (dims[k] < room ? dims[k] : room)) stable = false;
                }
                if ((a.nfixed ? a.nfixed[b] : 0u) >= n) stable = true;
                if (tile == 0 && lane == 0 && differentiable) differentiable[b] = stable ? 1 : 0;
            }
            const size_t B = a.batch;
            if (!stable) // (uniform) no derivative: exact zeros
            {
                for (uint32_t e = lane; e < kt * n; e += NT)
                {
                    const uint32_t c = e / n, i = e - c * n;
                    dx[(((size_t)tile * 64u + c) * B + b) * n + i] = 0.0;
                }
                return;
            }
            uint32_t lo = 0, hi = 0; // the rows of level k*: Y counts there alone
            if constexpr (TANGENT)
            {
                const int32_t ks = kstar[b];
                if (ks >= 0 && (uint32_t)ks < nObj)
                {
                    for (uint32_t k = 0; k < (uint32_t)ks; k++) lo += dims[k];
                    hi = lo + dims[ks];
                    if (hi > M) hi = M;
                }
            }

            // ---- staging; t = R - E_k* Y for every tangent of the tile, z = 0 ----
            for (uint32_t i = lane; i < n; i += NT) perm_l[i] = a.perm[(size_t)b * n + i];
            for (uint32_t i = lane; i < (n + cap) * LD; i += NT) state[i] = 0.0; // (dead lanes, absent rows, unreached columns: zeros)
            if (STAGED)
            {
                for (uint32_t i = lane; i < cap; i += NT) hh_l[i] = kf.hh[i];
                stage_factor<NT>(W, L, cap, n, ldl, lane); // (ends in a barrier)
            }
            else
                __syncthreads();
            for (uint32_t i = lane; i < n; i += NT) pos_l[i] = position_after_transpositions(perm_l, T, i);
            lane_load_rhs<NT, LD>(R, Y, ((size_t)b * ntan + (size_t)tile * 64u) * cap, lo, hi, t, kt, cap, M, lane);
            __syncthreads();
            double *zl = z + lane, *tl = t + lane; // this lane's column of the state

            // ---- (c)^T factorize()'s right-hand-side updates, levels ascending: the level's reflectors, first to last, then the Gauss step ----
            const uint32_t rows = kf.for_levels_ascending([&](uint32_t k, uint32_t dim, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                lane_reflectors_forward<LD>(Wat, tau_at, tl, F, Fc, dim, rank);
                const uint32_t Fn = F + dim;
                if (k + 1 < nObj && Fn < M) lane_gauss<LD>(Wat, tl, F, Fn, M, Fc, rank);
            });

            // ---- (b)^T solve(), levels descending: the top of the level minus [T_k] z on the pivot columns of the later levels, then the
            // triangle, last column first ----
            kf.for_levels_descending(rows, [&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                lane_back_substitute_level<LD>(Wat, tl, zl, F, Fc, rank, T);
            });
            __syncthreads();

            // ---- (a)^T dx = P z, and the fixed slots: variable i takes the entry of the position it reaches by the transpositions ----
            for (uint32_t e = lane; e < kt * n; e += NT)
            {
                const uint32_t c = e / n, i = e - c * n, p = pos_l[i];
                const size_t row = ((size_t)tile * 64u + c) * B + b;
                double val       = 0.0;
                if (p < nf)
                    val = dfixed ? dfixed[row * n + p] : 0.0;
                else if (p < T)
                    val = z[p * LD + c];
                dx[row * n + i] = val;
            }
        }

        /// lexls_lse_residual_rhs: get_v() and the cost per level for up to 64 right-hand sides of one problem at once on the kept, UNDAMPED factor,
        /// LANE = RIGHT-HAND SIDE — apply_solve_map_multi_kernel<NT, PLACE, false>'s pass (the same steps on the same state in the same order: dx,
        /// where asked for, has that kernel's bits), and behind it the residual of every level out of what the pass left in t:
        ///     v_k = Q_k [0 ; -tail_k],   tail_k = rows rank_k .. dim_k - 1 of the level's transformed right-hand side   (lane_level_residual)
        /// a level of rank 0 (also: every variable fixed, or no pivot column left) has no Q: v_k = -t_k.  cost[c, b, k] = the lane's own fma chain over
        /// the level's rows of v, in row order.  No cross-lane sum, no barrier between the steps: a right-hand side's bits do not depend on its lane,
        /// its tile or its neighbours.  One wavefront per (problem, tile of 64 right-hand sides); lanes beyond nrhs compute on zeros and store nothing.
        /// R: batch x nrhs x cap and fixed: nrhs x batch x nVar (solve_rhs_front_kernel's); dx (nrhs x batch x nVar), v (nrhs x batch x cap, zeros
        /// behind the problem's own rows), cost (nrhs x batch x nObj): each may be NULL.  PLACE: TangentPlacement, the state where that kernel keeps
        /// it (the same LDS, the same work doubles per (problem, tile)).  No atomics.
        template <int NT, int PLACE>
        __global__ __launch_bounds__(NT) void residual_rhs_kernel(LseArgs a, const double *__restrict__ R, const double *__restrict__ fixed, uint32_t nrhs, double *__restrict__ dx,
                                                                  double *__restrict__ v, double *__restrict__ cost, double *work)
        {
            static_assert(NT == 64, "one wavefront per (problem, tile): lane = right-hand side");
            constexpr bool STAGED = PLACE == 0, IN_WORK = PLACE == 2;
            constexpr uint32_t LD = IN_WORK ? kTangentWorkLd : kAdjointMultiLd;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x;
            if (b >= a.batch || tile * 64u >= nrhs) return; // (block-uniform)
            const uint32_t kt = nrhs - tile * 64u < 64u ? nrhs - tile * 64u : 64u; // live right-hand sides of this tile
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, nf = kf.nf, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W;
            double *state    = IN_WORK ? work + ((size_t)b * gridDim.y + tile) * tangent_map_work_doubles(n, cap) : smem;
            double *z        = state;
            double *t        = z + (size_t)n * LD;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(IN_WORK ? smem : t + (size_t)cap * LD);
            uint32_t *pos_l  = perm_l + n;
            double *L        = reinterpret_cast<double *>(pos_l + n); // (2 n words: still 8-byte aligned)
            const uint32_t ldl = cap | 1u;                            // odd_ld(cap)
            double *hh_l       = L + (size_t)ldl * n;
            auto Wat = [&](uint32_t r, uint32_t c) __attribute__((always_inline)) -> double { return STAGED ? L[r + c * ldl] : W[r + (size_t)c * cap]; };
            auto tau_at = [&](uint32_t r) __attribute__((always_inline)) -> double { return STAGED ? hh_l[r] : kf.hh[r]; };
            const size_t B = a.batch;

            // ---- staging; t = R for every right-hand side of the tile, z = 0 ----
            for (uint32_t i = lane; i < n; i += NT) perm_l[i] = a.perm[(size_t)b * n + i];
            for (uint32_t i = lane; i < (n + cap) * LD; i += NT) state[i] = 0.0; // (dead lanes, absent rows, unreached columns: zeros)
            if (STAGED)
            {
                for (uint32_t i = lane; i < cap; i += NT) hh_l[i] = kf.hh[i];
                stage_factor<NT>(W, L, cap, n, ldl, lane); // (ends in a barrier)
            }
            else
                __syncthreads();
            for (uint32_t i = lane; i < n; i += NT) pos_l[i] = position_after_transpositions(perm_l, T, i);
            lane_load_rhs<NT, LD>(R, nullptr, ((size_t)b * nrhs + (size_t)tile * 64u) * cap, 0, 0, t, kt, cap, M, lane);
            __syncthreads();
            double *zl = z + lane, *tl = t + lane; // this lane's column of the state

            // ---- factorize()'s right-hand-side updates, levels ascending, then solve(), levels descending: apply_solve_map_multi_kernel's ----
            const uint32_t rows = kf.for_levels_ascending([&](uint32_t k, uint32_t dim, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                lane_reflectors_forward<LD>(Wat, tau_at, tl, F, Fc, dim, rank);
                const uint32_t Fn = F + dim;
                if (k + 1 < nObj && Fn < M) lane_gauss<LD>(Wat, tl, F, Fn, M, Fc, rank);
            });
            if (dx) // (uniform) the solution is asked for too
            {
                kf.for_levels_descending(rows, [&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                    lane_back_substitute_level<LD>(Wat, tl, zl, F, Fc, rank, T);
                });
                __syncthreads();
                for (uint32_t e = lane; e < kt * n; e += NT)
                {
                    const uint32_t c = e / n, i = e - c * n, p = pos_l[i];
                    const size_t row = ((size_t)tile * 64u + c) * B + b;
                    dx[row * n + i]  = p < nf ? fixed[row * n + p] : (p < T ? z[p * LD + c] : 0.0);
                }
            }

            // ---- get_v(), every level of the problem's own rows (a level of rank 0 too): in place on the lane's column of t ----
            uint32_t F = 0, k = 0;
            for (; k < nObj; k++)
            {
                const uint32_t dim = kf.dims[k];
                if (F + dim > M) break; // (rows the problem does not hold: zeros from here on)
                const auto [rank, Fc] = kf.level(k, dim);
                const double ck       = lane_level_residual<LD>(Wat, tau_at, tl, F, Fc, dim, rank);
                if (cost && lane < kt) cost[(((size_t)tile * 64u + lane) * B + b) * nObj + k] = ck;
                F += dim;
            }
            for (; k < nObj; k++)
                if (cost && lane < kt) cost[(((size_t)tile * 64u + lane) * B + b) * nObj + k] = 0.0;
            if (!v) return;
            __syncthreads();
            for (uint32_t e = lane; e < kt * cap; e += NT)
            {
                const uint32_t c = e / cap, r = e - c * cap;
                v[(((size_t)tile * 64u + c) * B + b) * cap + r] = r < F ? t[r * LD + c] : 0.0;
            }
        }

        // new right-hand sides on the kept factor (lexls_lse_solve_rhs): the kernel in front of the map, the map of a damped factor
        /// Right-hand side c = blockIdx.y of problem b = blockIdx.x (rhs: nrhs x batch x cap, LOD row order; fixed: nrhs x batch x nVar, slot
        /// j < nfixed, NULL: the values the handle holds, a.fixed_val): per row i of the problem's own
        ///     R_i = rhs_i - sum_{j < nf} W(i, j) fixed_j
        /// (the untouched columns j < nf of the factor are A_fixed: where tangent_rhs_kernel takes it), R batch x nrhs x cap with zeros behind the
        /// problem's own rows, and Fx (nrhs x batch x nVar) = the fixed values in their slots, zero behind them: the layouts the map kernels read.
        /// Rows behind the problem's own and slots behind nfixed are never loaded.  One wavefront, the LANES ALONG THE ROWS of one factor column;
        /// R_i is the lane's own dfma chain over the fixed columns in ascending order.  LDS: the fixed values (nVar doubles).  No atomics.
        template <int NT>
        __global__ __launch_bounds__(NT) void solve_rhs_front_kernel(LseArgs a, const double *__restrict__ rhs, const double *__restrict__ fixed, uint32_t nrhs,
                                                                     double *__restrict__ R, double *__restrict__ Fx)
        {
            constexpr uint32_t AU = 8;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
            if (b >= a.batch || c >= nrhs) return; // (block-uniform)
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nf = kf.nf, M = kf.M;
            const double *__restrict__ W = kf.W;
            const size_t slot = (size_t)c * a.batch + b; // right-hand-side-major inputs
            double *fx = smem;
            for (uint32_t j = lane; j < n; j += NT)
            {
                const double v   = j < nf ? (fixed ? fixed[slot * n + j] : a.fixed_val[(size_t)b * n + j]) : 0.0;
                fx[j]            = v;
                Fx[slot * n + j] = v;
            }
            __syncthreads();
            double *Rb = R + ((size_t)b * nrhs + c) * cap;
            for (uint32_t i = lane; i < cap; i += NT)
            {
                double acc = 0.0;
                if (i < M)
                {
                    acc = rhs[slot * cap + i];
                    for (uint32_t j0 = 0; j0 < nf; j0 += AU)
                    {
                        double v[AU];
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++) v[u] = j0 + u < nf ? W[i + (size_t)(j0 + u) * cap] : 0.0;
#pragma unroll
                        for (uint32_t u = 0; u < AU; u++)
                            if (j0 + u < nf) acc = dfma(-v[u], fx[j0 + u], acc);
                    }
                }
                Rb[i] = acc;
            }
        }

        /// x = M_reg R + the fixed slots for up to 64 right-hand sides of one problem at once on a factor of a REGULARIZED factorize() of type 1,
        /// 3, 4, 5, 8 or 9 with a constant factor per level: the transpose of solve_adjoint_reg_multi_kernel, with its mapping — one wavefront
        /// per (problem, tile of 64 right-hand sides), LANE = RIGHT-HAND SIDE; lanes beyond nrhs compute on zeros and store nothing.  The forward
        /// pass of the damped solve on the kept factor alone, levels ascending; per level of rank > 0:
        ///     the level's reflectors on the lane's column t, first to last; y = t[F, F + rank)
        ///     |f| >= 1e-15:  y' = W D^-1 (W^T y + mu U^T r)  (types 4, 5: no U; type 9: y' = f y), D the level's damped normal matrix, mu = f^2
        ///     types 1, 3, 8:  s = R^-1 y',  r[0, m0) -= U_R s,  r[m0, m0 + rank) = -s   (r = the right-hand-side column of the basis)
        ///     the Gauss step with y' on the rows of the later levels
        /// then the block back-substitution and the permutation.  U = the rows [0, m0) of the null-space basis
        /// NS above the level's columns AS IT STANDS — the levels are walked in the order in which the basis grows, so no snapshot is kept — and
        /// the basis takes the level's step (shared_nullspace_level: A side only, the factor's final column order) behind the lanes' work.
        ///   SHARED phases (work of the problem, lanes over entries): D and its LL^T (spd_factor<NT>), the step of NS.  EVERY TILE REPEATS THEM.
        ///   PER LANE phases: everything on t, z, r and dv ([index][lane]): the lane's own serial dfma chains in a fixed order, no cross-lane
        ///     sum — a right-hand side's bits do not depend on its lane, its tile or its neighbours.
        /// Everything that steers the control flow belongs to the problem (wavefront-uniform).  The factor is read where it is kept.
        /// PLACE (SolveRhsRegForm, lexls_lds.h): 0 state (LD = 65) and NS, D in LDS; 1 the state in LDS, NS and D in `work`; 2 both in `work`
        /// (state LD = 64).  R: batch x nrhs x cap, fixed and x: nrhs x batch x nVar.  No atomics.
        template <int NT, int PLACE>
        __global__ __launch_bounds__(NT) void apply_solve_map_reg_multi_kernel(LseArgs a, const double *__restrict__ R, const double *__restrict__ fixed, uint32_t nrhs,
                                                                               double *__restrict__ x, double *work)
        {
            static_assert(NT == 64, "one wavefront per (problem, tile): lane = right-hand side");
            constexpr bool MAT_LDS = PLACE == 0, IN_WORK = PLACE == 2;
            constexpr uint32_t LD = IN_WORK ? kTangentWorkLd : kAdjointMultiLd;
            extern __shared__ double smem[];
            const uint32_t b = blockIdx.x, tile = blockIdx.y, lane = threadIdx.x;
            if (b >= a.batch || tile * 64u >= nrhs) return; // (block-uniform)
            const uint32_t kt = nrhs - tile * 64u < 64u ? nrhs - tile * 64u : 64u; // live right-hand sides of this tile
            const KeptFactor kf = kept_factor_of(a, b);
            const uint32_t n = kf.n, cap = kf.cap, nObj = kf.nObj, nf = kf.nf, T = kf.T, M = kf.M;
            const double *__restrict__ W = kf.W, *hh = kf.hh;
            const RegularizedLevels reg = regularized_levels_of(a, b);
            const size_t per_tile = MAT_LDS ? 0 : solve_rhs_reg_matrix_doubles(n) + (IN_WORK ? solve_rhs_reg_state_doubles(n, cap, LD) : 0);
            double *wb       = MAT_LDS ? nullptr : work + ((size_t)b * gridDim.y + tile) * per_tile;
            double *state    = IN_WORK ? wb + solve_rhs_reg_matrix_doubles(n) : smem;
            double *t = state, *z = t + (size_t)cap * LD, *rv = z + (size_t)n * LD, *dv = rv + (size_t)n * LD;
            uint32_t *perm_l = reinterpret_cast<uint32_t *>(IN_WORK ? smem : dv + (size_t)n * LD);
            uint32_t *pos_l  = perm_l + n;
            double *mat      = MAT_LDS ? reinterpret_cast<double *>(pos_l + n) : wb; // (2 n words: still 8-byte aligned)
            double *NS = mat, *D = NS + (size_t)n * n;
            auto ns = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double & { return NS[i + (size_t)j * n]; };
            auto w  = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double { return W[i + (size_t)j * cap]; };
            auto tau_at = [&](uint32_t r) __attribute__((always_inline)) -> double { return hh[r]; };

            // ---- t = R for every right-hand side of the tile, the rest of the state zero ----
            for (uint32_t i = lane; i < n; i += NT) perm_l[i] = a.perm[(size_t)b * n + i];
            for (uint32_t i = lane; i < (3 * n + cap) * LD; i += NT) state[i] = 0.0; // (dead lanes, absent rows, unreached columns: zeros)
            if (reg.accum)
                for (uint32_t i = lane; i < n * n; i += NT) NS[i] = 0.0;
            __syncthreads();
            for (uint32_t i = lane; i < n; i += NT) pos_l[i] = position_after_transpositions(perm_l, T, i);
            lane_load_rhs<NT, LD>(R, nullptr, ((size_t)b * nrhs + (size_t)tile * 64u) * cap, 0, 0, t, kt, cap, M, lane);
            __syncthreads();
            double *tl = t + lane, *zl = z + lane, *rl = rv + lane, *dvl = dv + lane; // this lane's column of the state

            // ---- the forward pass of factorize()'s right-hand-side updates, levels ascending ----
            const uint32_t rows = kf.for_levels_ascending([&](uint32_t k, uint32_t dim, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                lane_reflectors_forward<LD>(w, tau_at, tl, F, Fc, dim, rank); // PER LANE
                const uint32_t m0 = Fc > nf ? Fc - nf : 0, N = reg.width(n, Fc, rank);
                double *yb        = tl + F * LD;
                const double f    = reg.fac[k];
                if (reg.acts(f)) // (uniform)
                {
                    if (reg.type == 9)
                    {
                        for (uint32_t i = 0; i < rank; i++) yb[i * LD] *= f;
                    }
                    else
                    {
                        const double mu = f * f;
                        // SHARED: D (U = the basis in place) and its LL^T
                        shared_damped_normal_matrix<NT>(w, NS + (size_t)Fc * n, n, reg.accum, mu, D, n, F, Fc, rank, N, m0, lane);
                        __syncthreads();
                        spd_factor<NT>(D, n, N, lane); // (ends in a barrier: every lane reads all of L from here on)
                        // PER LANE: dv = W^T y + mu U^T r, then L q = dv and L^T p = q in place, y' = W p
                        for (uint32_t c = 0; c < N; c++)
                        {
                            double acc = lane_wt_y<LD>(w, yb, F, Fc, rank, c);
                            if (reg.accum)
                            {
                                double up = 0.0;
                                for (uint32_t s = 0; s < m0; s++) up = dfma(ns(s, Fc + c), rl[s * LD], up);
                                acc = dfma(mu, up, acc);
                            }
                            dvl[c * LD] = acc;
                        }
                        lane_spd_substitute<LD>(D, n, dvl, N);
                        lane_w_t<LD>(w, yb, dvl, F, Fc, rank, N);
                    }
                }
                if (reg.accum)
                {
                    // PER LANE: s = R^-1 y' (into dv, last row first), r[0, m0) -= U_R s, r[m0, m0 + rank) = -s
                    for (uint32_t j = rank; j--;)
                    {
                        double acc = yb[j * LD];
                        for (uint32_t q = j + 1; q < rank; q++) acc = dfma(-w(F + j, Fc + q), dvl[q * LD], acc);
                        dvl[j * LD] = acc / w(F + j, Fc + j);
                    }
                    for (uint32_t s = 0; s < m0; s++)
                    {
                        double acc = rl[s * LD];
                        for (uint32_t j = 0; j < rank; j++) acc = dfma(-ns(s, Fc + j), dvl[j * LD], acc);
                        rl[s * LD] = acc;
                    }
                    for (uint32_t j = 0; j < rank; j++) rl[(m0 + j) * LD] = -dvl[j * LD];
                }
                __syncthreads(); // (every lane has read L and U: the step of NS and the next damped level overwrite them)
                if (reg.accum) shared_nullspace_level<NT>(w, NS, n, F, Fc, m0, rank, lane); // SHARED: the basis takes the level's step
                const uint32_t Fn = F + dim;
                if (k + 1 < nObj && Fn < M) lane_gauss<LD>(w, tl, F, Fn, M, Fc, rank); // PER LANE
            });

            // ---- solve(), levels descending, on the damped right-hand sides, per lane ----
            kf.for_levels_descending(rows, [&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
                lane_back_substitute_level<LD>(w, tl, zl, F, Fc, rank, T);
            });
            __syncthreads();

            // ---- x = P z, and the fixed slots ----
            const size_t B = a.batch;
            for (uint32_t e = lane; e < kt * n; e += NT)
            {
                const uint32_t c = e / n, i = e - c * n, p = pos_l[i];
                const size_t row = ((size_t)tile * 64u + c) * B + b;
                x[row * n + i]   = p < nf ? fixed[row * n + p] : (p < T ? z[p * LD + c] : 0.0);
            }
        }
    } // namespace

    size_t adjoint_reg_work_bytes(const LseArgs &a)
    {
        return (a.reg_type == 0 || adjoint_reg_in_lds(a.nVar, a.cap, a.nObj)) ? 0 : 8 * (size_t)a.batch * adjoint_reg_matrix_doubles(a.nVar, a.nObj);
    }

    hipError_t launch_solve_adjoint(const LseArgs &a, const double *d_g, double *d_grad_rhs, double *d_grad_fixed, hipStream_t s, const char **variant, double *d_work)
    {
        if (a.reg_type != 0) // a regularized factor: the served types with a constant factor per level (the callers refuse the others)
        {
            if (!adjoint_reg_serves(a.reg_type) || a.reg_variable != 0.0 || !a.reg_factor) return hipErrorInvalidValue;
            const bool in_lds = adjoint_reg_in_lds(a.nVar, a.cap, a.nObj);
            const size_t lds  = adjoint_reg_lds_bytes(a.nVar, a.cap, a.nObj, in_lds);
            if (lds > kMaxLdsBytes || (!in_lds && !d_work)) return hipErrorInvalidValue;
            hipError_t e = in_lds ? set_lds(solve_adjoint_reg_kernel<64, true>, lds) : set_lds(solve_adjoint_reg_kernel<64, false>, lds);
            if (e != hipSuccess) return e;
            if (in_lds)
                hipLaunchKernelGGL((solve_adjoint_reg_kernel<64, true>), dim3(a.batch), dim3(64), lds, s, a, d_g, d_grad_rhs, d_grad_fixed, nullptr);
            else
                hipLaunchKernelGGL((solve_adjoint_reg_kernel<64, false>), dim3(a.batch), dim3(64), lds, s, a, d_g, d_grad_rhs, d_grad_fixed, d_work);
            if (variant) *variant = adjoint_reg_form_name(in_lds);
            return hipGetLastError();
        }
        const size_t lds = adjoint_lds_bytes(a.nVar, a.cap);
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        hipError_t e = set_lds(solve_adjoint_kernel<64>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((solve_adjoint_kernel<64>), dim3(a.batch), dim3(64), lds, s, a, d_g, d_grad_rhs, d_grad_fixed);
        if (variant) *variant = "solve_adjoint<64>";
        return hipGetLastError();
    }

    /// the form launch_solve_adjoint_multi takes for a shape: adjoint_multi_form (lexls_lds.h), unless LEXLS_ADJOINT_MULTI_FORM = staged | hbm |
    /// single names a later form of the list (measurements: a form whose LDS does not fit is never forced)
    static AdjointMultiForm adjoint_multi_form_for(uint32_t nVar, uint32_t cap)
    {
        AdjointMultiForm f = adjoint_multi_form(nVar, cap);
        if (const char *e = std::getenv("LEXLS_ADJOINT_MULTI_FORM"))
        {
            if (!std::strcmp(e, "single")) f = AdjointMultiForm::per_cotangent;
            if (!std::strcmp(e, "hbm") && f == AdjointMultiForm::staged) f = AdjointMultiForm::hbm;
        }
        return f;
    }

    /// the same for a regularized factor: adjoint_reg_multi_form (lexls_lds.h), unless LEXLS_ADJOINT_REG_MULTI_FORM = hbm | single names a later form
    /// of the list (measurements)
    static AdjointRegMultiForm adjoint_reg_multi_form_for(uint32_t nVar, uint32_t cap, uint32_t nObj)
    {
        AdjointRegMultiForm f = adjoint_reg_multi_form(nVar, cap, nObj);
        if (const char *e = std::getenv("LEXLS_ADJOINT_REG_MULTI_FORM"))
        {
            if (!std::strcmp(e, "single")) f = AdjointRegMultiForm::per_cotangent;
            if (!std::strcmp(e, "hbm") && f == AdjointRegMultiForm::lds) f = AdjointRegMultiForm::hbm;
        }
        return f;
    }
    static bool adjoint_multi_per_cotangent(const LseArgs &a)
    {
        return a.reg_type != 0 ? adjoint_reg_multi_form_for(a.nVar, a.cap, a.nObj) == AdjointRegMultiForm::per_cotangent
                               : adjoint_multi_form_for(a.nVar, a.cap) == AdjointMultiForm::per_cotangent;
    }

    size_t adjoint_multi_work_bytes(const LseArgs &a) { return adjoint_multi_per_cotangent(a) ? 8 * (size_t)a.batch * (2 * (size_t)a.nVar + a.cap) : 0; }

    size_t adjoint_reg_multi_work_bytes(const LseArgs &a, uint32_t ncot)
    {
        if (a.reg_type == 0 || adjoint_reg_multi_form_for(a.nVar, a.cap, a.nObj) != AdjointRegMultiForm::hbm) return 0;
        return 8 * (size_t)a.batch * ((ncot + 63u) / 64u) * adjoint_reg_matrix_doubles(a.nVar, a.nObj);
    }

    hipError_t launch_solve_adjoint_multi(const LseArgs &a, const double *d_G, uint32_t ncot, double *d_grad_rhs, double *d_grad_fixed, double *d_work, hipStream_t s,
                                          const char **variant, double *d_reg_work, double *d_reg_multi_work)
    {
        const uint32_t tiles = (ncot + 63u) / 64u;
        if (ncot == 0 || tiles > 65535u) return hipErrorInvalidValue;
        const bool reg = a.reg_type != 0;
        if (reg && (!adjoint_reg_serves(a.reg_type) || a.reg_variable != 0.0 || !a.reg_factor)) return hipErrorInvalidValue;
        const AdjointRegMultiForm rf = adjoint_reg_multi_form_for(a.nVar, a.cap, a.nObj);
        const AdjointMultiForm f     = adjoint_multi_form_for(a.nVar, a.cap);
        if (variant) *variant = reg ? adjoint_reg_multi_form_name(rf, adjoint_reg_in_lds(a.nVar, a.cap, a.nObj)) : adjoint_multi_form_name(f);
        if (adjoint_multi_per_cotangent(a))
        {
            // the single-cotangent kernel reads and writes one row per problem, a problem after the other: cotangent c's rows (a stride of ncot
            // rows apart) travel through three buffers of that layout
            if (!d_work) return hipErrorInvalidValue;
            const size_t B = a.batch, n = a.nVar, cap = a.cap;
            double *w_g = d_work, *w_rhs = w_g + B * n, *w_fixed = w_rhs + B * cap;
            for (uint32_t c = 0; c < ncot; c++)
            {
                hipError_t e = hipMemcpy2DAsync(w_g, 8 * n, d_G + (size_t)c * n, 8 * n * ncot, 8 * n, B, hipMemcpyDeviceToDevice, s);
                if (e == hipSuccess) e = launch_solve_adjoint(a, w_g, w_rhs, d_grad_fixed ? w_fixed : nullptr, s, nullptr, d_reg_work);
                if (e == hipSuccess) e = hipMemcpy2DAsync(d_grad_rhs + (size_t)c * cap, 8 * cap * ncot, w_rhs, 8 * cap, 8 * cap, B, hipMemcpyDeviceToDevice, s);
                if (e == hipSuccess && d_grad_fixed) e = hipMemcpy2DAsync(d_grad_fixed + (size_t)c * n, 8 * n * ncot, w_fixed, 8 * n, 8 * n, B, hipMemcpyDeviceToDevice, s);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        }
        if (reg)
        {
            const bool in_lds = rf == AdjointRegMultiForm::lds;
            const size_t lds  = adjoint_reg_multi_lds_bytes(a.nVar, a.cap, a.nObj, in_lds);
            if (lds > kMaxLdsBytes || (!in_lds && !d_reg_multi_work)) return hipErrorInvalidValue;
            hipError_t e = in_lds ? set_lds(solve_adjoint_reg_multi_kernel<64, true>, lds) : set_lds(solve_adjoint_reg_multi_kernel<64, false>, lds);
            if (e != hipSuccess) return e;
            if (in_lds)
                hipLaunchKernelGGL((solve_adjoint_reg_multi_kernel<64, true>), dim3(a.batch, tiles), dim3(64), lds, s, a, d_G, ncot, d_grad_rhs, d_grad_fixed, nullptr);
            else
                hipLaunchKernelGGL((solve_adjoint_reg_multi_kernel<64, false>), dim3(a.batch, tiles), dim3(64), lds, s, a, d_G, ncot, d_grad_rhs, d_grad_fixed, d_reg_multi_work);
            return hipGetLastError();
        }
        const bool staged = f == AdjointMultiForm::staged;
        const size_t lds  = adjoint_multi_lds_bytes(a.nVar, a.cap, staged);
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        hipError_t e = staged ? set_lds(solve_adjoint_multi_kernel<64, true>, lds) : set_lds(solve_adjoint_multi_kernel<64, false>, lds);
        if (e != hipSuccess) return e;
        if (staged)
            hipLaunchKernelGGL((solve_adjoint_multi_kernel<64, true>), dim3(a.batch, tiles), dim3(64), lds, s, a, d_G, ncot, d_grad_rhs, d_grad_fixed);
        else
            hipLaunchKernelGGL((solve_adjoint_multi_kernel<64, false>), dim3(a.batch, tiles), dim3(64), lds, s, a, d_G, ncot, d_grad_rhs, d_grad_fixed);
        return hipGetLastError();
    }

    hipError_t launch_apply_solve_map(const LseArgs &a, const double *d_rhs, const int32_t *d_only_level, double *d_out, hipStream_t s)
    {
        const size_t lds = adjoint_lds_bytes(a.nVar, a.cap);
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        hipError_t e = set_lds(apply_solve_map_kernel<64>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((apply_solve_map_kernel<64>), dim3(a.batch), dim3(64), lds, s, a, d_rhs, d_only_level, d_out, nullptr);
        return hipGetLastError();
    }

    /// y (batch x cap) | u (batch x nVar) | the scratch of the sensitivity launch (sensitivity_scratch_args lays it out) | k* (batch words)
    size_t adjoint_matrix_work_bytes(const LseArgs &a)
    {
        const size_t B = a.batch;
        return 8 * B * ((size_t)a.cap + a.nVar) + ((multipliers_scratch_bytes(a) + 7) & ~(size_t)7) + 4 * B;
    }

    hipError_t launch_solve_adjoint_matrix(const LseArgs &a, const double *d_g, double *d_grad_lod, uint8_t *d_differentiable, void *d_work, uint32_t sweep_level_dim_hint,
                                           hipStream_t s, const char **variant, double *d_grad_fixed)
    {
        if (!d_work || !d_grad_lod) return hipErrorInvalidValue;
        const size_t B = a.batch, n = a.nVar, cap = a.cap;
        const size_t lds = 8 * 2 * n;
        if (lds > kMaxLdsBytes) return hipErrorInvalidValue;
        double *w_y     = static_cast<double *>(d_work);
        double *w_u     = w_y + B * cap;
        char *w_sens    = reinterpret_cast<char *>(w_u + B * n);
        int32_t *w_star = reinterpret_cast<int32_t *>(w_sens + ((multipliers_scratch_bytes(a) + 7) & ~(size_t)7));
        // y = M^T g (and, where the caller wants it, N^T g from the same launch)
        hipError_t e = launch_solve_adjoint(a, d_g, w_y, d_grad_fixed, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(adjoint_matrix_level_kernel, dim3((a.batch + 63u) / 64u), dim3(64), 0, s, a, w_star);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // the multipliers of level k* — its own rows hold the residual, so no residual launch in front of it — written, with the decisions and
        // the marks of the removal search, into this call's work buffers (the types are copied there first): what get_lambda, get_v and
        // get_multipliers answer stays what it was
        LseArgs t;
        e            = sensitivity_scratch_args(a, w_sens, s, &t);
        t.wrong_sign = nullptr;
        if (e == hipSuccess) e = launch_sensitivity(t, w_star, 0, 1e-8, 1e-12, s, false, sweep_level_dim_hint);
        // u = M y~, y~ = y on the rows of level k*
        if (e == hipSuccess) e = launch_apply_solve_map(a, w_y, w_star, w_u, s);
        if (e != hipSuccess) return e;
        if ((e = set_lds(adjoint_matrix_kernel<256>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((adjoint_matrix_kernel<256>), dim3(a.batch), dim3(256), lds, s, a, w_y, t.lambda, w_u, w_star, d_grad_lod, d_differentiable);
        if (variant) *variant = "solve_adjoint_matrix<64>";
        return hipGetLastError();
    }

    /// the placement launch_solve_tangent takes for a shape: tangent_map_placement (lexls_lds.h), unless LEXLS_TANGENT_PLACEMENT = lds | work names
    /// a later placement of the list (measurements and tests: nothing moves a shape up)
    static TangentPlacement tangent_placement_for(uint32_t nVar, uint32_t cap, uint32_t nObj)
    {
        TangentPlacement p = tangent_map_placement(nVar, cap, nObj);
        if (const char *e = std::getenv("LEXLS_TANGENT_PLACEMENT"))
        {
            if (!std::strcmp(e, "work")) p = TangentPlacement::work;
            if (!std::strcmp(e, "lds") && p == TangentPlacement::staged) p = TangentPlacement::lds;
        }
        return p;
    }

    /// r (batch x ntan x cap) | w (batch x ntan x nVar) | M^T w (batch x ntan x cap) | the scratch of the sensitivity launch | k* (batch words,
    /// padded to 8 bytes) | under the work placement the per-lane vectors of every (problem, tile)
    size_t tangent_work_bytes(const LseArgs &a, uint32_t ntan)
    {
        const size_t B = a.batch, tiles = (ntan + 63u) / 64u;
        size_t bytes = 8 * B * ntan * (2 * (size_t)a.cap + a.nVar) + ((multipliers_scratch_bytes(a) + 7) & ~(size_t)7) + ((4 * B + 7) & ~(size_t)7);
        if (tangent_placement_for(a.nVar, a.cap, a.nObj) == TangentPlacement::work) bytes += 8 * B * tiles * tangent_map_work_doubles(a.nVar, a.cap);
        return bytes;
    }

    hipError_t launch_solve_tangent(const LseArgs &a, const double *d_dlod, const double *d_dfixed, uint32_t ntan, double *d_dx, uint8_t *d_differentiable, void *d_work,
                                    double *d_adjoint_multi_work, uint32_t sweep_level_dim_hint, hipStream_t s, const char **variant)
    {
        const uint32_t tiles = (ntan + 63u) / 64u;
        if (!d_work || !d_dlod || !d_dx || ntan == 0 || ntan > 65535u) return hipErrorInvalidValue;
        const size_t B = a.batch, n = a.nVar, cap = a.cap;
        const TangentPlacement place = tangent_placement_for(a.nVar, a.cap, a.nObj);
        const size_t lds = tangent_map_lds_bytes(a.nVar, a.cap, a.nObj, place), lds_rhs = tangent_rhs_lds_bytes(a.nVar, a.cap);
        if (lds > kMaxLdsBytes || lds_rhs > kMaxLdsBytes) return hipErrorInvalidValue;
        // what the M^T w step will ask for, checked here so that a shape it cannot serve is refused before anything is enqueued: the
        // single-cotangent kernel's LDS (ntan == 1, and every cotangent of the per-cotangent form) and that form's buffers
        const bool per_cotangent = ntan > 1 && adjoint_multi_per_cotangent(a);
        if ((ntan == 1 || per_cotangent) && adjoint_lds_bytes(a.nVar, a.cap) > kMaxLdsBytes) return hipErrorInvalidValue;
        if (per_cotangent && !d_adjoint_multi_work) return hipErrorInvalidValue;
        double *w_r     = static_cast<double *>(d_work);
        double *w_w     = w_r + B * ntan * cap;
        double *w_y     = w_w + B * ntan * n;
        char *w_sens    = reinterpret_cast<char *>(w_y + B * ntan * cap);
        int32_t *w_star = reinterpret_cast<int32_t *>(w_sens + ((multipliers_scratch_bytes(a) + 7) & ~(size_t)7));
        double *w_state = reinterpret_cast<double *>(reinterpret_cast<char *>(w_star) + ((4 * B + 7) & ~(size_t)7));
        // k*, and the multipliers of level k* into this call's buffers (launch_solve_adjoint_matrix's two steps: the getters answer what they did)
        hipLaunchKernelGGL(adjoint_matrix_level_kernel, dim3((a.batch + 63u) / 64u), dim3(64), 0, s, a, w_star);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        LseArgs t;
        e            = sensitivity_scratch_args(a, w_sens, s, &t);
        t.wrong_sign = nullptr;
        if (e == hipSuccess) e = launch_sensitivity(t, w_star, 0, 1e-8, 1e-12, s, false, sweep_level_dim_hint);
        if (e == hipSuccess) e = set_lds(tangent_rhs_kernel<64>, lds_rhs);
        if (e != hipSuccess) return e;
        // r = db - dA x - A_fixed dfixed, w = dA^T lambda: the one pass over the direction
        hipLaunchKernelGGL((tangent_rhs_kernel<64>), dim3(a.batch, ntan), dim3(64), lds_rhs, s, a, d_dlod, d_dfixed, t.lambda, w_star, ntan, w_r, w_w);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // M^T w
        e = ntan == 1 ? launch_solve_adjoint(a, w_w, w_y, nullptr, s) : launch_solve_adjoint_multi(a, w_w, ntan, w_y, nullptr, d_adjoint_multi_work, s);
        if (e != hipSuccess) return e;
        // dx = M (r - E_k* M^T w) + the fixed slots
        switch (place)
        {
        case TangentPlacement::staged:
            if ((e = set_lds(apply_solve_map_multi_kernel<64, 0>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_multi_kernel<64, 0>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_y, w_star, d_dfixed, ntan, d_dx, d_differentiable, nullptr);
            break;
        case TangentPlacement::lds:
            if ((e = set_lds(apply_solve_map_multi_kernel<64, 1>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_multi_kernel<64, 1>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_y, w_star, d_dfixed, ntan, d_dx, d_differentiable, nullptr);
            break;
        case TangentPlacement::work:
            if ((e = set_lds(apply_solve_map_multi_kernel<64, 2>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_multi_kernel<64, 2>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_y, w_star, d_dfixed, ntan, d_dx, d_differentiable, w_state);
            break;
        }
        if (variant) *variant = tangent_placement_name(place);
        return hipGetLastError();
    }

    /// the form launch_solve_rhs takes on a damped factor: solve_rhs_reg_form (lexls_lds.h), unless LEXLS_SOLVE_RHS_REG_FORM = hbm | work names a
    /// later form of the list (measurements and tests: nothing moves a shape up)
    static SolveRhsRegForm solve_rhs_reg_form_for(uint32_t nVar, uint32_t cap, uint32_t nObj)
    {
        SolveRhsRegForm f = solve_rhs_reg_form(nVar, cap, nObj);
        if (const char *e = std::getenv("LEXLS_SOLVE_RHS_REG_FORM"))
        {
            if (!std::strcmp(e, "work")) f = SolveRhsRegForm::work;
            if (!std::strcmp(e, "hbm") && f == SolveRhsRegForm::lds) f = SolveRhsRegForm::hbm;
        }
        return f;
    }

    /// R (batch x nrhs x cap) | the fixed slots (nrhs x batch x nVar) | what the map keeps per (problem, tile) outside LDS
    size_t solve_rhs_work_bytes(const LseArgs &a, uint32_t nrhs)
    {
        const size_t B = a.batch, tiles = (nrhs + 63u) / 64u;
        size_t bytes = 8 * B * nrhs * ((size_t)a.cap + a.nVar);
        if (a.reg_type != 0)
            bytes += 8 * B * tiles * solve_rhs_reg_work_doubles(a.nVar, a.cap, solve_rhs_reg_form_for(a.nVar, a.cap, a.nObj));
        else if (nrhs > 1 && tangent_placement_for(a.nVar, a.cap, a.nObj) == TangentPlacement::work)
            bytes += 8 * B * tiles * tangent_map_work_doubles(a.nVar, a.cap);
        return bytes;
    }

    hipError_t launch_solve_rhs(const LseArgs &a, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x, void *d_work, hipStream_t s, const char **variant)
    {
        const uint32_t tiles = (nrhs + 63u) / 64u;
        if (!d_work || !d_rhs || !d_x || nrhs == 0 || nrhs > 65535u) return hipErrorInvalidValue;
        const bool reg = a.reg_type != 0;
        if (reg && (!adjoint_reg_serves(a.reg_type) || a.reg_variable != 0.0 || !a.reg_factor)) return hipErrorInvalidValue;
        const size_t B = a.batch, n = a.nVar, cap = a.cap;
        const TangentPlacement place = tangent_placement_for(a.nVar, a.cap, a.nObj);
        const SolveRhsRegForm form   = solve_rhs_reg_form_for(a.nVar, a.cap, a.nObj);
        const size_t lds_front = 8 * n;
        const size_t lds = reg ? solve_rhs_reg_lds_bytes(a.nVar, a.cap, a.nObj, form) : nrhs == 1 ? adjoint_lds_bytes(a.nVar, a.cap) : tangent_map_lds_bytes(a.nVar, a.cap, a.nObj, place);
        if (lds > kMaxLdsBytes || lds_front > kMaxLdsBytes) return hipErrorInvalidValue; // (before anything is enqueued)
        double *w_r = static_cast<double *>(d_work), *w_f = w_r + B * nrhs * cap, *w_state = w_f + B * nrhs * n;
        hipError_t e = set_lds(solve_rhs_front_kernel<64>, lds_front);
        if (e != hipSuccess) return e;
        // R = rhs - A_fixed fixed, and the fixed slots
        hipLaunchKernelGGL((solve_rhs_front_kernel<64>), dim3(a.batch, nrhs), dim3(64), lds_front, s, a, d_rhs, d_fixed, nrhs, w_r, w_f);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (reg)
        {
            switch (form)
            {
            case SolveRhsRegForm::lds:
                if ((e = set_lds(apply_solve_map_reg_multi_kernel<64, 0>, lds)) != hipSuccess) return e;
                hipLaunchKernelGGL((apply_solve_map_reg_multi_kernel<64, 0>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_f, nrhs, d_x, nullptr);
                break;
            case SolveRhsRegForm::hbm:
                if ((e = set_lds(apply_solve_map_reg_multi_kernel<64, 1>, lds)) != hipSuccess) return e;
                hipLaunchKernelGGL((apply_solve_map_reg_multi_kernel<64, 1>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_f, nrhs, d_x, w_state);
                break;
            case SolveRhsRegForm::work:
                if ((e = set_lds(apply_solve_map_reg_multi_kernel<64, 2>, lds)) != hipSuccess) return e;
                hipLaunchKernelGGL((apply_solve_map_reg_multi_kernel<64, 2>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_f, nrhs, d_x, w_state);
                break;
            }
            if (variant) *variant = solve_rhs_reg_form_name(form);
            return hipGetLastError();
        }
        if (nrhs == 1) // the single-vector kernel (its sums are wavefront sums: against the lane-per-vector kernels the contract is the tolerance)
        {
            if ((e = set_lds(apply_solve_map_kernel<64, true>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_kernel<64, true>), dim3(a.batch), dim3(64), lds, s, a, w_r, nullptr, d_x, w_f);
            if (variant) *variant = "solve_rhs<64,single>";
            return hipGetLastError();
        }
        switch (place)
        {
        case TangentPlacement::staged:
            if ((e = set_lds(apply_solve_map_multi_kernel<64, 0, false>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_multi_kernel<64, 0, false>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, nullptr, nullptr, w_f, nrhs, d_x, nullptr, nullptr);
            break;
        case TangentPlacement::lds:
            if ((e = set_lds(apply_solve_map_multi_kernel<64, 1, false>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_multi_kernel<64, 1, false>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, nullptr, nullptr, w_f, nrhs, d_x, nullptr, nullptr);
            break;
        case TangentPlacement::work:
            if ((e = set_lds(apply_solve_map_multi_kernel<64, 2, false>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_multi_kernel<64, 2, false>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, nullptr, nullptr, w_f, nrhs, d_x, nullptr, w_state);
            break;
        }
        if (variant) *variant = solve_rhs_placement_name(place);
        return hipGetLastError();
    }

    /// R (batch x nrhs x cap) | the fixed slots (nrhs x batch x nVar) | under the work placement the per-lane vectors of every (problem, tile)
    size_t residual_rhs_work_bytes(const LseArgs &a, uint32_t nrhs)
    {
        const size_t B = a.batch, tiles = (nrhs + 63u) / 64u;
        size_t bytes = 8 * B * nrhs * ((size_t)a.cap + a.nVar);
        if (tangent_placement_for(a.nVar, a.cap, a.nObj) == TangentPlacement::work) bytes += 8 * B * tiles * tangent_map_work_doubles(a.nVar, a.cap);
        return bytes;
    }

    hipError_t launch_residual_rhs(const LseArgs &a, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x, double *d_v, double *d_cost, void *d_work,
                                   hipStream_t s, const char **variant)
    {
        const uint32_t tiles = (nrhs + 63u) / 64u;
        if (!d_work || !d_rhs || (!d_x && !d_v && !d_cost) || nrhs == 0 || nrhs > 65535u || a.reg_type != 0) return hipErrorInvalidValue;
        const size_t B = a.batch, n = a.nVar, cap = a.cap;
        const TangentPlacement place = tangent_placement_for(a.nVar, a.cap, a.nObj); // solve_rhs's rule: the state is that kernel's
        const size_t lds_front = 8 * n, lds = tangent_map_lds_bytes(a.nVar, a.cap, a.nObj, place);
        // one right-hand side: x is the single-vector kernel's, as lexls_lse_solve_rhs's is (its sums are wavefront sums); v and cost are the lane kernel's
        const bool single_x = nrhs == 1 && d_x;
        if (lds > kMaxLdsBytes || lds_front > kMaxLdsBytes || (single_x && adjoint_lds_bytes(a.nVar, a.cap) > kMaxLdsBytes)) return hipErrorInvalidValue; // (before anything is enqueued)
        double *w_r = static_cast<double *>(d_work), *w_f = w_r + B * nrhs * cap, *w_state = w_f + B * nrhs * n;
        hipError_t e = set_lds(solve_rhs_front_kernel<64>, lds_front);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((solve_rhs_front_kernel<64>), dim3(a.batch, nrhs), dim3(64), lds_front, s, a, d_rhs, d_fixed, nrhs, w_r, w_f);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (single_x)
        {
            if ((e = set_lds(apply_solve_map_kernel<64, true>, adjoint_lds_bytes(a.nVar, a.cap))) != hipSuccess) return e;
            hipLaunchKernelGGL((apply_solve_map_kernel<64, true>), dim3(a.batch), dim3(64), adjoint_lds_bytes(a.nVar, a.cap), s, a, w_r, nullptr, d_x, w_f);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            d_x = nullptr;
            if (!d_v && !d_cost)
            {
                if (variant) *variant = "solve_rhs<64,single>";
                return hipSuccess;
            }
        }
        switch (place)
        {
        case TangentPlacement::staged:
            if ((e = set_lds(residual_rhs_kernel<64, 0>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((residual_rhs_kernel<64, 0>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_f, nrhs, d_x, d_v, d_cost, nullptr);
            break;
        case TangentPlacement::lds:
            if ((e = set_lds(residual_rhs_kernel<64, 1>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((residual_rhs_kernel<64, 1>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_f, nrhs, d_x, d_v, d_cost, nullptr);
            break;
        case TangentPlacement::work:
            if ((e = set_lds(residual_rhs_kernel<64, 2>, lds)) != hipSuccess) return e;
            hipLaunchKernelGGL((residual_rhs_kernel<64, 2>), dim3(a.batch, tiles), dim3(64), lds, s, a, w_r, w_f, nrhs, d_x, d_v, d_cost, w_state);
            break;
        }
        if (variant) *variant = residual_rhs_placement_name(place);
        return hipGetLastError();
    }
} // namespace lexls
