// The steps of the kernels that walk a KEPT LexLSE factor (lse_adjoint.hip) — EACH STATED ONCE: a fixed dfma order per step, so that API
// entries documented as transposes of each other, and the forms of one entry, cannot drift apart.  Three families:
//   lane_*    LANE = VECTOR: the lane's own column of a state laid out [index][lane] with leading dimension LD (65 in LDS, 64 in a work
//             buffer); every sum is the lane's serial dfma chain, no cross-lane traffic, no barrier — a vector's bits do not depend on its
//             lane, its tile or its neighbours.  The factor comes through an accessor Wat(r, c) (staged in LDS or read where it is kept).
//             Consumers: solve_adjoint_multi_kernel, solve_adjoint_reg_multi_kernel, apply_solve_map_multi_kernel, apply_solve_map_reg_multi_kernel, residual_rhs_kernel
//   shared_*  work of the PROBLEM, the lanes of one wavefront spread over entries, barriers inside: the null-space basis and the damped
//             normal matrix of a regularized factor.  Consumers: solve_adjoint_reg_kernel, solve_adjoint_reg_multi_kernel,
//             apply_solve_map_reg_multi_kernel
//   wave_*    ONE VECTOR PER WAVEFRONT, the lanes along the rows of one factor column, wavefront sums (column_dot, apply_stored_reflector:
//             lse_kept_factor.h), columns AU at a time.  Consumers: solve_adjoint_kernel, solve_adjoint_reg_kernel
// and the regularized problem's view (RegularizedLevels) beside KeptFactor.  Everything is inlined into its kernel.
#pragma once
#include "lse_kept_factor.h"

#if defined(__HIPCC__)
namespace lexls
{
    /// what a kernel on the factor of a REGULARIZED factorize() (type 1, 3, 4, 5, 8 or 9, a constant factor per level) reads of the regularization
    struct RegularizedLevels
    {
        uint32_t type;
        bool accum, wideW; // the types that accumulate the null-space basis NS (and read it); W = [R | T] (else R)
        const double *fac; // the problem's factor per level
        /// the gate of regularize_level: the level is damped at all
        __device__ __forceinline__ static bool acts(double f) { return !(fabs(f - 0.0) < 1e-15); }
        /// the columns of W at a level of `rank` pivots from column Fc on: the order of the level's D
        __device__ __forceinline__ uint32_t width(uint32_t n, uint32_t Fc, uint32_t rank) const { return wideW ? n - Fc : rank; }
    };
    __device__ __forceinline__ RegularizedLevels regularized_levels_of(const LseArgs &a, uint32_t b)
    {
        const uint32_t type = a.reg_type;
        return {type, type == 1 || type == 3 || type == 8, type == 1 || type == 5 || type == 8, a.reg_factor + (size_t)b * a.nObj};
    }

    // ---- lane = vector ----
    /// the tile's kt vectors (rows of n doubles, contiguous at Gt) into the state by position: gh[pos_l[i]][c] = Gt[c][i]
    template <int NT, uint32_t LD>
    __device__ __forceinline__ void lane_gather_by_position(const double *__restrict__ Gt, const uint32_t *pos_l, double *gh, uint32_t kt, uint32_t n, uint32_t lane)
    {
        for (uint32_t e = lane; e < kt * n; e += NT)
        {
            const uint32_t c = e / n, i = e - c * n, p = pos_l[i];
            if (p < n) gh[p * LD + c] = Gt[e];
        }
    }
    /// the tile's kt right-hand sides (rows of cap doubles, contiguous from R + off) into the state: t[r][c] = R[c][r] on the problem's own
    /// rows, minus Y[c][r] on rows [lo, hi) (Y is not read where lo == hi)
    template <int NT, uint32_t LD>
    __device__ __forceinline__ void lane_load_rhs(const double *__restrict__ R, const double *__restrict__ Y, size_t off, uint32_t lo, uint32_t hi, double *t, uint32_t kt,
                                                  uint32_t cap, uint32_t M, uint32_t lane)
    {
        for (uint32_t e = lane; e < kt * cap; e += NT)
        {
            const uint32_t c = e / cap, r = e - c * cap;
            if (r < M) t[r * LD + c] = (r >= lo && r < hi) ? R[off + e] - Y[off + e] : R[off + e];
        }
    }
    /// v <- H v for the stored reflector of factor column `col` whose unit entry sits in row r0 = the row of v[0], on `rows` entries of the
    /// lane's column (a serial chain per lane, no barrier — not apply_stored_reflector's shape).  None where factorize() made none (uniform)
    template <uint32_t LD, class WAT>
    __device__ __forceinline__ void lane_stored_reflector(const WAT &Wat, double tau, double *v, uint32_t r0, uint32_t col, uint32_t rows)
    {
        if (rows == 1 || tau == 0.0) return;
        double t = 0.0;
        for (uint32_t i = 1; i < rows; i++) t = dfma(Wat(r0 + i, col), v[i * LD], t);
        t += v[0];
        v[0] = dfma(-tau, t, v[0]);
        for (uint32_t i = 1; i < rows; i++) v[i * LD] = dfma(-(tau * Wat(r0 + i, col)), t, v[i * LD]);
    }
    /// the level's reflectors on rows F + j .. F + dim - 1 of the lane's column v, first to last (factorize()'s order) / last to first (its
    /// reverse).  (forward, unroll 1: a reflector starts where the one before it ends, so two at a time gain nothing, and the unroller's
    /// form of this loop triples its code)
    template <uint32_t LD, class WAT, class TAU>
    __device__ __forceinline__ void lane_reflectors_forward(const WAT &Wat, const TAU &tau_at, double *vl, uint32_t F, uint32_t Fc, uint32_t dim, uint32_t rank)
    {
#pragma unroll 1
        for (uint32_t j = 0; j < rank; j++) lane_stored_reflector<LD>(Wat, tau_at(F + j), vl + (F + j) * LD, F + j, Fc + j, dim - j);
    }
    template <uint32_t LD, class WAT, class TAU>
    __device__ __forceinline__ void lane_reflectors_reversed(const WAT &Wat, const TAU &tau_at, double *vl, uint32_t F, uint32_t Fc, uint32_t dim, uint32_t rank)
    {
        for (uint32_t j = rank; j--;) lane_stored_reflector<LD>(Wat, tau_at(F + j), vl + (F + j) * LD, F + j, Fc + j, dim - j);
    }
    /// step (b) at one level, the reverse of solve(): y = R^-T gh on the level's pivot columns, written into cb rows F .. F + rank, then
    /// gh -= T^T y on the pivot columns of the later levels
    template <uint32_t LD, class WAT>
    __device__ __forceinline__ void lane_reverse_solve_level(const WAT &Wat, double *ghl, double *cbl, uint32_t F, uint32_t Fc, uint32_t rank, uint32_t T)
    {
        double *y = cbl + F * LD;
        for (uint32_t c = Fc; c < T; c++)
        {
            const uint32_t j = c - Fc, len = j < rank ? j : rank;
            double s = 0.0;
            for (uint32_t i = 0; i < len; i++) s = dfma(Wat(F + i, c), y[i * LD], s);
            if (j < rank) // (uniform) inside the triangle
                y[j * LD] = (ghl[c * LD] - s) / Wat(F + j, c);
            else
                ghl[c * LD] -= s;
        }
    }
    /// the transposed Gauss step: cb[F + p] -= (multiplier column Fc + p, rows Fn .. M)^T cb.  AU multiplier columns share one read of the
    /// lane's cb rows (each sum in ascending row order)
    template <uint32_t LD, class WAT>
    __device__ __forceinline__ void lane_gauss_transposed(const WAT &Wat, double *cbl, uint32_t F, uint32_t Fn, uint32_t M, uint32_t Fc, uint32_t rank)
    {
        constexpr uint32_t AU = 4;
        for (uint32_t p0 = 0; p0 < rank; p0 += AU)
        {
            double s[AU];
#pragma unroll
            for (uint32_t u = 0; u < AU; u++) s[u] = 0.0;
            for (uint32_t i = Fn; i < M; i++)
            {
                const double ci = cbl[i * LD];
#pragma unroll
                for (uint32_t u = 0; u < AU; u++)
                    if (p0 + u < rank) s[u] = dfma(Wat(i, Fc + p0 + u), ci, s[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
                if (p0 + u < rank) cbl[(F + p0 + u) * LD] -= s[u];
        }
    }
    /// the Gauss step: t[i] -= sum_p (multiplier of row i, column Fc + p) t[F + p] on rows Fn .. M.  AU rows of the later levels share one
    /// read of the level's top (each chain in ascending column order)
    template <uint32_t LD, class WAT>
    __device__ __forceinline__ void lane_gauss(const WAT &Wat, double *tl, uint32_t F, uint32_t Fn, uint32_t M, uint32_t Fc, uint32_t rank)
    {
        constexpr uint32_t AU = 4;
        for (uint32_t i0 = Fn; i0 < M; i0 += AU)
        {
            double acc[AU];
#pragma unroll
            for (uint32_t u = 0; u < AU; u++) acc[u] = i0 + u < M ? tl[(i0 + u) * LD] : 0.0;
            for (uint32_t p = 0; p < rank; p++)
            {
                const double tp = tl[(F + p) * LD];
#pragma unroll
                for (uint32_t u = 0; u < AU; u++)
                    if (i0 + u < M) acc[u] = dfma(-Wat(i0 + u, Fc + p), tp, acc[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
                if (i0 + u < M) tl[(i0 + u) * LD] = acc[u];
        }
    }
    /// step (b)^T at one level, solve(): the top of the level minus T z on the pivot columns of the later levels (descending column order,
    /// as apply_solve_map_kernel), then the triangle, last column first: z_c = t_c / R_cc, t[rows above] -= W[rows, c] z_c
    template <uint32_t LD, class WAT>
    __device__ __forceinline__ void lane_back_substitute_level(const WAT &Wat, double *tl, double *zl, uint32_t F, uint32_t Fc, uint32_t rank, uint32_t T)
    {
        constexpr uint32_t AU = 4;
        for (uint32_t i0 = 0; i0 < rank; i0 += AU)
        {
            double acc[AU];
#pragma unroll
            for (uint32_t u = 0; u < AU; u++) acc[u] = i0 + u < rank ? tl[(F + i0 + u) * LD] : 0.0;
            for (uint32_t c = T; c > Fc + rank; c--)
            {
                const double zc = zl[(c - 1) * LD];
#pragma unroll
                for (uint32_t u = 0; u < AU; u++)
                    if (i0 + u < rank) acc[u] = dfma(-Wat(F + i0 + u, c - 1), zc, acc[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
                if (i0 + u < rank) tl[(F + i0 + u) * LD] = acc[u];
        }
        for (uint32_t j = rank; j--;)
        {
            const double zc   = tl[(F + j) * LD] / Wat(F + j, Fc + j);
            zl[(Fc + j) * LD] = zc;
            for (uint32_t i = 0; i < j; i++) tl[(F + i) * LD] = dfma(-Wat(F + i, Fc + j), zc, tl[(F + i) * LD]);
        }
    }
    /// get_v() at one level on the lane's column, in place: v = Q_k [0 ; -tail], where tl rows F .. F + dim hold the level's right-hand side as
    /// the forward pass left it (reflectors, then the Gauss steps of the levels above): the tail, rows rank .. dim - 1, is written by no later
    /// step — a Gauss step writes the rows of the levels BEHIND its own, the back-substitution the first `rank` rows of its own.  Returns the
    /// level's cost, the sum of squares of its rows of v as one fma chain in row order.  rank == dim (uniform): nothing goes through Q, exact zeros
    template <uint32_t LD, class WAT, class TAU>
    __device__ __forceinline__ double lane_level_residual(const WAT &Wat, const TAU &tau_at, double *tl, uint32_t F, uint32_t Fc, uint32_t dim, uint32_t rank)
    {
        double *v = tl + F * LD;
        for (uint32_t i = 0; i < rank; i++) v[i * LD] = 0.0;
        if (rank >= dim) return 0.0;
        for (uint32_t i = rank; i < dim; i++) v[i * LD] = -v[i * LD];
        lane_reflectors_reversed<LD>(Wat, tau_at, tl, F, Fc, dim, rank);
        double cost = 0.0;
        for (uint32_t i = 0; i < dim; i++) cost = dfma(v[i * LD], v[i * LD], cost);
        return cost;
    }
    /// entry c of W^T y for the level's W (column c has min(c + 1, rank) rows), y = yb[0, rank)
    template <uint32_t LD, class WAT>
    __device__ __forceinline__ double lane_wt_y(const WAT &Wat, const double *yb, uint32_t F, uint32_t Fc, uint32_t rank, uint32_t c)
    {
        const uint32_t len = c < rank ? c + 1 : rank;
        double acc = 0.0;
        for (uint32_t r = 0; r < len; r++) acc = dfma(Wat(F + r, Fc + c), yb[r * LD], acc);
        return acc;
    }
    /// L z = d, then L^T t = z, in place on the lane's dv[0, N) against the factor spd_factor left in D (shared by the lanes), row by row: entry
    /// i receives the products j = 0 .. i-1, backwards j = N-1 .. i+1 — the order of spd_solve's column sweeps (lse_spd_solve.h)
    template <uint32_t LD>
    __device__ __forceinline__ void lane_spd_substitute(const double *D, uint32_t ldd, double *dvl, uint32_t N)
    {
        for (uint32_t i = 0; i < N; i++)
        {
            double acc = dvl[i * LD];
            for (uint32_t j = 0; j < i; j++) acc = dfma(-D[i + (size_t)j * ldd], dvl[j * LD], acc);
            dvl[i * LD] = acc / D[i + (size_t)i * ldd];
        }
        for (uint32_t i = N; i--;)
        {
            double acc = dvl[i * LD];
            for (uint32_t j = N - 1; j > i; j--) acc = dfma(-D[j + (size_t)i * ldd], dvl[j * LD], acc);
            dvl[i * LD] = acc / D[i + (size_t)i * ldd];
        }
    }
    /// yb[0, rank) = W dv[0, N)
    template <uint32_t LD, class WAT>
    __device__ __forceinline__ void lane_w_t(const WAT &Wat, double *yb, const double *dvl, uint32_t F, uint32_t Fc, uint32_t rank, uint32_t N)
    {
        for (uint32_t i = 0; i < rank; i++)
        {
            double acc = 0.0;
            for (uint32_t c = i; c < N; c++) acc = dfma(Wat(F + i, Fc + c), dvl[c * LD], acc);
            yb[i * LD] = acc;
        }
    }
    /// step (d): grad_fixed_j = gh_j - (column j of the fixed variables)^T cb, left in gh_j; then both outputs (grad_fixed may be NULL), the
    /// tile's kt rows from row0 on, transposed through the state: consecutive lanes take consecutive addresses
    template <int NT, uint32_t LD, class WAT>
    __device__ __forceinline__ void lane_step_d(const WAT &Wat, double *gh, double *cb, double *__restrict__ grad_rhs, double *__restrict__ grad_fixed, size_t row0, uint32_t kt,
                                                uint32_t n, uint32_t cap, uint32_t nf, uint32_t M, uint32_t lane)
    {
        double *ghl = gh + lane, *cbl = cb + lane;
        if (grad_fixed)
            for (uint32_t j = 0; j < nf; j++)
            {
                double s = 0.0;
                for (uint32_t r = 0; r < M; r++) s = dfma(Wat(r, j), cbl[r * LD], s);
                ghl[j * LD] -= s;
            }
        __syncthreads();
        {
            double *out = grad_rhs + row0 * cap;
            for (uint32_t e = lane; e < kt * cap; e += NT)
            {
                const uint32_t c = e / cap, r = e - c * cap;
                out[e]           = cb[r * LD + c]; // (rows behind the problem's own were never touched: 0)
            }
        }
        if (grad_fixed)
        {
            double *out = grad_fixed + row0 * n;
            for (uint32_t e = lane; e < kt * n; e += NT)
            {
                const uint32_t c = e / n, j = e - c * n;
                out[e]           = j < nf ? gh[j * LD + c] : 0.0;
            }
        }
    }

    // ---- work of the problem ----
    /// one level's step of the null-space basis NS (n x n, column-major; reg_accumulate_nullspace without the right-hand-side column, A side
    /// only, the factor's FINAL column order): the identity block, the columns left of it times R^-1, the trailing columns minus those
    /// times T.  Ends in a barrier
    template <int NT, class WAT>
    __device__ __forceinline__ void shared_nullspace_level(const WAT &w, double *NS, uint32_t n, uint32_t F, uint32_t Fc, uint32_t m0, uint32_t rank, uint32_t lane)
    {
        auto ns = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double & { return NS[i + (size_t)j * n]; };
        const uint32_t rows = m0 + rank, RC = n - Fc - rank;
        for (uint32_t e = lane; e < rank * rank; e += NT) ns(m0 + e % rank, Fc + e / rank) = (e % rank == e / rank) ? 1.0 : 0.0;
        __syncthreads();
        for (uint32_t i = lane; i < rows; i += NT) // Left <- Left R^-1, a row per lane
            for (uint32_t p = 0; p < rank; p++)
            {
                double sv = ns(i, Fc + p);
                for (uint32_t q = 0; q < p; q++) sv = dfma(-ns(i, Fc + q), w(F + q, Fc + p), sv);
                ns(i, Fc + p) = sv / w(F + p, Fc + p);
            }
        __syncthreads();
        for (uint32_t e = lane; e < rows * RC; e += NT) // Trailing -= Left T
        {
            const uint32_t i = e % rows, c = Fc + rank + e / rows;
            double t = ns(i, c);
            for (uint32_t p = 0; p < rank; p++) t = dfma(-ns(i, Fc + p), w(F + p, c), t);
            ns(i, c) = t;
        }
        __syncthreads();
    }
    /// the rebuild of NS from the factor, levels ascending, for a kernel that walks the levels DESCENDING afterwards: U = the rows [0, m0) of
    /// NS above the level's N columns at entry to the level is kept in SN first (m0 x N, leading dimension m0, a level behind the other).
    /// Returns the doubles of SN in use
    template <int NT, class WAT>
    __device__ __forceinline__ uint32_t shared_rebuild_nullspace(const KeptFactor &kf, const RegularizedLevels &reg, const WAT &w, double *NS, double *SN, uint32_t lane)
    {
        uint32_t soff = 0;
        kf.for_levels_ascending([&](uint32_t, uint32_t, uint32_t F, uint32_t rank, uint32_t Fc) __attribute__((always_inline)) {
            const uint32_t m0 = Fc > kf.nf ? Fc - kf.nf : 0, wc = reg.width(kf.n, Fc, rank);
            for (uint32_t e = lane; e < m0 * wc; e += NT) SN[soff + e] = NS[e % m0 + (size_t)(Fc + e / m0) * kf.n];
            soff += m0 * wc;
            shared_nullspace_level<NT>(w, NS, kf.n, F, Fc, m0, rank, lane);
        });
        return soff;
    }
    /// D = W^T W + mu U^T U + mu I, the lower triangle (order N, leading dimension n): the normal matrix of the level's damped problem.  Column
    /// c of W has min(c + 1, rank) rows; U (m0 x N, leading dimension ldu; read only where accum) = the rows of the null-space basis above the
    /// level's columns at entry to the level — a snapshot (SN + soff, m0) or the basis in place (NS + Fc n, n).  No barrier
    template <int NT, class WAT>
    __device__ __forceinline__ void shared_damped_normal_matrix(const WAT &w, const double *U, uint32_t ldu, bool accum, double mu, double *D, uint32_t n, uint32_t F, uint32_t Fc,
                                                                uint32_t rank, uint32_t N, uint32_t m0, uint32_t lane)
    {
        for (uint32_t e = lane; e < N * N; e += NT)
        {
            const uint32_t i = e % N, j = e / N;
            if (i < j) continue;
            const uint32_t len = j < rank ? j + 1 : rank;
            double acc = 0.0;
            for (uint32_t r = 0; r < len; r++) acc = dfma(w(F + r, Fc + i), w(F + r, Fc + j), acc);
            if (accum)
            {
                double up = 0.0;
                for (uint32_t s = 0; s < m0; s++) up = dfma(U[s + (size_t)i * ldu], U[s + (size_t)j * ldu], up);
                acc = dfma(mu, up, acc);
            }
            D[i + (size_t)j * n] = i == j ? acc + mu : acc;
        }
    }

    // ---- one vector per wavefront ----
    constexpr uint32_t kWaveAU = 4; // factor columns whose first 64 rows are requested together, ahead of the (dependent) steps that consume them
    /// step (a): gh = P^T g — variable i sits at the position it reaches by following the transpositions first to last — and cb = 0
    template <int NT>
    __device__ __forceinline__ void wave_step_a(const uint32_t *__restrict__ perm, const double *__restrict__ g, uint32_t *perm_l, double *gh, double *cb, uint32_t n,
                                                uint32_t cap, uint32_t T, uint32_t lane)
    {
        for (uint32_t i = lane; i < n; i += NT) perm_l[i] = perm[i];
        for (uint32_t i = lane; i < cap; i += NT) cb[i] = 0.0;
        __syncthreads();
        for (uint32_t i = lane; i < n; i += NT)
        {
            const uint32_t p = position_after_transpositions(perm_l, T, i);
            if (p < n) gh[p] = g[i];
        }
        __syncthreads();
    }
    /// step (b) at one level, the reverse of solve(): y = R_k^-T gh_k (into cb rows F .. F + rank), then gh -= [T_k]^T y on the pivot
    /// columns of the later levels.  Column c of [R_k | T_k] takes the dot product of its rows above the diagonal (all `rank` rows behind the
    /// triangle) with y.  Ends in a barrier
    template <int NT>
    __device__ __forceinline__ void wave_reverse_solve_level(const double *__restrict__ W, uint32_t cap, double *gh, double *cb, uint32_t F, uint32_t Fc, uint32_t rank,
                                                             uint32_t T, uint32_t lane)
    {
        constexpr uint32_t AU = kWaveAU;
        double *y = cb + F;
        for (uint32_t c0 = Fc; c0 < T; c0 += AU)
        {
            double w[AU], dg[AU];
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
            {
                const uint32_t c = c0 + u, j = c - Fc;
                const uint32_t len = c < T ? (j < rank ? j : rank) : 0;
                w[u]  = lane < len ? W[F + lane + (size_t)c * cap] : 0.0;
                dg[u] = (c < T && j < rank) ? W[F + j + (size_t)c * cap] : 1.0;
            }
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
            {
                const uint32_t c = c0 + u, j = c - Fc;
                if (c >= T) break;
                const uint32_t len = j < rank ? j : rank;
                const double s     = column_dot(W + F + (size_t)c * cap, y, len, w[u], lane);
                if (j < rank) // (uniform) inside the triangle: the next column reads this y
                {
                    if (lane == 0) y[j] = (gh[c] - s) / dg[u];
                    __syncthreads();
                }
                else if (lane == 0)
                    gh[c] -= s;
            }
        }
        __syncthreads();
    }
    /// the transposed Gauss step (the multipliers L sit in the level's pivot columns, rows Fn .. M of the later levels).  Ends in a barrier
    template <int NT>
    __device__ __forceinline__ void wave_gauss_transposed(const double *__restrict__ W, uint32_t cap, double *cb, uint32_t F, uint32_t Fn, uint32_t M, uint32_t Fc,
                                                          uint32_t rank, uint32_t lane)
    {
        constexpr uint32_t AU = kWaveAU;
        for (uint32_t p0 = 0; p0 < rank; p0 += AU)
        {
            double w[AU], s[AU];
#pragma unroll
            for (uint32_t u = 0; u < AU; u++) w[u] = (p0 + u < rank && lane < M - Fn) ? W[Fn + lane + (size_t)(Fc + p0 + u) * cap] : 0.0;
#pragma unroll
            for (uint32_t u = 0; u < AU; u++) s[u] = p0 + u < rank ? column_dot(W + Fn + (size_t)(Fc + p0 + u) * cap, cb + Fn, M - Fn, w[u], lane) : 0.0;
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
                if (lane == 0 && p0 + u < rank) cb[F + p0 + u] -= s[u];
        }
        __syncthreads();
    }
    /// the level's reflectors on rows F + j .. F + dim - 1 of cb, last first, AU at a time: their scalars and first 64 rows are requested together
    template <int NT>
    __device__ __forceinline__ void wave_reflectors_reversed(const double *__restrict__ W, const double *hh, uint32_t cap, double *cb, uint32_t F, uint32_t Fc, uint32_t dim,
                                                             uint32_t rank, uint32_t lane)
    {
        constexpr uint32_t AU = kWaveAU;
        for (uint32_t j0 = rank; j0 > 0; j0 -= (j0 < AU ? j0 : AU))
        {
            double e[AU], tau[AU];
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
            {
                const bool on = u < j0;
                const uint32_t j = on ? j0 - 1 - u : 0;
                tau[u] = on ? hh[F + j] : 0.0;
                e[u]   = (on && lane + 1 < dim - j) ? W[F + j + 1 + lane + (size_t)(Fc + j) * cap] : 0.0;
            }
#pragma unroll
            for (uint32_t u = 0; u < AU; u++)
            {
                if (u >= j0) break;
                const uint32_t j = j0 - 1 - u;
                apply_stored_reflector(W + F + j + 1 + (size_t)(Fc + j) * cap, cb + F + j, dim - j, tau[u], e[u], lane);
            }
        }
    }
    /// step (d): grad_rhs = cb (rows behind the problem's own stay 0); grad_fixed_j = gh_j - (column j of the fixed variables)^T cb, zero
    /// behind the fixed variables (grad_fixed may be NULL).  Rows b of both outputs
    template <int NT>
    __device__ __forceinline__ void wave_step_d(const double *__restrict__ W, const double *gh, const double *cb, double *__restrict__ grad_rhs, double *__restrict__ grad_fixed,
                                                uint32_t b, uint32_t n, uint32_t cap, uint32_t nf, uint32_t M, uint32_t lane)
    {
        constexpr uint32_t AU = kWaveAU;
        for (uint32_t i = lane; i < cap; i += NT) grad_rhs[(size_t)b * cap + i] = cb[i];
        if (grad_fixed)
        {
            for (uint32_t j0 = 0; j0 < nf; j0 += AU)
            {
                double w[AU], s[AU];
#pragma unroll
                for (uint32_t u = 0; u < AU; u++) w[u] = (j0 + u < nf && lane < M) ? W[lane + (size_t)(j0 + u) * cap] : 0.0;
#pragma unroll
                for (uint32_t u = 0; u < AU; u++) s[u] = j0 + u < nf ? column_dot(W + (size_t)(j0 + u) * cap, cb, M, w[u], lane) : 0.0;
#pragma unroll
                for (uint32_t u = 0; u < AU; u++)
                    if (lane == 0 && j0 + u < nf) grad_fixed[(size_t)b * n + j0 + u] = gh[j0 + u] - s[u];
            }
            for (uint32_t j = nf + lane; j < n; j += NT) grad_fixed[(size_t)b * n + j] = 0.0;
        }
    }
} // namespace lexls
#endif
