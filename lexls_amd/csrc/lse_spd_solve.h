// The dense symmetric positive-definite solve of the LexLSE device code — THE ONLY IMPLEMENTATION: LL^T of a lower triangle in place, then
// L y = d, then L^T z = y in place (oracle: cholesky_solve).  Its consumers: the regularization family (lexls_regularize.h), the adjoint of
// regularized solves (solve_adjoint_reg_kernel, lse_adjoint.hip), solveLeastNorm_2 and _3 (lse_postfactor.hip); spd_factor<NT> is the
// factorization alone, for the lane = vector kernels on regularized factors (solve_adjoint_reg_multi_kernel, apply_solve_map_reg_multi_kernel),
// which substitute per lane in the same order (lane_spd_substitute, lse_kept_steps.h).  Two forms behind one entry, spd_solve<NT>; both do the same
// operations on the same operands in the same order (entry (i, j) receives the products k = 0 .. j-1 in that order; the substitutions go
// column by column), so the results are the same bits whichever form runs.
#pragma once
#include "lqr_wave_common.h"

namespace lexls
{
    namespace
    {
        /// The form for ONE wavefront, N <= 64: lane i owns row i of the lower triangle and d_i.
        /// Panels of 16 columns at a time in registers; a finished column's entries reach the other lanes by v_readlane, the columns of
        /// earlier panels come back from the work matrix as the lane's OWN row (no lane reads what another lane wrote until the backward
        /// substitution) — so the 3 N dependent steps (square root / division each) cost their arithmetic, not a memory round trip plus a loop
        /// of unknown trip count each, which is where the routine's time went.  The panel loops have run-time trip counts and a fixed body:
        /// about 70 registers where it is inlined (the out-of-line call below is allocated about 150), a few KB of code.
        /// the factorization half: on return lane i has written row i of L over row i of the lower triangle (no barrier: the lanes have read
        /// and written their OWN rows only)
        __device__ __forceinline__ void spd_factor_wave(double *D, uint32_t ldd, uint32_t N, uint32_t lane)
        {
            auto dd = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double & { return D[i + (size_t)j * ldd]; };
            constexpr int PB = 16;
            const bool on    = lane < N;
            double row[PB];
            for (uint32_t c0 = 0; c0 < N; c0 += PB)
            {
#pragma unroll
                for (int jj = 0; jj < PB; jj++) row[jj] = (on && c0 + jj <= lane && c0 + jj < N) ? dd(lane, c0 + jj) : 0.0;
                for (uint32_t k = 0; k < c0; k++) // the columns of the panels before: own entry from the matrix, the panel rows' entries from their lanes
                {
                    const double lik = (on && lane >= c0) ? dd(lane, k) : 0.0;
#pragma unroll
                    for (int jj = 0; jj < PB; jj++) row[jj] = dfma(-lik, rdlane(lik, (int)(c0 + jj) & 63), row[jj]);
                }
#pragma unroll
                for (int kk = 0; kk < PB; kk++)
                    if (c0 + kk < N) // uniform
                    {
                        const double lkk = sqrt(rdlane(row[kk], (int)(c0 + kk)));
                        const double lik = (lane == c0 + kk) ? lkk : row[kk] / lkk; // (zeros above the diagonal and beyond N)
                        row[kk]          = lik;
#pragma unroll
                        for (int jj = kk + 1; jj < PB; jj++) row[jj] = dfma(-lik, rdlane(lik, (int)(c0 + jj) & 63), row[jj]);
                    }
#pragma unroll
                for (int jj = 0; jj < PB; jj++)
                    if (on && c0 + jj <= lane && c0 + jj < N) dd(lane, c0 + jj) = row[jj];
            }
        }
        /// factorization, then the two substitutions with d_i in lane i's register
        __device__ __forceinline__ void spd_solve_wave(double *D, uint32_t ldd, double *d, uint32_t N, uint32_t lane)
        {
            auto dd = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double & { return D[i + (size_t)j * ldd]; };
            constexpr int PB = 16;
            const bool on    = lane < N;
            double row[PB];
            spd_factor_wave(D, ldd, N, lane);
            double di = on ? d[lane] : 0.0;
            for (uint32_t c0 = 0; c0 < N; c0 += PB)
            {
#pragma unroll
                for (int jj = 0; jj < PB; jj++) row[jj] = (on && c0 + jj <= lane && c0 + jj < N) ? dd(lane, c0 + jj) : 0.0;
#pragma unroll
                for (int jj = 0; jj < PB; jj++)
                    if (c0 + jj < N)
                    {
                        const uint32_t j = c0 + jj;
                        const double yj  = rdlane(di, (int)j) / rdlane(row[jj], (int)j);
                        di               = (lane == j) ? yj : (lane > j ? dfma(-row[jj], yj, di) : di);
                    }
            }
            __syncthreads(); // the factor's columns are read across lanes from here on
            for (uint32_t c0 = ((N - 1) / PB) * PB; N > 0; c0 -= PB)
            {
#pragma unroll
                for (int jj = 0; jj < PB; jj++) row[jj] = (on && c0 + jj >= lane && c0 + jj < N) ? dd(c0 + jj, lane) : 0.0;
#pragma unroll
                for (int jj = PB - 1; jj >= 0; jj--)
                    if (c0 + jj < N)
                    {
                        const uint32_t j = c0 + jj;
                        const double zj  = rdlane(di, (int)j) / rdlane(row[jj], (int)j);
                        di               = (lane == j) ? zj : (lane < j ? dfma(-row[jj], zj, di) : di);
                    }
                if (c0 == 0) break;
            }
            if (on) d[lane] = di;
            __syncthreads();
        }
        /// the same body as a call: for the register-resident kernels, which run it once per level and pay for every inlined copy in code size
        __device__ __noinline__ void spd_solve_wave_call(double *D, uint32_t ldd, double *d, uint32_t N, uint32_t lane) { spd_solve_wave(D, ldd, d, N, lane); }

        /// the factorization half of the column-by-column form (any NT, any N): left-looking; for N > 0 the last statement is a barrier
        template <int NT>
        __device__ __forceinline__ void spd_factor_columns(double *D, uint32_t ldd, uint32_t N, uint32_t tid)
        {
            auto dd = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double & { return D[i + (size_t)j * ldd]; };
            for (uint32_t j = 0; j < N; j++)
            {
                if (tid == 0)
                {
                    double sjj = dd(j, j);
                    for (uint32_t k = 0; k < j; k++) sjj = dfma(-dd(j, k), dd(j, k), sjj);
                    dd(j, j) = sqrt(sjj);
                }
                __syncthreads();
                const double ljj = dd(j, j);
                for (uint32_t i = j + 1 + tid; i < N; i += NT)
                {
                    double t = dd(i, j);
                    for (uint32_t k = 0; k < j; k++) t = dfma(-dd(i, k), dd(j, k), t);
                    dd(i, j) = t / ljj;
                }
                __syncthreads();
            }
        }

        /// THE FACTORIZATION ALONE, for a consumer that substitutes for itself (lane_spd_substitute, lse_kept_steps.h: one substitution pair per
        /// lane against the shared factor): LL^T of the lower triangle of D in place — the very operations spd_solve<NT> does before its substitutions,
        /// in either form — and a barrier behind it (workgroup-uniform; the last statement for N > 0): every thread may then read all of L
        template <int NT>
        __device__ __forceinline__ void spd_factor(double *D, uint32_t ldd, uint32_t N, uint32_t tid)
        {
            if constexpr (NT == 64)
            {
                if (N <= 64)
                {
                    spd_factor_wave(D, ldd, N, tid);
                    __syncthreads();
                    return;
                }
            }
            spd_factor_columns<NT>(D, ldd, N, tid);
        }

        /// LL^T of the lower triangle of D (order N, column-major, leading dimension ldd) in place, then D z = d in place, by a workgroup of NT
        /// threads; every barrier is workgroup-uniform, and for N > 0 the last statement is one.  NT == 64 and N <= 64: the one-wavefront panel
        /// form (WAVE_AS_CALL: out of line); else column by column
        template <int NT, bool WAVE_AS_CALL = false>
        __device__ __forceinline__ void spd_solve(double *D, uint32_t ldd, double *d, uint32_t N, uint32_t tid)
        {
            if constexpr (NT == 64)
            {
                if (N <= 64) return WAVE_AS_CALL ? spd_solve_wave_call(D, ldd, d, N, tid) : spd_solve_wave(D, ldd, d, N, tid);
            }
            auto dd = [&](uint32_t i, uint32_t j) __attribute__((always_inline)) -> double & { return D[i + (size_t)j * ldd]; };
            spd_factor_columns<NT>(D, ldd, N, tid);
            for (uint32_t j = 0; j < N; j++) // L y = d
            {
                if (tid == 0) d[j] = d[j] / dd(j, j);
                __syncthreads();
                const double yj = d[j];
                for (uint32_t i = j + 1 + tid; i < N; i += NT) d[i] = dfma(-dd(i, j), yj, d[i]);
                __syncthreads();
            }
            for (uint32_t j = N; j--;) // L^T z = y
            {
                if (tid == 0) d[j] = d[j] / dd(j, j);
                __syncthreads();
                const double zj = d[j];
                for (uint32_t i = tid; i < j; i += NT) d[i] = dfma(-dd(j, i), zj, d[i]);
                __syncthreads();
            }
        }
    } // namespace
} // namespace lexls
