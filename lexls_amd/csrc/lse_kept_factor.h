// The kept factor of a LexLSE solve as the kernels behind it read it: the per-problem view, the rule for how far a level's stored rank may be
// trusted, the walk over the levels a kernel works on, and the wavefront-wide helpers that more than one of those kernels takes (lse_adjoint.hip:
// the adjoint family, whose steps on top of these are stated once in lse_kept_steps.h; lse_postfactor.hip: sensitivity_kernel stages the factor
// with stage_factor).  trusted_rank is plain C++ as well (tests/kept_factor_check.cpp runs the very same rule on the host).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LEXLS_KF_FN __host__ __device__ __forceinline__
#else
#define LEXLS_KF_FN inline
#endif
namespace lexls
{
    /// A level's rank as a kernel that walks the kept factor may trust it — THE ONLY STATEMENT OF THE RULE.  n variables, nf <= n of them fixed;
    /// T <= n = the total rank (pivot columns: [nf, T)); the level has dim rows, stored rank *rk, first column Fc.  0 when every variable is fixed
    /// (factorize() returns before the levels) or Fc >= T — *rk is not read then —; else *rk held inside the level's rows and the pivot columns
    constexpr LEXLS_KF_FN uint32_t trusted_rank(uint32_t n, uint32_t nf, uint32_t T, uint32_t dim, const uint32_t *rk, uint32_t Fc)
    {
        uint32_t rank = (nf < n && Fc < T) ? *rk : 0;
        if (rank > dim) rank = dim;
        if (rank > T - (Fc < T ? Fc : T)) rank = T - (Fc < T ? Fc : T);
        return rank;
    }
} // namespace lexls
#undef LEXLS_KF_FN

#if defined(__HIPCC__) // ---- device code from here on ----
#include "lexls_kernels.h"
#include "lqr_wave_common.h"

namespace lexls
{
    /// one problem's kept factor: W = cap x (nVar + 1), column-major (the right-hand side last), hh = the Householder scalars by row, the levels'
    /// rows / stored ranks / first columns, nf = the fixed variables and T = the total rank (both held to n), M = the problem's own rows (held to cap)
    struct KeptFactor
    {
        const double *__restrict__ W, *hh;
        const uint32_t *dims, *rk, *fc;
        uint32_t n, cap, nObj, nf, T, M;
        struct Level { uint32_t rank, Fc; };
        /// level k (of dim rows): its rank as the loops may trust it (trusted_rank) and its first column
        __device__ __forceinline__ Level level(uint32_t k, uint32_t dim) const { return {trusted_rank(n, nf, T, dim, rk + k, fc[k]), fc[k]}; }
        /// THE LEVEL WALK: body(k, dim, F, rank, Fc) for every level a kernel works on — rank > 0 and all of its rows F .. F + dim among the
        /// problem's own — first to last; body is an always-inlined callable (it may hold workgroup-uniform barriers: the walk is uniform).
        /// Returns the sum of all the levels' rows (not held to cap): where the walk from the last level starts
        template <class BODY>
        __device__ __forceinline__ uint32_t for_levels_ascending(const BODY &body) const
        {
            uint32_t F = 0;
            for (uint32_t k = 0; k < nObj; k++)
            {
                const uint32_t dim = dims[k];
                const Level lv     = level(k, dim);
                if (lv.rank > 0 && F + dim <= M) body(k, dim, F, lv.rank, lv.Fc);
                F += dim;
            }
            return F;
        }
        /// the same levels, last to first; Fend = the sum of all the levels' rows (for_levels_ascending's, or total_rows())
        __device__ __forceinline__ uint32_t total_rows() const
        {
            uint32_t Fend = 0;
            for (uint32_t k = 0; k < nObj; k++) Fend += dims[k];
            return Fend;
        }
        template <class BODY>
        __device__ __forceinline__ void for_levels_descending(uint32_t Fend, const BODY &body) const
        {
            for (uint32_t k = nObj; k--;)
            {
                const uint32_t dim = dims[k], F = Fend - dim;
                Fend               = F;
                const Level lv     = level(k, dim);
                if (lv.rank > 0 && F + dim <= M) body(k, dim, F, lv.rank, lv.Fc);
            }
        }
    };
    __device__ __forceinline__ KeptFactor kept_factor_of(const LseArgs &a, uint32_t b)
    {
        const uint32_t n = a.nVar, cap = a.cap, nObj = a.nObj;
        KeptFactor f{a.fac + (size_t)b * cap * (n + 1), a.hh + (size_t)b * cap, a.dims + (size_t)b * nObj, a.rank + (size_t)b * nObj, a.fcol + (size_t)b * nObj, n, cap, nObj, 0, 0, 0};
        f.nf = a.nfixed ? (a.nfixed[b] < n ? a.nfixed[b] : n) : 0;
        f.T  = a.totalrank[b] < n ? a.totalrank[b] : n; // pivot columns: [nf, T)
        for (uint32_t k = 0; k < nObj; k++) f.M += f.dims[k];
        if (f.M > f.cap) f.M = f.cap;
        return f;
    }
    /// the position variable i reaches by following the transpositions first to last (perm_l: the problem's, T of them count)
    __device__ __forceinline__ uint32_t position_after_transpositions(const uint32_t *perm_l, uint32_t T, uint32_t i)
    {
        uint32_t p = i;
        for (uint32_t k = 0; k < T; k++)
        {
            const uint32_t pk = perm_l[k];
            p                 = (p == k) ? pk : ((p == pk) ? k : p);
        }
        return p;
    }
    /// sum over the 64 lanes of a wavefront, the same bits in every lane and from run to run (xor butterfly: the two partners of a step
    /// add the same two values)
    __device__ __forceinline__ double wave_sum(double v)
    {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    }
    /// sum_{i < len} col[i] * vec[i], col in the stored factor (consecutive rows of ONE column: the lanes read consecutive addresses), vec in
    /// LDS; w0 = this lane's entry of the first 64 rows (0 beyond len), fetched by the caller ahead of the chain it sits on
    __device__ __forceinline__ double column_dot(const double *col, const double *vec, uint32_t len, double w0, uint32_t lane)
    {
        double p = lane < len ? w0 * vec[lane] : 0.0;
        for (uint32_t i = lane + 64; i < len; i += 64) p = dfma(col[i], vec[i], p);
        return wave_sum(p);
    }
    /// v <- H v for one stored reflector H = I - tau [1; ess] [1; ess]^T on the `rows` entries of the LDS vector v, one wavefront; e = this lane's
    /// entry of the first 64 rows of ess (0 beyond them).  None where factorize() made none (one row left, or tau == 0: uniform).  Two barriers
    __device__ __forceinline__ void apply_stored_reflector(const double *ess, double *v, uint32_t rows, double tau, double e, uint32_t lane)
    {
        if (rows == 1 || tau == 0.0) return;
        const double t = column_dot(ess, v + 1, rows - 1, e, lane) + v[0];
        __syncthreads(); // (every lane has read v[0])
        if (lane == 0) v[0] = dfma(-tau, t, v[0]);
        if (lane + 1 < rows) v[1 + lane] = dfma(-(tau * e), t, v[1 + lane]);
        for (uint32_t i = lane + 64; i + 1 < rows; i += 64) v[1 + i] = dfma(-(tau * ess[i]), t, v[1 + i]);
        __syncthreads();
    }
    /// One coalesced pass over a problem's stored factor (cap x (nVar+1), column-major) into LDS, odd leading dimension so that
    /// "thread = row" and "thread = column" walks are conflict-free.  For kernels that walk the factor along dependent chains
    /// when latency, not occupancy, is what counts (few problems per CU; several levels per launch).
    template <int NT>
    __device__ __forceinline__ void stage_factor(const double *__restrict__ G, double *L, uint32_t cap, uint32_t ncol, uint32_t ldl, uint32_t tid)
    {
        constexpr uint32_t U = NT <= 64 ? 20 : 8; // loads in flight per thread (one wavefront staging for itself: the rounds are latency, not bandwidth)
        const uint32_t total = cap * ncol;
        for (uint32_t base = tid; base < total; base += NT * U)
        {
            double v[U];
#pragma unroll
            for (uint32_t u = 0; u < U; u++)
            {
                const uint32_t e = base + u * NT;
                v[u]             = e < total ? G[e] : 0.0;
            }
#pragma unroll
            for (uint32_t u = 0; u < U; u++)
            {
                const uint32_t e = base + u * NT;
                if (e < total)
                {
                    const uint32_t j = e / cap;
                    L[(e - j * cap) + j * ldl] = v[u];
                }
            }
        }
        __syncthreads();
    }
} // namespace lexls
#endif
