// Steps of the generic kernels that more than one translation unit takes: the ordered dot product of lqr_generic.hip's factorization and of
// the kernels behind a kept factor (lse_postfactor.hip), the Householder sequence of a level on a vector, and x = P x by following the
// transpositions.  Arithmetic order as oracle/lexlse_oracle.h.
#pragma once
#include "lexls_kernels.h"
#include "lqr_wave_common.h"

namespace lexls
{
    namespace
    {
        /// s = fma(a_i, b_i, s) for i ascending, reads batched and prefetched as in chain_square
        template <int U>
        __device__ __forceinline__ double chain_dot(const double *a, const double *b, uint32_t len, double s)
        {
            uint32_t i = 0;
            if (len >= (uint32_t)U)
            {
                double x0[U], y0[U], x1[U], y1[U];
#pragma unroll
                for (int u = 0; u < U; u++)
                {
                    x0[u] = a[u];
                    y0[u] = b[u];
                }
                i = U;
                while (true)
                {
                    const bool more1 = i + U <= len;
                    if (more1)
                    {
#pragma unroll
                        for (int u = 0; u < U; u++)
                        {
                            x1[u] = a[i + u];
                            y1[u] = b[i + u];
                        }
                        i += U;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) s = dfma(x0[u], y0[u], s);
                    if (!more1) break;
                    const bool more0 = i + U <= len;
                    if (more0)
                    {
#pragma unroll
                        for (int u = 0; u < U; u++)
                        {
                            x0[u] = a[i + u];
                            y0[u] = b[i + u];
                        }
                        i += U;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) s = dfma(x1[u], y1[u], s);
                    if (!more0) break;
                }
            }
            for (; i < len; i++) s = dfma(a[i], b[i], s);
            return s;
        }

        /// v <- Q_k v (Householder sequence H_0 ... H_{r-1}, last reflector first; lexlse.h:1576-1578).
        /// v points at the level's first entry (LDS); W is the factor.  Block-wide.
        template <int NT>
        __device__ void apply_q_block(const double *W, size_t ld, const double *hh, uint32_t F, uint32_t Fc, uint32_t dim, uint32_t rank, double *v,
                                      double *bcast, uint32_t tid)
        {
            for (uint32_t j = rank; j--;)
            {
                const uint32_t rows = dim - j;
                const double tau    = hh[F + j];
                const double *ess   = W + (F + j + 1) + (size_t)(Fc + j) * ld;
                if (rows == 1)
                {
                    if (tid == 0) v[j] *= (1.0 - tau);
                    __syncthreads();
                }
                else if (tau != 0.0)
                {
                    if (tid == 0)
                    {
                        double t = chain_dot<8>(ess, v + j + 1, rows - 1, 0.0);
                        t += v[j];
                        *bcast = t;
                    }
                    __syncthreads();
                    const double t = *bcast;
                    for (uint32_t i = tid; i < rows; i += NT)
                    {
                        if (i == 0)
                            v[j] = dfma(-tau, t, v[j]);
                        else
                            v[j + i] = dfma(-(tau * ess[i - 1]), t, v[j + i]);
                    }
                    __syncthreads();
                }
            }
        }

        /// apply_q_block for ONE wavefront and a level of at most 64 rows: lane i keeps v[i] in a register, the ordered dot product of
        /// a reflector walks the lanes with v_readlane (a few cycles per term instead of a dependent LDS round trip), the update is
        /// lane-local and there is no barrier inside the sequence.  Same chains, same order, same results.
        __device__ __forceinline__ void apply_q_wave(const double *W, size_t ld, const double *hh, uint32_t F, uint32_t Fc, uint32_t dim, uint32_t rank, double *v,
                                                     uint32_t lane)
        {
            double vi = lane < dim ? v[lane] : 0.0;
            for (uint32_t j = rank; j--;)
            {
                const uint32_t rows = dim - j;
                const double tau    = hh[F + j];
                if (rows == 1)
                {
                    if (lane == j) vi *= (1.0 - tau);
                }
                else if (tau != 0.0)
                {
                    const bool tail = lane > j && lane < dim;
                    const double e  = tail ? W[(F + lane) + (size_t)(Fc + j) * ld] : 0.0; // essential part: entry of row j + i sits in lane j + i
                    double t        = 0.0;
                    for (uint32_t i = 1; i < rows; i++)
                    {
                        const int l     = (int)(j + i);
                        const double ei = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(e), l), __builtin_amdgcn_readlane(__double2loint(e), l));
                        const double xi = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(vi), l), __builtin_amdgcn_readlane(__double2loint(vi), l));
                        t               = dfma(ei, xi, t);
                    }
                    t += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(vi), (int)j), __builtin_amdgcn_readlane(__double2loint(vi), (int)j));
                    if (lane == j)
                        vi = dfma(-tau, t, vi);
                    else if (tail)
                        vi = dfma(-(tau * e), t, vi);
                }
            }
            if (lane < dim) v[lane] = vi;
            __syncthreads();
        }

        /// x = P x (lexlse.h:1044): the transpositions k <-> perm[k], last first, on x by position — read the other way round: variable i follows
        /// them first to last from position i to its final position p, and x_i is what sits there.  Every thread for its own variables, on indices
        /// only (one thread swapping entries behind a load of perm[k] each was 128 of the 150 us of configs[1]'s solve).  perm_l: LDS scratch of T
        /// words, 16-BYTE ALIGNED (it is read four words at a time), that nothing else uses while this runs; xs: x by position (LDS)
        template <int NT>
        __device__ __forceinline__ void apply_permutation_by_following(const LseArgs &a, uint32_t b, const uint32_t *perm, uint32_t T, const double *xs, uint32_t *perm_l, uint32_t tid)
        {
            const uint32_t n = a.nVar;
            for (uint32_t k = tid; k < T; k += NT) perm_l[k] = perm[k];
            __syncthreads();
            // (UV variables per thread and pass: independent index chains side by side)
            auto follow = [&](auto uv_c, uint32_t i0) __attribute__((always_inline)) {
                constexpr int UV = decltype(uv_c)::value;
                uint32_t p[UV];
#pragma unroll
                for (int u = 0; u < UV; u++) p[u] = i0 + u * NT;
                for (uint32_t k = 0; k + 4 <= T; k += 4)
                {
                    const uint4 pk4      = *reinterpret_cast<const uint4 *>(perm_l + k);
                    const uint32_t pk[4] = {pk4.x, pk4.y, pk4.z, pk4.w};
#pragma unroll
                    for (int kk = 0; kk < 4; kk++)
#pragma unroll
                        for (int u = 0; u < UV; u++) p[u] = (p[u] == k + kk) ? pk[kk] : ((p[u] == pk[kk]) ? k + kk : p[u]);
                }
                for (uint32_t k = T & ~3u; k < T; k++)
                {
                    const uint32_t pk = perm_l[k];
#pragma unroll
                    for (int u = 0; u < UV; u++) p[u] = (p[u] == k) ? pk : ((p[u] == pk) ? k : p[u]);
                }
#pragma unroll
                for (int u = 0; u < UV; u++)
                    if (i0 + u * NT < n) a.x[(size_t)b * n + i0 + u * NT] = xs[p[u]];
            };
            const uint32_t rows = (n + NT - 1) / NT; // variables per thread (the last pass may reach beyond n: those are not stored)
            uint32_t done       = 0;
            for (; rows - done >= 4; done += 4) follow(std::integral_constant<int, 4>{}, tid + done * NT);
            switch (rows - done)
            {
            case 3: follow(std::integral_constant<int, 3>{}, tid + done * NT); break;
            case 2: follow(std::integral_constant<int, 2>{}, tid + done * NT); break;
            case 1: follow(std::integral_constant<int, 1>{}, tid + done * NT); break;
            default: break;
            }
        }
    } // namespace
} // namespace lexls
