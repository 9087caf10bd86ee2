// What follows a run of a lock-step LexLSI batch (lsi_batch.h): the working sets it leaves behind, the final equality problems formed and factorized from
// them with the factor kept, and the calls that work on that factor — getLambda and the gradients of the solutions (bounds, many cotangents, matrices).
#pragma once
#include <array>
#include <atomic>
#include <memory>
#include "lsi_batch_ctx.h"
#include "lsi_worker_pool.h"

namespace
{
    /// getLambda's last loop (lexlsi.h:592-604) for a whole group: the rows of the multiplier matrices (lexls_lse_multipliers: B x nObjL x ldo,
    /// row r = r-th active constraint in working-set order, simple bounds first) go to the user's order — instance b's output is total x nObj,
    /// column-major, column off + k = LexLSE objective k, column 0 zero when objective 0 holds simple bounds, inactive rows zero.
    /// One workgroup per instance, lane = active constraint; map = [nact (B) | pos (B x total): user row of active constraint r].
    /// fault (lexls_lsi_batch_enqueue_device; else NULL): the run's fault word — with it set nothing is written
    /// mask (the group's bytes of lexls_lsi_batch_set_instance_mask, or NULL): `out` is the caller's d_lambda and the rows of a skipped instance stay as they are
    __global__ __launch_bounds__(64) void lsi_lambda_scatter_kernel(const double *__restrict__ mult, const uint32_t *__restrict__ map, uint32_t B, uint32_t total,
                                                                    uint32_t nObj, uint32_t nObjL, uint32_t off, uint32_t ldo, double *__restrict__ out,
                                                                    const uint32_t *__restrict__ fault, const uint8_t *mask)
    {
        if (fault && *fault != 0xffffffffu) return;
        const uint32_t b = blockIdx.x;
        if (lsi_mask_byte(mask, b) == 0) return; // (block-uniform)
        double *o        = out + (size_t)b * total * nObj;
        for (uint32_t i = threadIdx.x; i < total * nObj; i += blockDim.x) o[i] = 0.0;
        __syncthreads();
        const uint32_t na   = min(map[b], min(total, ldo));
        const uint32_t *pos = map + B + (size_t)b * total;
        const double *m     = mult + (size_t)b * nObjL * ldo;
        for (uint32_t r = threadIdx.x; r < na; r += blockDim.x)
        {
            const uint32_t u = pos[r];
            if (u >= total) continue;
            for (uint32_t k = 0; k < nObjL; k++) o[u + (size_t)(off + k) * total] = m[(size_t)k * ldo + r];
        }
    }

    /// lexls_lsi_batch_solve_adjoint and lexls_lsi_batch_solve_adjoint_multi for a whole group (the single call: ncot = 1, a grid of B x 1): the adjoint of
    /// the final equality problems (lexls_lse_solve_adjoint(_multi)_device: grad_rhs B x ncot x cap in LOD row order, grad_fixed B x ncot x n in fixVariable
    /// order) goes to the user's constraint order — out_lb / out_ub are B x ncot x total (either may be NULL).  Block (b, c) — one wavefront — serves
    /// cotangent c of instance b: row b * ncot + c of the gradients and of the outputs.  map = [nact (B) | pos (B x total)] as for
    /// lsi_lambda_scatter_kernel: row r of the final problem (the nf fixed variables first, then the LOD rows) is user row pos[r]; types (B x total) = its
    /// activation type, in the same row order; meta (B x 2) = the instance's status of the run and nf (map, types, meta: per instance, whatever ncot).
    /// CTR_ACTIVE_LB goes to out_lb, CTR_ACTIVE_UB and CTR_ACTIVE_EQ to out_ub (the bound form_final_problem posts); an instance that did not end
    /// PROBLEM_SOLVED has no active rows here.  The zeros and the active values meet in an LDS tile of ADJ_TILE user rows (pos is injective: no two
    /// rows of the map claim one entry, no atomics), then the lanes run along the user rows: every entry of the outputs is stored once, by consecutive lanes.
    /// mask (the group's bytes of lexls_lsi_batch_set_instance_mask, or NULL): a skipped instance writes none of its ncot rows
    constexpr uint32_t ADJ_TILE = 1024;
    __global__ __launch_bounds__(64) void lsi_adjoint_scatter_multi_kernel(const double *__restrict__ grad_rhs, const double *__restrict__ grad_fixed,
                                                                           const uint32_t *__restrict__ map, const uint8_t *__restrict__ types,
                                                                           const int32_t *__restrict__ meta, uint32_t B, uint32_t ncot, uint32_t total, uint32_t n, uint32_t cap,
                                                                           double *__restrict__ out_lb, double *__restrict__ out_ub, const uint8_t *mask)
    {
        __shared__ double s_lb[ADJ_TILE], s_ub[ADJ_TILE];
        const uint32_t b = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
        if (b >= B || c >= ncot || lsi_mask_byte(mask, b) == 0) return; // (block-uniform)
        const uint32_t nf   = min((uint32_t)max(meta[2 * b + 1], 0), n);
        const uint32_t na   = meta[2 * b] == (int32_t)PROBLEM_SOLVED ? min(map[b], min(total, nf + cap)) : 0u;
        const uint32_t *pos = map + B + (size_t)b * total;
        const uint8_t *ty   = types + (size_t)b * total;
        const size_t row    = (size_t)b * ncot + c;
        const double *gr = grad_rhs + row * cap, *gf = grad_fixed + row * n;
        for (uint32_t u0 = 0; u0 < total; u0 += ADJ_TILE)
        {
            const uint32_t len = min(ADJ_TILE, total - u0);
            for (uint32_t i = lane; i < len; i += 64) s_lb[i] = s_ub[i] = 0.0;
            __syncthreads();
            for (uint32_t r = lane; r < na; r += 64)
            {
                const uint32_t u = pos[r];
                if (u < u0 || u - u0 >= len) continue;
                const double val = r < nf ? gf[r] : gr[r - nf];
                const uint8_t t  = ty[r];
                if (t == CTR_ACTIVE_LB)
                    s_lb[u - u0] = val;
                else if (t == CTR_ACTIVE_UB || t == CTR_ACTIVE_EQ)
                    s_ub[u - u0] = val;
            }
            __syncthreads();
            for (uint32_t i = lane; i < len; i += 64)
            {
                if (out_lb) out_lb[row * total + u0 + i] = s_lb[i];
                if (out_ub) out_ub[row * total + u0 + i] = s_ub[i];
            }
            __syncthreads();
        }
    }

    /// lexls_lsi_batch_solve_adjoint_matrix for a whole group: the matrix gradient of the final equality problems (launch_solve_adjoint_matrix:
    /// grad_lod B x (n + 1) x cap in the layout of the problem data — entry (LOD row i, column j) at j * cap + i, column n = y = M^T g — and grad_fixed
    /// B x n = N^T g in fixVariable order) goes to the caller's constraint data layout: instance b's slice of `out` is per_data doubles, per
    /// objective o a column-major dim x w block at shape[4 o + 2] (w = n + 2, [A | lb | ub], where shape[4 o + 1] != 0: a general objective; else
    /// w = 2, [lb | ub]); shape (nObj x 4) = {dim, general, offset of the block, first user row} of every objective.  map, types and meta are
    /// lsi_adjoint_scatter_multi_kernel's (one upload per run serves both): row r of the final problem (the nf fixed variables first, then the LOD rows)
    /// is user row pos[r].  An active general row takes its row of grad_lod in the A columns and its y in the lb (CTR_ACTIVE_LB) or ub column
    /// (CTR_ACTIVE_UB, CTR_ACTIVE_EQ); an active simple bound takes its slot of grad_fixed by the same rule; every other entry is an exact zero.
    /// differentiable[b] (may be NULL) = lse_flag[b] (the rank-stability flag of the final problem, launch_solve_adjoint_matrix's; NULL: the group
    /// launched no chain, nobody has an active constraint) && status PROBLEM_SOLVED — where it is 0 the whole slice is exact zeros.
    /// One workgroup of ADJM_NT threads per instance.  Per objective and tile of ADJM_TILE user rows the inverse of pos is formed in LDS (one word
    /// per user row: final-problem row + 1 | type << 24; pos is injective: no two rows claim one word, no atomics), then the threads run along the
    /// tile's entries in the order they are stored — along the user rows of one data column, column after column, consecutive threads at
    /// consecutive addresses (an objective of at most ADJM_TILE rows is one contiguous run) — so every entry of the slice is stored exactly once,
    /// zeros and values alike; the reads of grad_lod are the scattered side.
    /// mask (the group's bytes of lexls_lsi_batch_set_instance_mask, or NULL): slice and flag of a skipped instance stay as they are
    constexpr uint32_t ADJM_TILE = 1024, ADJM_NT = 256;
    __global__ __launch_bounds__(ADJM_NT) void lsi_adjoint_matrix_scatter_kernel(const double *__restrict__ grad_lod, const double *__restrict__ grad_fixed,
                                                                                 const uint8_t *__restrict__ lse_flag, const uint32_t *__restrict__ map,
                                                                                 const uint8_t *__restrict__ types, const int32_t *__restrict__ meta,
                                                                                 const uint32_t *__restrict__ shape, uint32_t B, uint32_t nObj, uint32_t total, uint32_t n,
                                                                                 uint32_t cap, size_t per_data, double *__restrict__ out,
                                                                                 uint8_t *__restrict__ differentiable, const uint8_t *mask)
    {
        __shared__ uint32_t s_row[ADJM_TILE];
        const uint32_t b = blockIdx.x, tid = threadIdx.x;
        if (b >= B || lsi_mask_byte(mask, b) == 0) return; // (block-uniform)
        const uint32_t nf     = min((uint32_t)max(meta[2 * b + 1], 0), n);
        const uint32_t na_all = min(map[b], min(total, nf + cap));
        const bool diff       = meta[2 * b] == (int32_t)PROBLEM_SOLVED && (na_all == 0 || (lse_flag && lse_flag[b] != 0)); // (an empty working set: x = 0 whatever the data)
        const uint32_t na     = diff ? na_all : 0u;
        if (tid == 0 && differentiable) differentiable[b] = diff ? 1 : 0;
        const uint32_t *pos = map + B + (size_t)b * total;
        const uint8_t *ty   = types + (size_t)b * total;
        const double *gl = grad_lod + (size_t)b * cap * (n + 1), *gf = grad_fixed + (size_t)b * n;
        double *o_b      = out + (size_t)b * per_data;
        for (uint32_t o = 0; o < nObj; o++)
        {
            const uint32_t dim = shape[4 * o], general = shape[4 * o + 1], first = shape[4 * o + 3];
            const uint32_t w   = general ? n + 2 : 2u, col_lb = w - 2;
            double *o_k        = o_b + shape[4 * o + 2];
            for (uint32_t t0 = 0; t0 < dim; t0 += ADJM_TILE)
            {
                const uint32_t len = min(ADJM_TILE, dim - t0), u0 = first + t0;
                for (uint32_t i = tid; i < len; i += ADJM_NT) s_row[i] = 0u;
                __syncthreads();
                for (uint32_t r = tid; r < na; r += ADJM_NT)
                {
                    const uint32_t u = pos[r];
                    if (u < u0 || u - u0 >= len) continue;
                    s_row[u - u0] = (r + 1) | ((uint32_t)ty[r] << 24);
                }
                __syncthreads();
                for (uint32_t e = tid; e < len * w; e += ADJM_NT)
                {
                    const uint32_t j = e / len, i = e - j * len, code = s_row[i];
                    double val = 0.0;
                    if (code)
                    {
                        const uint32_t r = (code & 0xffffffu) - 1, t = code >> 24;
                        const bool to_lb = t == CTR_ACTIVE_LB, to_ub = t == CTR_ACTIVE_UB || t == CTR_ACTIVE_EQ;
                        if (j < col_lb)
                        {
                            if (r >= nf && (to_lb || to_ub)) val = gl[(size_t)j * cap + (r - nf)];
                        }
                        else if (j == col_lb ? to_lb : to_ub)
                            val = r < nf ? gf[r] : gl[(size_t)n * cap + (r - nf)];
                    }
                    o_k[(size_t)j * dim + t0 + i] = val;
                }
                __syncthreads();
            }
        }
    }
    /// lexls_lsi_batch_solve_tangent for a whole group: the transpose of lsi_adjoint_matrix_scatter_kernel, with its routes (map, types, meta, shape).
    /// Direction c = blockIdx.y of instance b = blockIdx.x (the caller's ddata: ntan x batch x per_data, the layout lexls_lsi_batch_run_device reads;
    /// the group's instances start at instance lo of the batch) becomes the direction of its final equality problem, in the layouts
    /// lexls_lse_solve_tangent_device reads: dlod (ntan x B x (n + 1) x cap: entry (LOD row i, column j) at j * cap + i) and dfixed (ntan x B x n).
    /// Row r of the final problem (the nf fixed variables first, then the LOD rows) is user row pos[r]: an active general row contributes its dA row
    /// and dlb (CTR_ACTIVE_LB) or dub (CTR_ACTIVE_UB, CTR_ACTIVE_EQ) — the bound the final problem reads —, an active simple bound its slot of
    /// dfixed by the same rule.  Rows outside the working set, and rows absent under lexls_lsi_batch_set_instance_obj_dims, are never read; LOD rows
    /// behind the problem's own and slots behind nf are not written (the equality solver does not read them).
    /// The threads run along the LOD rows of one column of dlod, column after column: consecutive threads store at consecutive addresses; the
    /// reads of ddata are the scattered side.  No atomics.  A masked instance is skipped.
    __global__ __launch_bounds__(ADJM_NT) void lsi_tangent_gather_kernel(const double *__restrict__ ddata, const uint32_t *__restrict__ map, const uint8_t *__restrict__ types,
                                                                         const int32_t *__restrict__ meta, const uint32_t *__restrict__ shape, uint32_t B, uint32_t batch,
                                                                         uint32_t lo, uint32_t ntan, uint32_t nObj, uint32_t total, uint32_t n, uint32_t cap, size_t per_data,
                                                                         double *__restrict__ dlod, double *__restrict__ dfixed, const uint8_t *mask)
    {
        const uint32_t b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
        if (b >= B || c >= ntan || lsi_mask_byte(mask, b) == 0) return; // (block-uniform)
        const uint32_t nf = min((uint32_t)max(meta[2 * b + 1], 0), n);
        const uint32_t na = min(map[b], min(total, nf + cap));
        if (na == 0) return;
        const uint32_t *pos = map + B + (size_t)b * total;
        const uint8_t *ty   = types + (size_t)b * total;
        const double *d_b   = ddata + ((size_t)c * batch + lo + b) * per_data;
        double *lod = dlod + ((size_t)c * B + b) * cap * (n + 1), *fx = dfixed + ((size_t)c * B + b) * n;
        const uint32_t M = na - nf; // LOD rows of the final problem
        // (entry e: LOD row i of column j, j == n + 1 standing for the fixed slots)
        for (uint32_t e = tid; e < M * (n + 1) + nf; e += ADJM_NT)
        {
            const bool fixed_slot = e >= M * (n + 1);
            const uint32_t j = fixed_slot ? n : e / M, r = fixed_slot ? e - M * (n + 1) : nf + (e - j * M);
            const uint32_t u = pos[r], t = ty[r];
            const bool from_lb = t == CTR_ACTIVE_LB, from_ub = t == CTR_ACTIVE_UB || t == CTR_ACTIVE_EQ;
            double val = 0.0;
            for (uint32_t o = 0; o < nObj; o++) // the objective of user row u
            {
                const uint32_t dim = shape[4 * o], first = shape[4 * o + 3];
                if (u < first || u - first >= dim) continue;
                const uint32_t w = shape[4 * o + 1] ? n + 2 : 2u;
                const double *blk = d_b + shape[4 * o + 2];
                if (j < n)
                {
                    if (w > 2 && (from_lb || from_ub)) val = blk[(size_t)j * dim + (u - first)];
                }
                else if (from_lb)
                    val = blk[(size_t)(w - 2) * dim + (u - first)];
                else if (from_ub)
                    val = blk[(size_t)(w - 1) * dim + (u - first)];
                break;
            }
            if (fixed_slot)
                fx[r] = val;
            else
                lod[(size_t)j * cap + (r - nf)] = val;
        }
    }

    /// The tangents of the final equality problems (dx_lse: ntan x B x n, lexls_lse_solve_tangent_device's) into the caller's dx (ntan x batch x n) with
    /// the conventions of lsi_adjoint_matrix_scatter_kernel: differentiable[b] = status PROBLEM_SOLVED && (empty working set || lse_flag[b]); where it
    /// is 0, and for an empty working set (x = 0 whatever the data), the instance's rows of dx are exact zeros.  lse_flag / dx_lse NULL: the group
    /// launched no chain.  A masked instance keeps the bits of its rows and of its flag.  Consecutive threads at consecutive addresses.
    __global__ __launch_bounds__(64) void lsi_tangent_finish_kernel(const double *__restrict__ dx_lse, const uint8_t *__restrict__ lse_flag, const uint32_t *__restrict__ map,
                                                                    const int32_t *__restrict__ meta, uint32_t B, uint32_t batch, uint32_t lo, uint32_t ntan, uint32_t total,
                                                                    uint32_t n, uint32_t cap, double *__restrict__ dx, uint8_t *__restrict__ differentiable, const uint8_t *mask)
    {
        const uint32_t b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
        if (b >= B || c >= ntan || lsi_mask_byte(mask, b) == 0) return; // (block-uniform)
        const uint32_t nf = min((uint32_t)max(meta[2 * b + 1], 0), n);
        const uint32_t na = min(map[b], min(total, nf + cap));
        const bool diff   = meta[2 * b] == (int32_t)PROBLEM_SOLVED && (na == 0 || (lse_flag && lse_flag[b] != 0));
        if (c == 0 && tid == 0 && differentiable) differentiable[b] = diff ? 1 : 0;
        const bool live = diff && na != 0 && dx_lse;
        for (uint32_t i = tid; i < n; i += 64) dx[((size_t)c * batch + lo + b) * n + i] = live ? dx_lse[((size_t)c * B + b) * n + i] : 0.0;
    }

    /// lexls_lsi_batch_solve_bounds for a whole group, first half: the transpose of lsi_adjoint_scatter_multi_kernel, with the routes of
    /// lsi_tangent_gather_kernel (map, types, meta).  Bound set c = blockIdx.y of instance b = blockIdx.x (the caller's lb / ub: nrhs x batch x total,
    /// user's constraint order; the group's instances start at instance lo of the batch) becomes the right-hand side of its final equality problem in
    /// the layouts lexls_lse_solve_rhs_device reads: rhs (nrhs x B x cap, LOD row order) and fixed (nrhs x B x n, fixVariable order).  Row r of the
    /// final problem (the nf fixed variables first, then the LOD rows) is user row pos[r] and takes lb (CTR_ACTIVE_LB) or ub (CTR_ACTIVE_UB,
    /// CTR_ACTIVE_EQ) of that row — the bound form_final_problem posts.  Rows outside the working set (and so every row absent under
    /// lexls_lsi_batch_set_instance_obj_dims) are never read; rows behind the problem's own and slots behind nf are not written (the equality solver
    /// does not read them).  The threads run along the rows of the final problem: consecutive threads store at consecutive addresses, the reads of
    /// lb / ub are the scattered side.  No atomics.  A masked instance is skipped.
    __global__ __launch_bounds__(64) void lsi_bounds_gather_kernel(const double *__restrict__ lbq, const double *__restrict__ ubq, const uint32_t *__restrict__ map,
                                                                   const uint8_t *__restrict__ types, const int32_t *__restrict__ meta, uint32_t B, uint32_t batch, uint32_t lo,
                                                                   uint32_t nrhs, uint32_t total, uint32_t n, uint32_t cap, double *__restrict__ rhs, double *__restrict__ fixed,
                                                                   const uint8_t *mask)
    {
        const uint32_t b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
        if (b >= B || c >= nrhs || lsi_mask_byte(mask, b) == 0) return; // (block-uniform)
        const uint32_t nf   = min((uint32_t)max(meta[2 * b + 1], 0), n);
        const uint32_t na   = min(map[b], min(total, nf + cap));
        const uint32_t *pos = map + B + (size_t)b * total;
        const uint8_t *ty   = types + (size_t)b * total;
        const size_t in     = ((size_t)c * batch + lo + b) * total;
        double *r_b = rhs + ((size_t)c * B + b) * cap, *f_b = fixed + ((size_t)c * B + b) * n;
        for (uint32_t r = tid; r < na; r += 64)
        {
            const uint32_t u = pos[r], t = ty[r];
            double val = 0.0;
            if (u < total)
            {
                if (t == CTR_ACTIVE_LB)
                    val = lbq[in + u];
                else if (t == CTR_ACTIVE_UB || t == CTR_ACTIVE_EQ)
                    val = ubq[in + u];
            }
            if (r < nf)
                f_b[r] = val;
            else
                r_b[r - nf] = val;
        }
    }

    /// lexls_lsi_batch_solve_bounds for a whole group, second half: x into the caller's layout, the valid flags and the violations.  One wavefront per
    /// instance b = blockIdx.x and tile of 64 bound sets (blockIdx.y), lane = bound set c.
    /// x_lse (nrhs x B x n, lexls_lse_solve_rhs_device's; NULL: the group factorized nothing) goes to x (nrhs x batch x n) — exact zeros where the
    /// instance did not end PROBLEM_SOLVED, and for an empty working set —, the lanes running along the tile's vectors one after the other: runs of n
    /// consecutive addresses on both sides.
    /// XLDS: on the way the tile's vectors are transposed into LDS ([variable][lane], leading dimension 65); else each lane reads its own from x.
    /// violation[c, b] = the largest of max(lb - a.x, a.x - ub, lb - ub, 0) over all present rows of all objectives (a simple bound: x[var] for a.x),
    /// 0 where the instance did not end PROBLEM_SOLVED.  The rows of the resident constraint data (cdata: B x per_data, lexls_lsi_batch_run_device's
    /// layout; shape: the objectives' {dim, general, offset, first row}; var: B x dims[0] variable indices; counts: B x counts_ld present rows per
    /// objective, or NULL) are read once per tile at wavefront-uniform addresses; every lane accumulates a.x as its own ordered fma chain over
    /// j = 0 .. n - 1 (no cross-lane sums: a bound set's bits do not depend on nrhs, its position or its company).  lb / ub of kBoundsCheckRows rows
    /// at a time are loaded along the rows (consecutive lanes at consecutive addresses) and turned to [row][lane] in LDS.  Rows at and behind an
    /// instance's count are never read.  valid[b] = status PROBLEM_SOLVED, written by tile 0.  A masked instance keeps the bits of all three outputs.
    /// COST (lexls_lsi_batch_solve_bounds_cost: "lsi_bounds_cost<lds|hbm>"; false: every line of it is compiled out, and `cost` is not read):
    /// besides, cost[c, b, o] (nrhs x batch x nObj) = the sum over objective o's present rows, in the user's row order, of d^2, d = max(lb - a.x,
    /// a.x - ub, 0) with the very a.x of the violation — the lane's own ordered fma chain —, exact zeros where the instance did not end
    /// PROBLEM_SOLVED; x may be NULL there (not wanted).
    template <bool XLDS, bool COST = false>
    __global__ __launch_bounds__(64) void lsi_bounds_check_kernel(const double *__restrict__ x_lse, const double *__restrict__ lbq, const double *__restrict__ ubq,
                                                                  const double *__restrict__ cdata, const uint32_t *__restrict__ var, const uint32_t *__restrict__ counts,
                                                                  uint32_t counts_ld, const uint32_t *__restrict__ map, const int32_t *__restrict__ meta,
                                                                  const uint32_t *__restrict__ shape, uint32_t B, uint32_t batch, uint32_t lo, uint32_t nrhs, uint32_t nObj,
                                                                  uint32_t total, uint32_t n, uint32_t cap, size_t per_data, double *__restrict__ x, double *__restrict__ violation,
                                                                  uint8_t *__restrict__ valid, const uint8_t *mask, double *__restrict__ cost)
    {
        extern __shared__ double s_bounds[];
        constexpr uint32_t LD = lexls::kAdjointMultiLd, ROWS = lexls::kBoundsCheckRows;
        double *s_lb = s_bounds, *s_ub = s_bounds + ROWS * LD, *s_x = s_bounds + 2 * ROWS * LD; // (s_x: XLDS only)
        const uint32_t b = blockIdx.x, c0 = blockIdx.y * 64u, lane = threadIdx.x;
        if (b >= B || c0 >= nrhs || lsi_mask_byte(mask, b) == 0) return; // (block-uniform)
        const uint32_t nc   = min(64u, nrhs - c0), c = c0 + lane;
        const bool solved   = meta[2 * b] == (int32_t)PROBLEM_SOLVED;
        const uint32_t nf   = min((uint32_t)max(meta[2 * b + 1], 0), n);
        const uint32_t na   = min(map[b], min(total, nf + cap));
        const bool live     = solved && na != 0 && x_lse; // (else x = 0: an empty working set, or no answer)
        if (blockIdx.y == 0 && lane == 0 && valid) valid[b] = solved ? 1 : 0;
        // ---- x: the tile's nc vectors, element e of vector cc at a time ----
        for (uint32_t e = lane; e < nc * n; e += 64)
        {
            const uint32_t cc = e / n, j = e - cc * n;
            const double val  = live ? x_lse[((size_t)(c0 + cc) * B + b) * n + j] : 0.0;
            if (!COST || x) x[((size_t)(c0 + cc) * batch + lo + b) * n + j] = val;
            if (XLDS) s_x[j * LD + cc] = val;
        }
        if (!solved) // (block-uniform: exact zeros)
        {
            if (violation && lane < nc) violation[(size_t)c * batch + lo + b] = 0.0;
            if constexpr (COST)
                for (uint32_t e = lane; e < nc * nObj; e += 64) cost[((size_t)(c0 + e / nObj) * batch + lo + b) * nObj + e % nObj] = 0.0;
            return;
        }
        if (!COST && !violation) return;
        __syncthreads();
        const double *xg    = live ? x_lse + ((size_t)min(c, nrhs - 1) * B + b) * n : NULL; // (!XLDS: the lane's own vector)
        const double *d_b   = cdata + (size_t)b * per_data;
        const size_t in     = ((size_t)c0 * batch + lo + b) * total;         // bound set c0's rows of this instance
        const size_t in_ld  = (size_t)batch * total;                          // from one bound set to the next
        double viol = 0.0;
        for (uint32_t o = 0; o < nObj; o++)
        {
            const uint32_t dim = shape[4 * o], general = shape[4 * o + 1], first = shape[4 * o + 3];
            const uint32_t cnt = counts && o < counts_ld ? min(counts[(size_t)b * counts_ld + o], dim) : dim;
            const double *blk  = d_b + shape[4 * o + 2];
            [[maybe_unused]] double co = 0.0; // (COST: the objective's cost of this lane's bound set)
            for (uint32_t i0 = 0; i0 < cnt; i0 += ROWS)
            {
                const uint32_t len = min(ROWS, cnt - i0);
                // the chunk's bounds: ROWS consecutive rows of 64 / ROWS bound sets per pass
                for (uint32_t e = lane; e < ROWS * 64u; e += 64)
                {
                    const uint32_t cc = e / ROWS, rr = e % ROWS;
                    if (cc < nc && rr < len)
                    {
                        const size_t at = in + (size_t)cc * in_ld + first + i0 + rr;
                        s_lb[rr * LD + cc] = lbq[at];
                        s_ub[rr * LD + cc] = ubq[at];
                    }
                }
                __syncthreads();
                for (uint32_t rr = 0; rr < len; rr++)
                {
                    const uint32_t i = i0 + rr;
                    double ax = 0.0;
                    if (general)
                    {
                        if (live)
                            for (uint32_t j = 0; j < n; j++) ax = fma(blk[(size_t)j * dim + i], XLDS ? s_x[j * LD + lane] : xg[j], ax);
                    }
                    else if (live && o == 0)
                    {
                        const uint32_t vi = var ? var[(size_t)b * dim + i] : n; // (objective 0 alone holds simple bounds: dim = dims[0])
                        if (vi < n) ax = XLDS ? s_x[vi * LD + lane] : xg[vi];
                    }
                    if (lane < nc)
                    {
                        const double l = s_lb[rr * LD + lane], u = s_ub[rr * LD + lane];
                        viol = fmax(viol, fmax(fmax(l - ax, ax - u), l - u));
                        if constexpr (COST)
                        {
                            const double d = fmax(fmax(l - ax, ax - u), 0.0);
                            co             = fma(d, d, co);
                        }
                    }
                }
                __syncthreads();
            }
            if constexpr (COST)
                if (lane < nc) cost[((size_t)c * batch + lo + b) * nObj + o] = co;
        }
        if ((!COST || violation) && lane < nc) violation[(size_t)c * batch + lo + b] = viol;
    }
} // namespace

/// What the after-run stage reads of the batch object (lexls_lsi_batch_s derives from it): its shape, the groups with their equality-solver handles and
/// streams, the worker pool and the instance mask.  The run fills it; the stage changes nothing here but what lives in the groups' handles.
struct LsiBatchShape
{
    int device;
    uint32_t batch, nVar, nObj, off = 0;
    std::vector<uint32_t> dims;
    std::vector<int32_t> types;
    size_t per_data = 0, total = 0;
    bool gather = false;
    uint32_t nGroups = 1;
    std::vector<std::unique_ptr<BatchCtx>> grp;
    std::vector<uint32_t> lo, group_of;
    std::unique_ptr<WorkerPool> pool;
    // ---- lexls_lsi_batch_set_instance_mask: batch bytes in device memory, the caller's; read by the kernels of every device run while set, never on the host ----
    const uint8_t *d_mask = NULL;
    const uint8_t *group_mask(uint32_t g) const { return d_mask ? d_mask + lo[g] : NULL; }
    LsiBatchShape(int device_, uint32_t batch_, uint32_t nVar_, uint32_t nObj_) : device(device_), batch(batch_), nVar(nVar_), nObj(nObj_) {}
};

/// The after-run stage of a lock-step batch.  The run calls begin_run / forget when it starts, keep_working_set(_resident) for every instance when it
/// ends, and set_rule; what the caller asks for afterwards — get_lambda, solve_adjoint, solve_adjoint_multi, solve_adjoint_matrix — is served here.
struct LsiFinal
{
    const LsiBatchShape &s;
    // ---- getLambda of the last run (lexls_lsi_batch_get_lambda, lexlsi.h:552-605) ----
    // What the run leaves behind for it: every instance's final working set in working-set order and its active simple bounds (variable and
    // bound value, the fixed variables of formLexLSE, objective.h:255-272); the general rows are gathered from the constraint data that stays
    // resident in the group handles.  lam_rc: -1 no run yet (or the last one failed), LEXLS_OK, or the code get_lambda returns (lam_msg).
    int lam_rc = -1;
    std::string lam_msg;
    double lam_tol = 1e-12;           // tol_linear_dependence of that run (the factorizations of getLambda use it, as the reference's do)
    std::vector<uint32_t> data_off;   // per objective: offset of its block in one instance's constraint data
    std::vector<uint32_t> first;      // per objective: its first row among an instance's `total` constraints
    std::vector<uint16_t> ws_na;      // batch x nObj: active constraints per objective
    std::vector<uint16_t> ws_idx;     // batch x total: per objective (from its first row on) the active constraints in working-set order
    std::vector<uint8_t> ws_type;     // batch x total: their activation types
    std::vector<uint32_t> ws_fixvar;  // batch x dims[0] (simple bounds only): variables of the active simple bounds, working-set order
    std::vector<double> ws_fixval;    // batch x dims[0]: the bound each one is fixed at
    std::vector<int32_t> ws_status;   // batch: every instance's TerminationStatus of the last run, from its host object or the resident slab
    std::vector<uint32_t> ws_var;     // batch x dims[0] (simple bounds only): the variable of every simple bound, where the run had them on the host (keep_fixed)
    struct Bufs                       // per group, made at the first get_lambda
    {
        Pinned<uint32_t> map;         // [nact (B) | pos (B x total)]
        uint32_t *d_map = NULL;
        double *d_out   = NULL;       // B x total x nObj
        // the gradient calls (ensure_adjoint_bufs): the activation type of every row of the map and [status of the run | nfixed] per instance, for the
        // scatter kernels, made at the first call; with room for m_room cotangents per instance (the largest ncot so far; 1: the single call and the
        // matrix call) g and the two outputs of a host caller and the adjoint of the final equality problems (grad_rhs B x m_room x cap, grad_fixed
        // B x m_room x nVar)
        Pinned<uint8_t> types;        // B x total
        Pinned<int32_t> meta;         // B x 2
        uint8_t *d_types = NULL;
        int32_t *d_meta  = NULL;
        double *d_g = NULL, *d_grad_rhs = NULL, *d_grad_fixed = NULL, *d_grad_lb = NULL, *d_grad_ub = NULL;
        uint32_t m_room = 0;
        // lexls_lsi_batch_solve_adjoint_matrix (ensure_adjoint_matrix_bufs): the matrix gradient of the final equality problems (B x (nVar + 1) x cap)
        // and their rank-stability flags (B), the objectives' {dim, general, offset, first row} for lsi_adjoint_matrix_scatter_kernel (the same for every
        // group; uploaded when made); grad_data (B x per_data) and the flags (B) of a host caller, made at the first host call
        double *d_grad_lod = NULL, *d_mat_out = NULL;
        uint8_t *d_lse_flag = NULL, *d_mat_flag = NULL;
        uint32_t *d_shape = NULL;
        // lexls_lsi_batch_solve_tangent (ensure_tangent_bufs): the directions of the final equality problems (t_room x B x (nVar + 1) x cap and t_room x B x
        // nVar) and their tangents (t_room x B x nVar), made for the largest ntan so far
        double *d_tan_dlod = NULL, *d_tan_dfixed = NULL, *d_tan_dx = NULL;
        uint32_t t_room = 0;
        // lexls_lsi_batch_solve_bounds (ensure_bounds_bufs): the right-hand sides of the final equality problems (b_room x B x cap and b_room x B x nVar)
        // and their solutions (b_room x B x nVar), made for the largest nrhs so far; the variable indices of objective 0's simple bounds (B x dims[0])
        // after a run that had them on the host (a device run left them in the group's d_rvar)
        double *d_bnd_rhs = NULL, *d_bnd_fixed = NULL, *d_bnd_x = NULL;
        uint32_t *d_bnd_var = NULL;
        uint32_t b_room = 0;
        ~Bufs()
        {
            void *dev[] = {d_map, d_out, d_types, d_meta, d_g, d_grad_rhs, d_grad_fixed, d_grad_lb, d_grad_ub, d_grad_lod, d_mat_out, d_lse_flag, d_mat_flag, d_shape,
                           d_tan_dlod, d_tan_dfixed, d_tan_dx, d_bnd_rhs, d_bnd_fixed, d_bnd_x, d_bnd_var};
            for (void *q : dev)
                if (q) (void)hipFree(q);
        }
    };
    std::vector<std::unique_ptr<Bufs>> bufs;
    // What a group's handle holds of the last run: final_kept — its final equality problems, formed and factorized with the factor kept
    // (ensure_final_factor; get_lambda and the gradient calls all start there, whichever comes first pays for it), final_any — some instance of the
    // group has an active constraint (else nothing was factorized), adj_uploaded — map, types and meta of that formation are on the device,
    // final_solved — the handle holds the x of that factor (solve_adjoint_matrix's chain needs it; the stage factorizes only).
    // Every new run drops all four (forget).
    std::vector<char> final_kept, final_any, adj_uploaded, final_solved;
    // lexls_lsi_batch_solve_bounds reads every row of every instance, not the working set alone: var_on_host — the last run's variable indices are in
    // ws_var (else, a device run: in the groups' d_rvar), var_uploaded — and on the device for this run; run_counts — the run had per-instance row
    // counts (lexls_lsi_batch_set_instance_obj_dims: the groups' d_inst_dims hold the copies it made); bounds_kernel — the variant of the last call
    std::atomic<bool> var_on_host{false};
    std::vector<char> var_uploaded;
    bool run_counts = false;
    const char *bounds_kernel = "";
    // lexls_lsi_batch_set_adjoint_regularized: solve_adjoint answers after a resident regularized run of type 1, 3, 4, 5, 8, 9 (constant factors); off:
    // the rules of get_lambda, as before.  adj_rc / adj_msg: what solve_adjoint answers after the last run (set_rule); final_reg: the run was such
    // a run, and ensure_final_factor leaves the run's regularization on the groups' handles
    // lexls_lsi_batch_set_adjoint_regularized_multi: the same for solve_adjoint_multi (adjm_rc / adjm_msg), independent of the first switch;
    // final_reg: either call is served after a regularized run
    bool adj_regularized = false, adj_regularized_multi = false, final_reg = false;
    int adj_rc = -1, adjm_rc = -1;
    std::string adj_msg, adjm_msg;
    uint32_t final_formations = 0; // since creation: how often ensure_final_factor formed and factorized a group's final problems (lexls_lsi_batch_final_factorizations)

    explicit LsiFinal(const LsiBatchShape &shape) : s(shape) {}
    /// once, when the batch's shape and its number of groups stand
    void create()
    {
        size_t elems = 0, rows = 0;
        for (uint32_t k = 0; k < s.nObj; k++)
        {
            data_off.push_back(static_cast<uint32_t>(elems));
            first.push_back(static_cast<uint32_t>(rows));
            elems += objective_elems(s.dims[k], s.types[k], s.nVar);
            rows += s.dims[k];
        }
        ws_na.assign((size_t)s.batch * s.nObj, 0);
        ws_idx.assign((size_t)s.batch * s.total, 0);
        ws_type.assign((size_t)s.batch * s.total, 0);
        ws_status.assign(s.batch, static_cast<int32_t>(TERMINATION_STATUS_UNKNOWN));
        if (s.off)
        {
            ws_fixvar.assign((size_t)s.batch * s.dims[0], 0);
            ws_fixval.assign((size_t)s.batch * s.dims[0], 0.0);
            ws_var.assign((size_t)s.batch * s.dims[0], 0);
        }
        final_kept.assign(s.nGroups, 0), final_any.assign(s.nGroups, 0), adj_uploaded.assign(s.nGroups, 0), final_solved.assign(s.nGroups, 0);
        var_uploaded.assign(s.nGroups, 0);
    }

    // ---- what the run calls ----
    /// nothing of the last run is valid any more: no rule, no factor in the groups' handles
    void forget()
    {
        lam_rc = -1;
        std::fill(final_kept.begin(), final_kept.end(), 0);
        std::fill(final_any.begin(), final_any.end(), 0);
        std::fill(adj_uploaded.begin(), adj_uploaded.end(), 0);
        std::fill(final_solved.begin(), final_solved.end(), 0);
        std::fill(var_uploaded.begin(), var_uploaded.end(), 0);
        var_on_host = false, run_counts = false;
    }
    /// a run starts
    void begin_run(const ParametersLexLSI &par)
    {
        forget();
        lam_tol = par.tol_linear_dependence;
    }
    /// some run has completed on this batch (and none has failed or started since)
    bool ran() const { return lam_rc >= 0; }

    /// instance b's final working set from its host objects (workingset.h order)
    template <class LSI>
    void keep_working_set(uint32_t b, const LSI &inst, const double *data, const uint32_t *var_index)
    {
        uint16_t *ix = &ws_idx[(size_t)b * s.total];
        uint8_t *ty  = &ws_type[(size_t)b * s.total];
        ws_status[b] = static_cast<int32_t>(inst.getStatus());
        for (uint32_t k = 0; k < s.nObj; k++) ws_na[(size_t)b * s.nObj + k] = static_cast<uint16_t>(inst.getObjectives()[k].getActiveCtrCount());
        walk_working_set(inst.getObjectives(), s.nObj, [&](uint32_t k, Index a, Index c, ConstraintActivationType t) { ix[first[k] + a] = static_cast<uint16_t>(c), ty[first[k] + a] = static_cast<uint8_t>(t); }, [](uint32_t, Index, Index) {});
        keep_fixed(b, data, var_index);
    }
    /// the same from the resident slabs a run downloaded (lists in working-set order, types by constraint)
    void keep_working_set_resident(uint32_t b, BatchCtx &ctx, uint32_t k, const double *data, const uint32_t *var_index)
    {
        const size_t total  = s.total;
        char *base          = ctx.rws_host.data();
        const uint8_t *cs   = ctx.rl.ctr_state(base, k);
        const uint16_t *act = ctx.rl.act(base, k), *na = ctx.rl.na(base, k);
        ws_status[b]        = ctx.rl.info(base, k)[0];
        for (uint32_t o = 0; o < s.nObj; o++)
        {
            ws_na[(size_t)b * s.nObj + o] = na[o];
            for (uint32_t a = 0; a < na[o]; a++)
            {
                ws_idx[(size_t)b * total + first[o] + a]  = act[first[o] + a];
                ws_type[(size_t)b * total + first[o] + a] = cs[first[o] + act[first[o] + a]];
            }
        }
        if (data)
            keep_fixed(b, data, var_index);
        else if (s.off && ctx.fix_var_host.n) // (a lexls_lsi_batch_run_device run: the scatter kernel read them from the resident data)
            for (uint32_t a = 0; a < na[0] && a < s.dims[0]; a++)
            {
                ws_fixvar[(size_t)b * s.dims[0] + a] = ctx.fix_var_host[(size_t)k * s.dims[0] + a];
                ws_fixval[(size_t)b * s.dims[0] + a] = ctx.fix_val_host[(size_t)k * s.dims[0] + a];
            }
    }
    /// fixVariable(var, bound) of formLexLSE for the active simple bounds (objective.h:257-271): lb, or ub for CTR_ACTIVE_UB / CTR_ACTIVE_EQ
    void keep_fixed(uint32_t b, const double *data, const uint32_t *var_index)
    {
        if (!s.off) return;
        const uint32_t d0 = s.dims[0], na = ws_na[(size_t)b * s.nObj];
        if (var_index)
        {
            std::copy(var_index, var_index + d0, ws_var.begin() + (size_t)b * d0);
            var_on_host = true;
        }
        for (uint32_t a = 0; a < na && a < d0; a++)
        {
            const uint32_t c = ws_idx[(size_t)b * s.total + a];
            ws_fixvar[(size_t)b * d0 + a] = var_index ? var_index[c] : 0u;
            ws_fixval[(size_t)b * d0 + a] = ws_type[(size_t)b * s.total + a] == CTR_ACTIVE_LB ? data[c] : data[d0 + c];
        }
    }

    /// what lexls_lsi_batch_get_lambda answers after a run with these parameters (LEXLS_OK: it is served)
    int lam_rc_after(const ParametersLexLSI &par) const
    {
        return (par.cycling_handling_enabled || par.regularization_type != REGULARIZATION_NONE || !s.gather || s.total > 65535) ? LEXLS_ERR_UNSUPPORTED : LEXLS_OK;
    }
    /// the fixed bounds of a device run are fetched for get_lambda and for the adjoint calls
    bool needs_final_problem(const ParametersLexLSI &par) const
    {
        const int t = static_cast<int>(par.regularization_type);
        return lam_rc_after(par) == LEXLS_OK || ((adj_regularized || adj_regularized_multi) && t != 0 && !par.cycling_handling_enabled && s.gather && s.total <= 65535);
    }
    /// The run is over and its working sets are kept: what get_lambda answers from now on (rc, and why not: msg), and what
    /// lexls_lsi_batch_solve_adjoint(_device) and lexls_lsi_batch_solve_adjoint_multi(_device) answer — the same, except that a regularized run is
    /// served when the batch asked for it for that call (adj_regularized, adj_regularized_multi), the run was resident (its regularization is on the
    /// groups' handles), its type is one of the six whose damped solve is affine in the bounds and its variable factor is zero
    /// counts: the run read per-instance row counts (a device run under lexls_lsi_batch_set_instance_obj_dims)
    void set_rule(int rc, const char *msg, const ParametersLexLSI &par, bool resident, bool counts = false)
    {
        lam_rc = rc, lam_msg = msg, run_counts = counts;
        adj_rc = adjm_rc = lam_rc, adj_msg = adjm_msg = lam_msg, final_reg = false;
        const int t = static_cast<int>(par.regularization_type);
        if (lam_rc != LEXLS_ERR_UNSUPPORTED || t == 0 || par.cycling_handling_enabled || !s.gather || s.total > 65535) return;
        auto rule = [&](bool on, const std::string &setter, const std::string &call, int &call_rc, std::string &call_msg) {
            const std::string who = call + ": ";
            if (!on)
                call_msg = lam_msg + " (" + setter + ", called before the run, lets " + call + " serve regularization types 1, 3, 4, 5, 8, 9)";
            else if (!resident)
                call_msg = who + "not available after a regularized run that was not resident on the device";
            else if (!(t == 1 || t == 3 || t == 4 || t == 5 || t == 8 || t == 9))
                call_msg = who + "not available after a regularized run of regularization_type " + std::to_string(t) + " (served: 1, 3, 4, 5, 8, 9)";
            else if (par.variable_regularization_factor != 0.0)
                call_msg = who + "not available after a regularized run with variable_regularization_factor != 0";
            else
                call_rc = LEXLS_OK, call_msg.clear(), final_reg = true;
        };
        rule(adj_regularized, "lexls_lsi_batch_set_adjoint_regularized", "lexls_lsi_batch_solve_adjoint", adj_rc, adj_msg);
        rule(adj_regularized_multi, "lexls_lsi_batch_set_adjoint_regularized_multi", "lexls_lsi_batch_solve_adjoint_multi", adjm_rc, adjm_msg);
    }

    // ---- the final equality problems ----
    /// instance k of group g: the in block of its final equality problem (lexls_lse_round_layout), as formLexLSE posts it (objective.h:255-294),
    /// and the user row of every active constraint
    void form_final_problem(uint32_t g, uint32_t k, Bufs &lb)
    {
        BatchCtx &ctx        = *s.grp[g];
        const uint32_t nObj = s.nObj, nVar = s.nVar, off = s.off;
        const size_t total   = s.total;
        const uint32_t nObjL = nObj - off, d0 = off ? s.dims[0] : 0u;
        const uint32_t b  = s.lo[g] + k;
        const uint16_t *na = ws_na.data() + (size_t)b * nObj;
        const uint16_t *ix = ws_idx.data() + (size_t)b * total;
        const uint8_t *ty  = ws_type.data() + (size_t)b * total;
        uint32_t *pos      = lb.map.data() + ctx.B + (size_t)k * total;
        uint32_t r = 0, row = 0;
        const uint32_t nf = off ? std::min<uint32_t>(na[0], nVar) : 0u; // (formLexLSE fixes each variable once: at most nVar, lexlse.h:1453)
        ctx.nfixed[k]     = nf;
        for (uint32_t a = 0; a < nf; a++)
        {
            ctx.fixed_idx[(size_t)k * nVar + a]  = ws_fixvar[(size_t)b * d0 + a];
            ctx.fixed_val[(size_t)k * nVar + a]  = ws_fixval[(size_t)b * d0 + a];
            ctx.fixed_type[(size_t)k * nVar + a] = ty[a];
            pos[r++]                             = ix[a];
        }
        std::fill(ctx.row_ld.begin() + (size_t)k * ctx.cap, ctx.row_ld.begin() + (size_t)(k + 1) * ctx.cap, 0u);
        for (uint32_t o = off; o < nObj; o++)
        {
            ctx.dims[(size_t)k * nObjL + (o - off)] = na[o];
            for (uint32_t a = 0; a < na[o]; a++)
            {
                const uint8_t t                      = ty[first[o] + a];
                ctx.row_src[(size_t)k * ctx.cap + row] = data_off[o] + ix[first[o] + a];
                ctx.row_ld[(size_t)k * ctx.cap + row]  = s.dims[o] | (t == CTR_ACTIVE_LB ? 0u : 0x80000000u);
                ctx.ctr_type[(size_t)k * ctx.cap + row] = t;
                row++;
                pos[r++] = first[o] + ix[first[o] + a];
            }
        }
        lb.map[k]     = r;
        ctx.skip[k]   = 0;
        ctx.objidx[k] = -1;
    }

    /// the groups' buffers of get_lambda, made at the first call that needs them
    void ensure_lambda_bufs()
    {
        if (!bufs.empty()) return;
        bufs.resize(s.nGroups);
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            bufs[g].reset(new Bufs());
            Bufs &lb        = *bufs[g];
            const size_t Bg = s.grp[g]->B, total = s.total;
            lb.map.assign(Bg + Bg * total, 0u);
            if (hipSetDevice(s.device) != hipSuccess || hipMalloc((void **)&lb.d_map, 4 * (Bg + Bg * total)) != hipSuccess ||
                hipMalloc((void **)&lb.d_out, 8 * Bg * total * s.nObj) != hipSuccess)
                throw Exception("hipMalloc failed (lexls_lsi_batch_get_lambda)");
        }
    }

    /// The final equality problems of group g's instances (the downloaded working sets of the last run, form_final_problem) formed, uploaded and
    /// factorized with the factor kept on a bit-exact kernel, in the group's stream — once per run: the handle then holds that factor until the
    /// next run (final_kept), and lb.map the rows' user positions.  -> some instance has an active constraint (else nothing is factorized).
    /// formed(): called between the host's formation and the device work (get_lambda's stage clock)
    template <class Formed>
    bool ensure_final_factor(uint32_t g, Formed formed)
    {
        if (final_kept[g]) return final_any[g] != 0;
        BatchCtx &ctx = *s.grp[g];
        Bufs &lb      = *bufs[g];
        s.pool->run(ctx.B, [&](uint32_t k) { form_final_problem(g, k, lb); });
        formed();
        bool any_active = false; // (a run whose mask skipped every instance of the group, or whose instances all ended with empty working sets)
        for (uint32_t k = 0; k < ctx.B && !any_active; k++) any_active = lb.map[k] != 0;
        // the equality solver's parameters of this run, whichever path it took (the one-by-one path of a non-resident deactivate_first_wrong_sign run never set
        // them on these handles; an earlier run of the batch object may have left a regularization there): lam_rc == LEXLS_OK means unregularized
        hip_check(lexls_lse_set_tolerance(ctx.h, lam_tol));
        // (final_reg: a resident regularized run whose adjoint is served — its type and factors, shared or per instance, host or device rows, are on the
        // handle since the run's upload_regularization_block and stay there: the final factor is the damped one)
        if (final_reg)
        {
            hip_check(lexls_lse_set_adjoint_regularized(ctx.h, adj_rc == LEXLS_OK));
            hip_check(lexls_lse_set_adjoint_regularized_multi(ctx.h, adjm_rc == LEXLS_OK));
        }
        else
            hip_check(lexls_lse_set_regularization(ctx.h, 0, NULL, 0, 0.0));
        const int policy = lexls_internal_kernel_policy(ctx.h);
        hip_check(lexls_lse_set_kernel_policy(ctx.h, 5)); // bit-exact kernels whatever the shape (the factor of the reference's getLambda)
        int rc = any_active ? lexls_internal_upload_round_trusted(ctx.h, ctx.in_block.data(), 1) : LEXLS_OK;
        if (rc == LEXLS_OK && any_active) rc = lexls_lse_factorize(ctx.h);
        hip_check(lexls_lse_set_kernel_policy(ctx.h, policy));
        hip_check(rc);
        final_kept[g] = 1, final_any[g] = any_active ? 1 : 0;
        final_formations++;
        return any_active;
    }

    // ---- getLambda ----
    /// lsi_lambda_scatter_kernel for group g, in its stream: the multipliers into the user's order, at `out` (the group's rows)
    void launch_lambda_scatter(uint32_t g, const double *d_mult, double *out, const uint32_t *d_fault, const uint8_t *mask)
    {
        BatchCtx &ctx = *s.grp[g];
        hipLaunchKernelGGL(lsi_lambda_scatter_kernel, dim3(ctx.B), dim3(64), 0, ctx.stream, d_mult, bufs[g]->d_map, ctx.B, (uint32_t)s.total, s.nObj, s.nObj - s.off, s.off,
                           s.nVar + ctx.cap, out, d_fault, mask);
        if (hipGetLastError() != hipSuccess) throw Exception("lsi_lambda_scatter_kernel launch failed");
    }
    /// lexls_lsi_batch_enqueue_device with d_lambda, behind group g's results: get_lambda(NULL, d_lambda) with the final problems formed where the working
    /// sets live (ensure_lambda_bufs has been called; nothing here waits or allocates)
    void enqueue_lambda(uint32_t g, int32_t max_fact, uint32_t *d_fault, double *d_lambda)
    {
        const double *d_mult = s.grp[g]->enqueue_lambda(max_fact, bufs[g]->d_map, d_fault, s.group_mask(g));
        launch_lambda_scatter(g, d_mult, d_lambda + (size_t)s.lo[g] * s.total * s.nObj, d_fault, s.group_mask(g));
    }

    /// LexLSI::getLambda (lexlsi.h:552-605) for every instance of the last run, on the device in each group's stream: the final equality
    /// problems are formed (rows gathered by reference, fixed variables posted), factorized with the factor kept on a bit-exact kernel, all
    /// objectives' multipliers taken in one sweep (lexls_lse_multipliers), scattered into the user's order, one copy back per group.
    /// d_lambda (lexls_lsi_batch_run_device_ex): memory of the batch's device instead — the scatter kernel writes there, nothing is copied back
    int get_lambda(double *h_lambda, double *d_lambda = NULL)
    {
        if (lam_rc < 0) throw Exception("lexls_lsi_batch_get_lambda: no completed lexls_lsi_batch_run on this batch");
        if (lam_rc != LEXLS_OK)
        {
            lexls_internal_set_error(lam_msg.c_str());
            return lam_rc;
        }
        if (!h_lambda && !d_lambda) throw Exception("lexls_lsi_batch_get_lambda: null output");
        const size_t total = s.total;
        ensure_lambda_bufs();
        // LEXLS_LSI_TIMING: the stages one by one (a synchronisation behind each) and their times on stderr
        const bool timing = RunSwitches().timing;
        double ts[4] = {0, 0, 0, 0}, tp = BatchCtx::now();
        auto stage = [&](int i, BatchCtx &c) {
            if (!timing) return;
            hip_check(lexls_lse_synchronize(c.h));
            const double t = BatchCtx::now();
            ts[i] += t - tp;
            tp = t;
        };
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            BatchCtx &ctx = *s.grp[g];
            Bufs &lb      = *bufs[g];
            const bool any_active = ensure_final_factor(g, [&]() { stage(0, ctx); });
            stage(1, ctx);
            if (any_active) hip_check(lexls_lse_multipliers(ctx.h));
            stage(2, ctx);
            // nobody has an active constraint: there is nothing to factorize and every row is zero — the scatter kernel reads no multiplier (nact = 0)
            const double *d_mult = any_active ? lexls_internal_multipliers(ctx.h, NULL) : lb.d_out;
            if (!d_mult) throw Exception("lexls_lsi_batch_get_lambda: no multipliers");
            if (hipMemcpyAsync(lb.d_map, lb.map.data(), 4 * ((size_t)ctx.B + (size_t)ctx.B * total), hipMemcpyHostToDevice, ctx.stream) != hipSuccess)
                throw Exception("hipMemcpyAsync failed (lexls_lsi_batch_get_lambda)");
            launch_lambda_scatter(g, d_mult, d_lambda ? d_lambda + (size_t)s.lo[g] * total * s.nObj : lb.d_out, NULL, d_lambda ? s.group_mask(g) : (const uint8_t *)NULL);
            if (!d_lambda && hipMemcpyAsync(h_lambda + (size_t)s.lo[g] * total * s.nObj, lb.d_out, 8 * (size_t)ctx.B * total * s.nObj, hipMemcpyDeviceToHost, ctx.stream) != hipSuccess)
                throw Exception("hipMemcpyAsync failed (lexls_lsi_batch_get_lambda)");
            stage(3, ctx);
        }
        for (uint32_t g = 0; g < s.nGroups; g++)
            if (hipStreamSynchronize(s.grp[g]->stream) != hipSuccess) throw Exception("lexls_lsi_batch_get_lambda: stream synchronisation failed");
        if (timing)
            std::fprintf(stderr, "lexls_lsi_batch_get_lambda: %.4f ms = form the problems (host) %.4f + upload, gather, factorize %.4f + multipliers %.4f + scatter, copy back %.4f (%u groups)\n",
                         1e3 * (ts[0] + ts[1] + ts[2] + ts[3]), 1e3 * ts[0], 1e3 * ts[1], 1e3 * ts[2], 1e3 * ts[3], s.nGroups);
        return LEXLS_OK;
    }

    // ---- the gradient calls ----
    /// The groups' buffers of the gradient calls: the routes of the scatter kernels at the first call, and room for ncot cotangents per instance — made for
    /// the largest ncot so far (a single call after a multi call works in the larger set).  call: the one named when an allocation fails
    void ensure_adjoint_bufs(uint32_t ncot, const char *call)
    {
        ensure_lambda_bufs();
        if (!bufs[0]->d_meta && hipSetDevice(s.device) != hipSuccess) throw Exception("hipSetDevice failed (lexls_lsi_batch_solve_adjoint)");
        const size_t total = s.total, nVar = s.nVar;
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            Bufs &lb        = *bufs[g];
            const size_t Bg = s.grp[g]->B, cap = s.grp[g]->cap, rows = Bg * ncot;
            if (!lb.d_meta)
            {
                lb.types.assign(Bg * total, 0);
                lb.meta.assign(2 * Bg, 0);
                if (hipMalloc((void **)&lb.d_types, Bg * total ? Bg * total : 1) != hipSuccess ||
                    hipMalloc((void **)&lb.d_meta, 8 * Bg) != hipSuccess) // (last: its presence says that the other one is there)
                    throw Exception("hipMalloc failed (lexls_lsi_batch_solve_adjoint)");
            }
            if (ncot <= lb.m_room) continue;
            lb.m_room = 0;
            for (double **q : {&lb.d_g, &lb.d_grad_rhs, &lb.d_grad_fixed, &lb.d_grad_lb, &lb.d_grad_ub})
            {
                if (*q) (void)hipFree(*q);
                *q = NULL;
            }
            if (hipMalloc((void **)&lb.d_g, 8 * rows * nVar) != hipSuccess || hipMalloc((void **)&lb.d_grad_rhs, 8 * rows * (cap ? cap : 1)) != hipSuccess ||
                hipMalloc((void **)&lb.d_grad_fixed, 8 * rows * nVar) != hipSuccess || hipMalloc((void **)&lb.d_grad_lb, 8 * rows * (total ? total : 1)) != hipSuccess ||
                hipMalloc((void **)&lb.d_grad_ub, 8 * rows * (total ? total : 1)) != hipSuccess)
                throw Exception(std::string("hipMalloc failed (") + call + ")");
            lb.m_room = ncot;
        }
    }

    /// what the scatter kernels read next to the map, for instance k of group g: the activation type of every row of its final problem in
    /// form_final_problem's row order, its status of the run and its number of fixed variables
    void form_adjoint_routes(uint32_t g, uint32_t k, Bufs &lb)
    {
        const uint32_t b   = s.lo[g] + k;
        const uint16_t *na = ws_na.data() + (size_t)b * s.nObj;
        const uint8_t *ty  = ws_type.data() + (size_t)b * s.total;
        uint8_t *out       = lb.types.data() + (size_t)k * s.total;
        const uint32_t nf  = s.off ? std::min<uint32_t>(na[0], s.nVar) : 0u;
        uint32_t r         = 0;
        for (uint32_t a = 0; a < nf; a++) out[r++] = ty[a];
        for (uint32_t o = s.off; o < s.nObj; o++)
            for (uint32_t a = 0; a < na[o]; a++) out[r++] = ty[first[o] + a];
        lb.meta[2 * k]     = ws_status[b];
        lb.meta[2 * k + 1] = static_cast<int32_t>(nf);
    }

    /// the routes of the scatter kernels (map, types, meta: form_final_problem's and form_adjoint_routes') on the device, in the group's stream —
    /// once per run, whichever gradient call comes first (behind ensure_final_factor, which forms the map)
    void upload_adjoint_routes(uint32_t g, const char *who)
    {
        if (adj_uploaded[g]) return;
        BatchCtx &ctx     = *s.grp[g];
        Bufs &lb          = *bufs[g];
        const size_t rows = (size_t)ctx.B * s.total;
        s.pool->run(ctx.B, [&](uint32_t k) { form_adjoint_routes(g, k, lb); });
        if (hipMemcpyAsync(lb.d_map, lb.map.data(), 4 * ((size_t)ctx.B + rows), hipMemcpyHostToDevice, ctx.stream) != hipSuccess ||
            hipMemcpyAsync(lb.d_types, lb.types.data(), rows, hipMemcpyHostToDevice, ctx.stream) != hipSuccess ||
            hipMemcpyAsync(lb.d_meta, lb.meta.data(), 8 * (size_t)ctx.B, hipMemcpyHostToDevice, ctx.stream) != hipSuccess)
            throw Exception(std::string(who) + ": hipMemcpyAsync failed (row map)");
        adj_uploaded[g] = 1;
    }

    /// What one gradient call hands to gradient(), next to its three pieces of code
    struct GradientForm
    {
        const char *who, *g_name;  // the entry point and its name of g, for the exception texts
        int rc;                    // the rule of the last run for this call, and why not
        const std::string &msg;
        uint32_t ncot;             // cotangents per instance
        size_t g_bytes;            // of g, per instance
        size_t out_bytes[2];       // of each of the two outputs, per instance
        bool wants_x;              // the equality solver's call needs the x of the final factor: lexls_lse_solve, once per run (final_solved)
    };
    /// The one skeleton of the gradient calls, d loss / d (something of the problems) of the last run from g = d loss / d x.  Per group, in its stream: the
    /// final equality problems factorized with the factor kept (ensure_final_factor: get_lambda's stage, shared with it and among the gradient calls —
    /// nothing is factorized twice), the routes of the scatter (once per run), adjoint(ctx, lb, d_g): the equality solver's call on the group's rows of g,
    /// into the group's buffers; scatter(g, any_active, d_out): the launch that takes its results to the caller's order.
    /// on_device: g and the outputs are memory of the batch's device (nothing of them passes through the host); else the host's, staged in the group's
    /// d_g and in staging(lb)'s two buffers.  out[i] == NULL: that output is not asked for.  Waits for the groups' streams before it returns.
    template <class Ensure, class Staging, class Adjoint, class Scatter>
    int gradient(const GradientForm &f, const void *g_in, void *const (&out)[2], bool on_device, Ensure ensure, Staging staging, Adjoint adjoint, Scatter scatter)
    {
        const std::string who = f.who;
        if (lam_rc < 0) throw Exception(who + ": no completed lexls_lsi_batch_run on this batch");
        if (f.rc != LEXLS_OK)
        {
            lexls_internal_set_error(f.msg.c_str());
            return f.rc;
        }
        if (f.ncot > 65535u) throw Exception(who + ": more than 65535 cotangents per instance");
        if (hipSetDevice(s.device) != hipSuccess) throw Exception(who + ": hipSetDevice failed");
        ensure();
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            BatchCtx &ctx         = *s.grp[g];
            Bufs &lb              = *bufs[g];
            const bool any_active = ensure_final_factor(g, []() {});
            upload_adjoint_routes(g, f.who);
            if (f.wants_x && any_active && !final_solved[g])
            {
                hip_check(lexls_lse_solve(ctx.h)); // the stage factorizes only: the chain wants the x of this factor
                final_solved[g] = 1;
            }
            const void *d_g = static_cast<const char *>(g_in) + (size_t)s.lo[g] * f.g_bytes;
            void *user[2], *d_out[2];
            for (int i = 0; i < 2; i++) user[i] = d_out[i] = out[i] ? static_cast<char *>(out[i]) + (size_t)s.lo[g] * f.out_bytes[i] : NULL;
            if (!on_device)
            {
                const std::array<void *, 2> stage = staging(lb);
                // with an instance mask the entries of a skipped instance keep the caller's bits: they travel to the staging buffers first
                bool ok = hipMemcpyAsync(lb.d_g, d_g, ctx.B * f.g_bytes, hipMemcpyHostToDevice, ctx.stream) == hipSuccess;
                for (int i = 0; i < 2 && ok; i++)
                    ok = !(s.group_mask(g) && user[i]) || hipMemcpyAsync(stage[i], user[i], ctx.B * f.out_bytes[i], hipMemcpyHostToDevice, ctx.stream) == hipSuccess;
                if (!ok) throw Exception(who + ": hipMemcpyAsync failed (" + f.g_name + ")");
                d_g = lb.d_g;
                for (int i = 0; i < 2; i++) d_out[i] = user[i] ? stage[i] : NULL;
            }
            // nobody has an active constraint: nothing was factorized, every entry is zero (and every solved instance differentiable) — the scatter
            // kernel reads no gradient (nact = 0) and no flag of the equality solver
            if (any_active) hip_check(adjoint(ctx, lb, static_cast<const double *>(d_g)));
            scatter(g, any_active, d_out);
            for (int i = 0; i < 2 && !on_device; i++)
                if (user[i] && hipMemcpyAsync(user[i], d_out[i], ctx.B * f.out_bytes[i], hipMemcpyDeviceToHost, ctx.stream) != hipSuccess)
                    throw Exception(who + ": hipMemcpyAsync failed (results)");
        }
        for (uint32_t g = 0; g < s.nGroups; g++)
            if (hipStreamSynchronize(s.grp[g]->stream) != hipSuccess) throw Exception(who + ": stream synchronisation failed");
        return LEXLS_OK;
    }

    /// solve_adjoint and solve_adjoint_multi: d loss / d lb and d loss / d ub for ncot cotangents per instance — G batch x ncot x nVar, the outputs
    /// batch x ncot x total, either may be NULL.  `single`: the call of one cotangent — its own rule of set_rule (adj_rc), and
    /// lexls_lse_solve_adjoint_device; else the multi call's rule (adjm_rc) and lexls_lse_solve_adjoint_multi_device.  lsi_adjoint_scatter_multi_kernel serves both.
    int bounds_gradient(const char *who, bool single, const double *G_in, uint32_t ncot, double *grad_lb, double *grad_ub, bool on_device)
    {
        const size_t total = s.total;
        const GradientForm f = {who, single ? "g" : "G", single ? adj_rc : adjm_rc, single ? adj_msg : adjm_msg, ncot, 8 * (size_t)ncot * s.nVar, {8 * (size_t)ncot * total, 8 * (size_t)ncot * total}, false};
        void *const out[2]   = {grad_lb, grad_ub};
        return gradient(
            f, G_in, out, on_device, [&]() { ensure_adjoint_bufs(ncot, single ? "lexls_lsi_batch_solve_adjoint" : "lexls_lsi_batch_solve_adjoint_multi"); },
            [](Bufs &lb) { return std::array<void *, 2>{lb.d_grad_lb, lb.d_grad_ub}; },
            [&](BatchCtx &ctx, Bufs &lb, const double *d_G) {
                return single ? lexls_lse_solve_adjoint_device(ctx.h, d_G, lb.d_grad_rhs, lb.d_grad_fixed) : lexls_lse_solve_adjoint_multi_device(ctx.h, d_G, ncot, lb.d_grad_rhs, lb.d_grad_fixed);
            },
            [&](uint32_t g, bool, void *const d_out[2]) {
                BatchCtx &ctx = *s.grp[g];
                Bufs &lb      = *bufs[g];
                hipLaunchKernelGGL(lsi_adjoint_scatter_multi_kernel, dim3(ctx.B, ncot), dim3(64), 0, ctx.stream, lb.d_grad_rhs, lb.d_grad_fixed, lb.d_map, lb.d_types, lb.d_meta,
                                   ctx.B, ncot, (uint32_t)total, s.nVar, ctx.cap, static_cast<double *>(d_out[0]), static_cast<double *>(d_out[1]), s.group_mask(g));
                if (hipGetLastError() != hipSuccess) throw Exception("lsi_adjoint_scatter_multi_kernel launch failed");
            });
    }
    /// lexls_lsi_batch_solve_adjoint(_device): one cotangent per instance, g batch x nVar
    int solve_adjoint(const double *g_in, double *grad_lb, double *grad_ub, bool on_device)
    {
        return bounds_gradient(on_device ? "lexls_lsi_batch_solve_adjoint_device" : "lexls_lsi_batch_solve_adjoint", true, g_in, 1, grad_lb, grad_ub, on_device);
    }
    /// lexls_lsi_batch_solve_adjoint_multi(_device)
    int solve_adjoint_multi(const double *G_in, uint32_t ncot, double *grad_lb, double *grad_ub, bool on_device)
    {
        return bounds_gradient(on_device ? "lexls_lsi_batch_solve_adjoint_multi_device" : "lexls_lsi_batch_solve_adjoint_multi", false, G_in, ncot, grad_lb, grad_ub, on_device);
    }

    /// the groups' buffers of solve_adjoint_matrix, made at the first call; host_form: also the staging buffers of a host caller
    void ensure_adjoint_matrix_bufs(bool host_form)
    {
        ensure_adjoint_bufs(1, "lexls_lsi_batch_solve_adjoint");
        const uint32_t nObj = s.nObj;
        std::vector<uint32_t> shape(4 * (size_t)nObj);
        for (uint32_t k = 0; k < nObj; k++) shape[4 * k] = s.dims[k], shape[4 * k + 1] = s.types[k] == 1 ? 0u : 1u, shape[4 * k + 2] = data_off[k], shape[4 * k + 3] = first[k];
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            Bufs &lb        = *bufs[g];
            const size_t Bg = s.grp[g]->B, cap = s.grp[g]->cap;
            if (!lb.d_shape)
            {
                if (hipMalloc((void **)&lb.d_grad_lod, 8 * Bg * (s.nVar + 1) * (cap ? cap : 1)) != hipSuccess || hipMalloc((void **)&lb.d_lse_flag, Bg) != hipSuccess ||
                    hipMalloc((void **)&lb.d_shape, 16 * (size_t)nObj) != hipSuccess) // (last: its presence says that the others are there)
                    throw Exception("hipMalloc failed (lexls_lsi_batch_solve_adjoint_matrix)");
                if (hipMemcpy(lb.d_shape, shape.data(), 16 * (size_t)nObj, hipMemcpyHostToDevice) != hipSuccess)
                    throw Exception("hipMemcpy failed (lexls_lsi_batch_solve_adjoint_matrix)");
            }
            if (host_form && !lb.d_mat_flag &&
                (hipMalloc((void **)&lb.d_mat_out, 8 * Bg * (s.per_data ? s.per_data : 1)) != hipSuccess || hipMalloc((void **)&lb.d_mat_flag, Bg) != hipSuccess))
                throw Exception("hipMalloc failed (lexls_lsi_batch_solve_adjoint_matrix)");
        }
    }

    /// lexls_lsi_batch_solve_adjoint_matrix(_device): d loss / d (constraint data) of the last run from g = d loss / d x, in the layout
    /// lexls_lsi_batch_run_device reads, and the instances' differentiable flags (may be NULL).  The equality solver's call is its matrix chain on the
    /// x of the final factor (grad_lod, N^T g from the chain's own solve_adjoint launch, the rank-stability flags); lsi_adjoint_matrix_scatter_kernel
    /// takes them to the caller's layout — with a NULL lse_flag where the group launched no chain.
    int solve_adjoint_matrix(const double *g_in, double *grad_data, uint8_t *differentiable, bool on_device)
    {
        const GradientForm f = {on_device ? "lexls_lsi_batch_solve_adjoint_matrix_device" : "lexls_lsi_batch_solve_adjoint_matrix", "g", lam_rc, lam_msg, 1, 8 * (size_t)s.nVar, {8 * s.per_data, 1}, true};
        void *const out[2]   = {grad_data, differentiable};
        return gradient(
            f, g_in, out, on_device, [&]() { ensure_adjoint_matrix_bufs(!on_device); }, [](Bufs &lb) { return std::array<void *, 2>{lb.d_mat_out, lb.d_mat_flag}; },
            [](BatchCtx &ctx, Bufs &lb, const double *d_g) { return lexls_internal_solve_adjoint_matrix(ctx.h, d_g, lb.d_grad_lod, lb.d_grad_fixed, lb.d_lse_flag); },
            [&](uint32_t g, bool any_active, void *const d_out[2]) {
                BatchCtx &ctx = *s.grp[g];
                Bufs &lb      = *bufs[g];
                hipLaunchKernelGGL(lsi_adjoint_matrix_scatter_kernel, dim3(ctx.B), dim3(ADJM_NT), 0, ctx.stream, lb.d_grad_lod, lb.d_grad_fixed,
                                   any_active ? lb.d_lse_flag : (const uint8_t *)NULL, lb.d_map, lb.d_types, lb.d_meta, lb.d_shape, ctx.B, s.nObj, (uint32_t)s.total, s.nVar, ctx.cap,
                                   s.per_data, static_cast<double *>(d_out[0]), static_cast<uint8_t *>(d_out[1]), s.group_mask(g));
                if (hipGetLastError() != hipSuccess) throw Exception("lsi_adjoint_matrix_scatter_kernel launch failed");
            });
    }
    // ---- forward mode ----
    /// the groups' buffers of solve_tangent (behind those of solve_adjoint_matrix: the routes, the shape, the equality solver's flags), for the largest
    /// ntan so far
    void ensure_tangent_bufs(uint32_t ntan)
    {
        ensure_adjoint_matrix_bufs(false);
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            Bufs &lb = *bufs[g];
            if (ntan <= lb.t_room) continue;
            const size_t Bg = s.grp[g]->B, cap = s.grp[g]->cap, rows = Bg * ntan;
            lb.t_room = 0;
            for (double **q : {&lb.d_tan_dlod, &lb.d_tan_dfixed, &lb.d_tan_dx})
            {
                if (*q) (void)hipFree(*q);
                *q = NULL;
            }
            if (hipMalloc((void **)&lb.d_tan_dlod, 8 * rows * (s.nVar + 1) * (cap ? cap : 1)) != hipSuccess || hipMalloc((void **)&lb.d_tan_dfixed, 8 * rows * s.nVar) != hipSuccess ||
                hipMalloc((void **)&lb.d_tan_dx, 8 * rows * s.nVar) != hipSuccess)
                throw Exception("hipMalloc failed (lexls_lsi_batch_solve_tangent)");
            lb.t_room = ntan;
        }
    }
    /// a host caller's directions, tangents and flags on the device (made for the largest request so far)
    struct TangentStage
    {
        double *d_ddata = NULL, *d_dx = NULL;
        uint8_t *d_flag = NULL;
        size_t ddata_bytes = 0, dx_bytes = 0;
        ~TangentStage()
        {
            for (void *q : {(void *)d_ddata, (void *)d_dx, (void *)d_flag})
                if (q) (void)hipFree(q);
        }
    } tan_stage;

    /// lexls_lsi_batch_solve_tangent(_device): how x of the last run moves along ntan directions of the constraint data per instance (ddata: ntan x
    /// batch x per_data, the layout lexls_lsi_batch_run_device reads; dx: ntan x batch x nVar; differentiable: batch bytes, may be NULL), while the
    /// working set holds: the tangent of the final equality problem.  Per group, in its stream: the final factor (ensure_final_factor, shared with
    /// get_lambda and every adjoint call: nothing is factorized twice), its x and the routes once per run, lsi_tangent_gather_kernel,
    /// lexls_lse_solve_tangent_device, lsi_tangent_finish_kernel.  The rule of the last run is solve_adjoint_matrix's (lam_rc).  The host form stages in
    /// buffers of the batch (under a mask the caller's dx and flags travel there first).  Waits for the groups' streams before it returns.
    int solve_tangent(const double *ddata, uint32_t ntan, double *dx, uint8_t *differentiable, bool on_device)
    {
        const std::string who = on_device ? "lexls_lsi_batch_solve_tangent_device" : "lexls_lsi_batch_solve_tangent";
        if (lam_rc < 0) throw Exception(who + ": no completed lexls_lsi_batch_run on this batch");
        if (lam_rc != LEXLS_OK)
        {
            lexls_internal_set_error(lam_msg.c_str());
            return lam_rc;
        }
        if (ntan > 65535u) throw Exception(who + ": more than 65535 directions per instance");
        if (hipSetDevice(s.device) != hipSuccess) throw Exception(who + ": hipSetDevice failed");
        ensure_tangent_bufs(ntan);
        const size_t in_bytes = 8 * (size_t)ntan * s.batch * s.per_data, out_bytes = 8 * (size_t)ntan * s.batch * s.nVar;
        const double *d_ddata = ddata;
        double *d_dx          = dx;
        uint8_t *d_flag       = differentiable;
        if (!on_device)
        {
            TangentStage &st = tan_stage;
            if (in_bytes > st.ddata_bytes)
            {
                if (st.d_ddata) (void)hipFree(st.d_ddata);
                st.d_ddata = NULL, st.ddata_bytes = 0;
                if (hipMalloc((void **)&st.d_ddata, in_bytes ? in_bytes : 8) != hipSuccess) throw Exception(who + ": hipMalloc failed");
                st.ddata_bytes = in_bytes;
            }
            if (out_bytes > st.dx_bytes)
            {
                if (st.d_dx) (void)hipFree(st.d_dx);
                st.d_dx = NULL, st.dx_bytes = 0;
                if (hipMalloc((void **)&st.d_dx, out_bytes) != hipSuccess) throw Exception(who + ": hipMalloc failed");
                st.dx_bytes = out_bytes;
            }
            if (!st.d_flag && hipMalloc((void **)&st.d_flag, s.batch) != hipSuccess) throw Exception(who + ": hipMalloc failed");
            bool ok = hipMemcpy(st.d_ddata, ddata, in_bytes, hipMemcpyHostToDevice) == hipSuccess;
            if (ok && s.d_mask) ok = hipMemcpy(st.d_dx, dx, out_bytes, hipMemcpyHostToDevice) == hipSuccess; // a skipped instance keeps the caller's bits
            if (ok && s.d_mask && differentiable) ok = hipMemcpy(st.d_flag, differentiable, s.batch, hipMemcpyHostToDevice) == hipSuccess;
            if (!ok) throw Exception(who + ": hipMemcpy failed (ddata)");
            d_ddata = st.d_ddata, d_dx = st.d_dx, d_flag = differentiable ? st.d_flag : NULL;
        }
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            BatchCtx &ctx         = *s.grp[g];
            Bufs &lb              = *bufs[g];
            const bool any_active = ensure_final_factor(g, []() {});
            upload_adjoint_routes(g, who.c_str());
            if (any_active && !final_solved[g])
            {
                hip_check(lexls_lse_solve(ctx.h)); // the stage factorizes only: the chain wants the x of this factor
                final_solved[g] = 1;
            }
            // nobody has an active constraint: nothing was factorized, every tangent is zero (and every solved instance differentiable)
            if (any_active)
            {
                hipLaunchKernelGGL(lsi_tangent_gather_kernel, dim3(ctx.B, ntan), dim3(ADJM_NT), 0, ctx.stream, d_ddata, lb.d_map, lb.d_types, lb.d_meta, lb.d_shape, ctx.B, s.batch,
                                   s.lo[g], ntan, s.nObj, (uint32_t)s.total, s.nVar, ctx.cap, s.per_data, lb.d_tan_dlod, lb.d_tan_dfixed, s.group_mask(g));
                if (hipGetLastError() != hipSuccess) throw Exception("lsi_tangent_gather_kernel launch failed");
                hip_check(lexls_lse_solve_tangent_device(ctx.h, lb.d_tan_dlod, lb.d_tan_dfixed, ntan, lb.d_tan_dx, lb.d_lse_flag));
            }
            hipLaunchKernelGGL(lsi_tangent_finish_kernel, dim3(ctx.B, ntan), dim3(64), 0, ctx.stream, any_active ? lb.d_tan_dx : (const double *)NULL,
                               any_active ? lb.d_lse_flag : (const uint8_t *)NULL, lb.d_map, lb.d_meta, ctx.B, s.batch, s.lo[g], ntan, (uint32_t)s.total, s.nVar, ctx.cap, d_dx,
                               d_flag ? d_flag + s.lo[g] : (uint8_t *)NULL, s.group_mask(g));
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_tangent_finish_kernel launch failed");
        }
        for (uint32_t g = 0; g < s.nGroups; g++)
            if (hipStreamSynchronize(s.grp[g]->stream) != hipSuccess) throw Exception(who + ": stream synchronisation failed");
        if (!on_device)
        {
            bool ok = hipMemcpy(dx, d_dx, out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && differentiable) ok = hipMemcpy(differentiable, d_flag, s.batch, hipMemcpyDeviceToHost) == hipSuccess;
            if (!ok) throw Exception(who + ": hipMemcpy failed (results)");
        }
        return LEXLS_OK;
    }

    // ---- new bounds on the final working set ----
    /// the groups' buffers of solve_bounds (behind those of solve_adjoint_matrix: the routes and the shape), for the largest nrhs so far
    void ensure_bounds_bufs(uint32_t nrhs)
    {
        ensure_adjoint_matrix_bufs(false);
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            Bufs &lb        = *bufs[g];
            const size_t Bg = s.grp[g]->B, cap = s.grp[g]->cap, rows = Bg * nrhs;
            if (s.off && !lb.d_bnd_var && hipMalloc((void **)&lb.d_bnd_var, 4 * Bg * (s.dims[0] ? s.dims[0] : 1)) != hipSuccess)
                throw Exception("hipMalloc failed (lexls_lsi_batch_solve_bounds)");
            if (nrhs <= lb.b_room) continue;
            lb.b_room = 0;
            for (double **q : {&lb.d_bnd_rhs, &lb.d_bnd_fixed, &lb.d_bnd_x})
            {
                if (*q) (void)hipFree(*q);
                *q = NULL;
            }
            if (hipMalloc((void **)&lb.d_bnd_rhs, 8 * rows * (cap ? cap : 1)) != hipSuccess || hipMalloc((void **)&lb.d_bnd_fixed, 8 * rows * s.nVar) != hipSuccess ||
                hipMalloc((void **)&lb.d_bnd_x, 8 * rows * s.nVar) != hipSuccess)
                throw Exception("hipMalloc failed (lexls_lsi_batch_solve_bounds)");
            lb.b_room = nrhs;
        }
    }
    /// a host caller's bounds, solutions, violations and flags on the device (made for the largest request so far)
    struct BoundsStage
    {
        double *d_lb = NULL, *d_ub = NULL, *d_x = NULL, *d_viol = NULL, *d_cost = NULL; // (d_cost: made by the first lexls_lsi_batch_solve_bounds_cost)
        uint8_t *d_valid = NULL;
        uint32_t room = 0, cost_room = 0;
        void release()
        {
            for (void *q : {(void *)d_lb, (void *)d_ub, (void *)d_x, (void *)d_viol, (void *)d_cost})
                if (q) (void)hipFree(q);
            d_lb = d_ub = d_x = d_viol = d_cost = NULL, room = cost_room = 0;
        }
        ~BoundsStage()
        {
            release();
            if (d_valid) (void)hipFree(d_valid);
        }
    } bnd_stage;

    /// lexls_lsi_batch_solve_bounds(_device): x of the last run's final working sets under nrhs other bound sets per instance (lb, ub: nrhs x batch x
    /// total, user's constraint order; x: nrhs x batch x nVar), how far each answer breaks the instance's bounds (violation: nrhs x batch, may be NULL)
    /// and which instances ended PROBLEM_SOLVED (valid: batch bytes, may be NULL).  Per group, in its stream: the final factor (ensure_final_factor,
    /// shared with get_lambda and every gradient call: nothing is factorized twice) and the routes once per run, lsi_bounds_gather_kernel,
    /// lexls_lse_solve_rhs_device, lsi_bounds_check_kernel on the constraint data resident in the group's handle.  The rule of the last run is
    /// solve_tangent's (lam_rc).  The host form stages in buffers of the batch (under a mask the caller's outputs travel there first).  Waits for the
    /// groups' streams before it returns.
    /// with_cost (lexls_lsi_batch_solve_bounds_cost(_device)): besides, cost (nrhs x batch x nObj) = every objective's squared distance from bound set
    /// c at x[c, i], from lsi_bounds_check_kernel<placement, true>; x may be NULL then.  Without it: exactly the launches of before.
    int solve_bounds(const double *lbq, const double *ubq, uint32_t nrhs, double *x, double *violation, uint8_t *valid, bool on_device, bool with_cost = false,
                     double *cost = NULL)
    {
        const std::string who = std::string("lexls_lsi_batch_solve_bounds") + (with_cost ? "_cost" : "") + (on_device ? "_device" : "");
        if (lam_rc < 0) throw Exception(who + ": no completed lexls_lsi_batch_run on this batch");
        if (lam_rc != LEXLS_OK)
        {
            lexls_internal_set_error(lam_msg.c_str());
            return lam_rc;
        }
        if (hipSetDevice(s.device) != hipSuccess) throw Exception(who + ": hipSetDevice failed");
        ensure_bounds_bufs(nrhs);
        const size_t total = s.total, in_bytes = 8 * (size_t)nrhs * s.batch * total, x_bytes = 8 * (size_t)nrhs * s.batch * s.nVar, v_bytes = 8 * (size_t)nrhs * s.batch;
        const size_t c_bytes = 8 * (size_t)nrhs * s.batch * s.nObj;
        const double *d_lbq = lbq, *d_ubq = ubq;
        double *d_x = x, *d_viol = violation, *d_cost = cost;
        uint8_t *d_valid = valid;
        if (!on_device)
        {
            BoundsStage &st = bnd_stage;
            if (nrhs > st.room)
            {
                st.release();
                if (hipMalloc((void **)&st.d_lb, in_bytes ? in_bytes : 8) != hipSuccess || hipMalloc((void **)&st.d_ub, in_bytes ? in_bytes : 8) != hipSuccess ||
                    hipMalloc((void **)&st.d_x, x_bytes) != hipSuccess || hipMalloc((void **)&st.d_viol, v_bytes) != hipSuccess)
                    throw Exception(who + ": hipMalloc failed");
                st.room = nrhs;
            }
            if (!st.d_valid && hipMalloc((void **)&st.d_valid, s.batch) != hipSuccess) throw Exception(who + ": hipMalloc failed");
            if (with_cost && nrhs > st.cost_room)
            {
                if (st.d_cost) (void)hipFree(st.d_cost);
                st.d_cost = NULL, st.cost_room = 0;
                if (hipMalloc((void **)&st.d_cost, c_bytes) != hipSuccess) throw Exception(who + ": hipMalloc failed");
                st.cost_room = nrhs;
            }
            bool ok = hipMemcpy(st.d_lb, lbq, in_bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(st.d_ub, ubq, in_bytes, hipMemcpyHostToDevice) == hipSuccess;
            if (ok && s.d_mask && x) ok = hipMemcpy(st.d_x, x, x_bytes, hipMemcpyHostToDevice) == hipSuccess; // a skipped instance keeps the caller's bits
            if (ok && s.d_mask && with_cost) ok = hipMemcpy(st.d_cost, cost, c_bytes, hipMemcpyHostToDevice) == hipSuccess;
            if (ok && s.d_mask && violation) ok = hipMemcpy(st.d_viol, violation, v_bytes, hipMemcpyHostToDevice) == hipSuccess;
            if (ok && s.d_mask && valid) ok = hipMemcpy(st.d_valid, valid, s.batch, hipMemcpyHostToDevice) == hipSuccess;
            if (!ok) throw Exception(who + ": hipMemcpy failed (bounds)");
            d_lbq = st.d_lb, d_ubq = st.d_ub, d_x = x ? st.d_x : NULL, d_viol = violation ? st.d_viol : NULL, d_valid = valid ? st.d_valid : NULL;
            d_cost = with_cost ? st.d_cost : NULL;
        }
        const lexls::BoundsCheckPlacement place = lexls::bounds_check_placement(s.nVar);
        const size_t lds                        = lexls::bounds_check_lds_bytes(s.nVar, place);
        const uint32_t tiles                    = (nrhs + 63) / 64;
        for (uint32_t g = 0; g < s.nGroups; g++)
        {
            BatchCtx &ctx         = *s.grp[g];
            Bufs &lb              = *bufs[g];
            const bool any_active = ensure_final_factor(g, []() {});
            upload_adjoint_routes(g, who.c_str());
            const uint32_t *d_var = NULL; // the variables of objective 0's simple bounds, every row's
            if (s.off)
            {
                if (var_on_host && !var_uploaded[g])
                {
                    if (hipMemcpyAsync(lb.d_bnd_var, ws_var.data() + (size_t)s.lo[g] * s.dims[0], 4 * (size_t)ctx.B * s.dims[0], hipMemcpyHostToDevice, ctx.stream) != hipSuccess)
                        throw Exception(who + ": hipMemcpyAsync failed (variable indices)");
                    var_uploaded[g] = 1;
                }
                d_var = var_on_host ? lb.d_bnd_var : ctx.d_rvar;
            }
            // nobody has an active constraint: nothing was factorized, every x is zero
            if (any_active)
            {
                hipLaunchKernelGGL(lsi_bounds_gather_kernel, dim3(ctx.B, nrhs), dim3(64), 0, ctx.stream, d_lbq, d_ubq, lb.d_map, lb.d_types, lb.d_meta, ctx.B, s.batch, s.lo[g], nrhs,
                                   (uint32_t)total, s.nVar, ctx.cap, lb.d_bnd_rhs, lb.d_bnd_fixed, s.group_mask(g));
                if (hipGetLastError() != hipSuccess) throw Exception("lsi_bounds_gather_kernel launch failed");
                hip_check(lexls_lse_solve_rhs_device(ctx.h, lb.d_bnd_rhs, lb.d_bnd_fixed, nrhs, lb.d_bnd_x));
            }
            const double *x_lse    = any_active ? lb.d_bnd_x : (const double *)NULL;
            const uint32_t *counts = run_counts ? ctx.d_inst_dims : (const uint32_t *)NULL;
            uint8_t *flag          = d_valid ? d_valid + s.lo[g] : (uint8_t *)NULL;
            if (with_cost && place == lexls::BoundsCheckPlacement::lds)
                hipLaunchKernelGGL((lsi_bounds_check_kernel<true, true>), dim3(ctx.B, tiles), dim3(64), lds, ctx.stream, x_lse, d_lbq, d_ubq, lexls_internal_cdata(ctx.h), d_var, counts,
                                   (uint32_t)RESIDENT_DIMS_STRIDE, lb.d_map, lb.d_meta, lb.d_shape, ctx.B, s.batch, s.lo[g], nrhs, s.nObj, (uint32_t)total, s.nVar, ctx.cap, s.per_data, d_x,
                                   d_viol, flag, s.group_mask(g), d_cost);
            else if (with_cost)
                hipLaunchKernelGGL((lsi_bounds_check_kernel<false, true>), dim3(ctx.B, tiles), dim3(64), lds, ctx.stream, x_lse, d_lbq, d_ubq, lexls_internal_cdata(ctx.h), d_var, counts,
                                   (uint32_t)RESIDENT_DIMS_STRIDE, lb.d_map, lb.d_meta, lb.d_shape, ctx.B, s.batch, s.lo[g], nrhs, s.nObj, (uint32_t)total, s.nVar, ctx.cap, s.per_data, d_x,
                                   d_viol, flag, s.group_mask(g), d_cost);
            else if (place == lexls::BoundsCheckPlacement::lds)
                hipLaunchKernelGGL(lsi_bounds_check_kernel<true>, dim3(ctx.B, tiles), dim3(64), lds, ctx.stream, x_lse, d_lbq, d_ubq, lexls_internal_cdata(ctx.h), d_var, counts,
                                   (uint32_t)RESIDENT_DIMS_STRIDE, lb.d_map, lb.d_meta, lb.d_shape, ctx.B, s.batch, s.lo[g], nrhs, s.nObj, (uint32_t)total, s.nVar, ctx.cap, s.per_data, d_x,
                                   d_viol, flag, s.group_mask(g), (double *)NULL);
            else
                hipLaunchKernelGGL(lsi_bounds_check_kernel<false>, dim3(ctx.B, tiles), dim3(64), lds, ctx.stream, x_lse, d_lbq, d_ubq, lexls_internal_cdata(ctx.h), d_var, counts,
                                   (uint32_t)RESIDENT_DIMS_STRIDE, lb.d_map, lb.d_meta, lb.d_shape, ctx.B, s.batch, s.lo[g], nrhs, s.nObj, (uint32_t)total, s.nVar, ctx.cap, s.per_data, d_x,
                                   d_viol, flag, s.group_mask(g), (double *)NULL);
            if (hipGetLastError() != hipSuccess) throw Exception("lsi_bounds_check_kernel launch failed");
        }
        bounds_kernel = with_cost ? lexls::bounds_cost_placement_name(place) : lexls::bounds_check_placement_name(place);
        for (uint32_t g = 0; g < s.nGroups; g++)
            if (hipStreamSynchronize(s.grp[g]->stream) != hipSuccess) throw Exception(who + ": stream synchronisation failed");
        if (!on_device)
        {
            bool ok = !x || hipMemcpy(x, d_x, x_bytes, hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && with_cost) ok = hipMemcpy(cost, d_cost, c_bytes, hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && violation) ok = hipMemcpy(violation, d_viol, v_bytes, hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && valid) ok = hipMemcpy(valid, d_valid, s.batch, hipMemcpyDeviceToHost) == hipSuccess;
            if (!ok) throw Exception(who + ": hipMemcpy failed (results)");
        }
        return LEXLS_OK;
    }
};
